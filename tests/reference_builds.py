"""Loader of the reference's own kernels, as built into oracle/_ref/ by oracle/reference_build.py (test infrastructure).

Everything comes from oracle/_ref/MANIFEST.json; the reference tree itself is never read here.  `skip_if_missing()` skips a
test only when the manifest says "reference_missing".  No manifest, a listed binary that does not load, an expected build
that is not listed and a binary without its entry point all raise ReferenceBuildError: a failure, not a skip.

The reference's kernels have none of the guards of include/bloomscene_*.h: hand them well-formed inputs only
(P >= 1; tables whose offsets[-1] is the embedding row count).  The checks below refuse anything else.
"""
from __future__ import annotations

import ctypes
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
MANIFEST = os.path.join(REF_DIR, "MANIFEST.json")
BUILDS = ("strict", "contract")

_cache = {}


class ReferenceBuildError(RuntimeError):
    pass


def manifest() -> dict:
    if "manifest" not in _cache:
        if not os.path.exists(MANIFEST):
            raise ReferenceBuildError("oracle/_ref/MANIFEST.json does not exist: run build() (oracle/reference_build.py)")
        with open(MANIFEST) as f:
            _cache["manifest"] = json.load(f)
    return _cache["manifest"]


def reference_missing() -> bool:
    return manifest().get("reference_missing") is True


def skip_if_missing():
    """The only skip there is: build() found no reference tree and said so in the manifest."""
    if reference_missing():
        import pytest
        pytest.skip("oracle/_ref/MANIFEST.json: reference_missing (build() found no reference tree to build)")


def _entry(name: str) -> dict:
    b = manifest().get("builds", {})
    if name not in b:
        raise ReferenceBuildError(f"oracle/_ref/MANIFEST.json lists no build '{name}' (it lists {sorted(b)})")
    path = os.path.join(REF_DIR, b[name]["path"])
    if not os.path.exists(path):
        raise ReferenceBuildError(f"{path} is listed in the manifest and does not exist")
    return dict(b[name], abspath=path)


def knn_library(build: str = "strict"):
    assert build in BUILDS, build
    key = "knn_" + build
    if key not in _cache:
        e = _entry(key)
        import torch  # noqa: F401  (the HIP runtime of the process is torch's: load it first)
        try:
            lib = ctypes.CDLL(e["abspath"])
        except OSError as err:
            raise ReferenceBuildError(f"{e['abspath']} does not load: {err}") from err
        for s in e["symbols"]:
            if not hasattr(lib, s):
                raise ReferenceBuildError(f"{e['abspath']} has no symbol {s}")
        lib.bsr_ref_knn.restype = ctypes.c_int
        lib.bsr_ref_knn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        _cache[key] = lib
    return _cache[key]


def grid_module(build: str = "strict"):
    assert build in BUILDS, build
    key = "grid_" + build
    if key not in _cache:
        e = _entry(key)
        import torch  # noqa: F401  (libtorch must be in the process before the module)
        try:
            spec = importlib.util.spec_from_file_location(e["module"], e["abspath"])
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        except (ImportError, OSError) as err:
            raise ReferenceBuildError(f"{e['abspath']} does not load: {err}") from err
        for s in e["symbols"]:
            if not hasattr(mod, s):
                raise ReferenceBuildError(f"{e['abspath']} has no function {s}")
        sys.modules.setdefault(e["module"], mod)
        _cache[key] = mod
    return _cache[key]


def ref_mean_dist3(points, build: str = "strict"):
    """The reference's SimpleKNN::knn on a float32 [P, 3] cuda tensor, P >= 1 -> float32 [P] (its distCUDA2)."""
    import torch
    lib = knn_library(build)
    if not (points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 3
            and points.shape[0] >= 1):
        raise ValueError("ref_mean_dist3: a float32 [P, 3] cuda tensor with P >= 1")
    p = points.contiguous()
    out = torch.zeros(p.shape[0], dtype=torch.float32, device=p.device)   # (distCUDA2 hands it torch.full({P}, 0))
    torch.cuda.synchronize()
    rc = lib.bsr_ref_knn(int(p.shape[0]), p.data_ptr(), out.data_ptr())    # the null stream; returns after a device sync
    if rc != 0:
        raise RuntimeError(f"ref_mean_dist3: hipDeviceSynchronize returned {rc}")
    return out


def _well_formed(who, inputs, embeddings, offsets_list, resolutions_list, N, num_dim, n_features, n_levels):
    import torch
    offs = offsets_list.cpu().tolist()
    ok = (inputs.is_cuda and embeddings.is_cuda and offsets_list.is_cuda and resolutions_list.is_cuda
          and inputs.dtype == torch.float32 and embeddings.dtype == torch.float32
          and offsets_list.dtype == torch.int32 and resolutions_list.dtype == torch.int32
          and tuple(inputs.shape) == (N, num_dim) and N >= 1 and embeddings.shape[1] == n_features
          and len(offs) == n_levels + 1 and resolutions_list.numel() == n_levels
          and all(0 <= a < b for a, b in zip(offs, offs[1:])) and offs[-1] <= embeddings.shape[0]
          and int(resolutions_list.min()) >= 3)
    if not ok:
        raise ValueError(f"{who}: the reference has no guards; refusing inputs that are not well-formed")


def ref_grid_forward(inputs, embeddings, offsets_list, resolutions_list, outputs, N, num_dim, n_features, n_levels,
                     max_level, Rb, PV, dy_dx, binary_vxl, min_level_id, build: str = "strict"):
    """The reference's grid_encode_forward, argument for argument (fp32 tensors on the GPU)."""
    import torch
    mod = grid_module(build)
    assert binary_vxl is None and min_level_id is None
    _well_formed("ref_grid_forward", inputs, embeddings, offsets_list, resolutions_list, N, num_dim, n_features, n_levels)
    assert outputs.numel() == n_levels * N * n_features and (dy_dx is None or dy_dx.numel() == N * n_levels * num_dim * n_features)
    torch.cuda.synchronize()
    mod.grid_encode_forward(inputs, embeddings, offsets_list, resolutions_list, outputs, N, num_dim, n_features, n_levels,
                            max_level, Rb, PV, dy_dx, binary_vxl, min_level_id)
    torch.cuda.synchronize()


def ref_grid_backward(grad, inputs, embeddings, offsets_list, resolutions_list, grad_embeddings, N, num_dim, n_features,
                      n_levels, max_level, Rb, dy_dx, grad_inputs, binary_vxl, min_level_id, build: str = "strict"):
    """The reference's grid_encode_backward, argument for argument.  It ADDS into grad_embeddings: hand it zeros."""
    import torch
    mod = grid_module(build)
    assert binary_vxl is None and min_level_id is None
    _well_formed("ref_grid_backward", inputs, embeddings, offsets_list, resolutions_list, N, num_dim, n_features, n_levels)
    assert grad.dtype == torch.float32 and grad.numel() == n_levels * N * n_features and grad.is_contiguous()
    assert tuple(grad_embeddings.shape) == tuple(embeddings.shape) and grad_embeddings.is_contiguous()
    assert (dy_dx is None) == (grad_inputs is None)
    assert dy_dx is None or (dy_dx.numel() == N * n_levels * num_dim * n_features and grad_inputs.numel() == N * num_dim)
    torch.cuda.synchronize()
    mod.grid_encode_backward(grad, inputs, embeddings, offsets_list, resolutions_list, grad_embeddings, N, num_dim,
                             n_features, n_levels, max_level, Rb, dy_dx, grad_inputs, binary_vxl, min_level_id)
    torch.cuda.synchronize()
