"""ctypes binding of ``libbloomscene_rast.so``: the C ABI the headers under ``include/`` declare (``SIGNATURES`` names
each).

The library is built in-tree (``bloomscene_amd/csrc/Makefile``, hipcc --offload-arch=gfx950).
There is deliberately NO fallback: if the shared object is missing or a call fails, this module
raises -- the product path never routes through the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbloomscene_rast.so")
CSRC = os.path.join(_HERE, "csrc")

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)

_F = C.c_void_p  # device pointer
ABI_VERSION = 4  # BSR_VERSION of include/bloomscene_rast.h this binding was written against
# use_library(..., allow_older_abi=True): 2 -> 3 only added entry points; 3 -> 4 dropped bsr_set_option / bsr_get_option (not
# bound here any more) and added flag bits -- every entry point bound below has the same signature in all three
# (tests/helpers.decode_buffers parses the image-buffer and hist1 layout of ABI 4 only, and the numerics(test_flags=...) bits
# are unknown flags to an older library: A/B runs against one must do without both)
OLDER_ABI_ACCEPTED = frozenset({2, 3})


class StageProfile(C.Structure):
    _fields_ = [("name", C.c_char_p), ("total_ms", C.c_double), ("launches", C.c_int)]


class AdamTensor(C.Structure):
    """``bsr_adam_tensor`` of ``include/bloomscene_adam.h``."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("numel", C.c_longlong),
                ("lr", C.c_double), ("step", C.c_longlong), ("lr_dev", C.c_void_p), ("step_dev", C.c_void_p)]


class ResizeTensor(C.Structure):
    """``bsr_resize_tensor`` of ``include/bloomscene_adjust.h``."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("append", C.c_void_p), ("flags", C.c_void_p), ("width", C.c_int),
                ("flags_per_element", C.c_int), ("flag_mask", C.c_uint), ("fill", C.c_uint), ("op", C.c_int),
                ("clamp_col", C.c_int), ("clamp", C.c_float)]


# name -> (restype, argtypes); every symbol include/*.h declares
SIGNATURES = {
    "bsr_version": (C.c_int, []),
    "bsr_last_error": (C.c_char_p, []),
    "bsr_mark_visible": (C.c_int, [C.c_int, _F, _F, _F, _F, C.c_void_p]),
    "bsr_forward": (C.c_int, [ALLOC_FN, C.c_void_p, ALLOC_FN, C.c_void_p, ALLOC_FN, C.c_void_p,
                              C.c_int, C.c_int, C.c_int, _F, C.c_int, C.c_int, _F, _F, _F, _F, _F, C.c_float, _F, _F,
                              _F, _F, _F, C.c_float, C.c_float, C.c_int, _F, _F, _F, C.c_int, C.c_void_p,
                              C.POINTER(C.c_int)]),
    "bsr_forward_ex": (C.c_int, [ALLOC_FN, C.c_void_p, ALLOC_FN, C.c_void_p, ALLOC_FN, C.c_void_p,
                                 C.c_int, C.c_int, C.c_int, _F, C.c_int, C.c_int, _F, _F, _F, _F, _F, C.c_float, _F, _F,
                                 _F, _F, _F, C.c_float, C.c_float, C.c_int, _F, _F, _F, C.c_int, C.c_void_p,
                                 C.POINTER(C.c_int)] + [C.c_uint]),
    "bsr_forward_views": (C.c_int, [ALLOC_FN, C.c_void_p, ALLOC_FN, C.c_void_p, ALLOC_FN, C.c_void_p,
                                    C.c_int, C.c_int, C.c_int, C.c_int, _F, C.c_int, C.c_int, _F, _F, _F, _F, _F,
                                    C.c_float, _F, _F, _F, _F, _F, C.c_float, C.c_float, C.c_int, _F, _F, _F, C.c_int,
                                    C.c_void_p, C.POINTER(C.c_int), C.c_uint]),
    "bsr_visible_filter": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F, _F, C.c_float, _F, _F, _F, _F,
                                     C.c_float, C.c_float, C.c_int, _F, C.c_int, C.c_void_p]),
    "bsr_visible_scratch_bytes": (C.c_size_t, [C.c_int]),
    "bsr_visible_filter_indices": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F, _F, C.c_float, _F, _F, _F, _F,
                                             C.c_float, C.c_float, C.c_int, _F, _F, _F, C.POINTER(C.c_int), C.c_int,
                                             C.c_void_p]),
    "bsr_visible_filter_views": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F, _F, C.c_float, _F, _F, _F, _F,
                                           C.c_float, C.c_float, _F, C.c_int, C.c_void_p]),
    "bsr_visible_groups_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "bsr_visible_filter_groups": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F, _F, C.c_float, _F, _F, _F, _F,
                                            C.c_float, C.c_float, _F, _F, _F, _F, C.c_int, C.c_void_p]),
    "bsr_pack_rows": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), _F, C.c_int, _F, C.c_int,
                                C.c_void_p]),
    "bsr_gather_rows": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), _F, C.c_int,
                                  C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    "bsr_backward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F, C.c_int, C.c_int, _F, _F, _F, _F, C.c_float,
                               _F, _F, _F, _F, _F, C.c_float, C.c_float, _F, _F, _F, _F, _F, _F, _F, _F, _F, _F, _F,
                               _F, _F, _F, _F, C.c_int, C.c_void_p]),
    "bsr_backward_depth": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F, C.c_int, C.c_int, _F, _F, _F, _F, C.c_float,
                                     _F, _F, _F, _F, _F, C.c_float, C.c_float, _F, _F, _F, _F, _F, _F, _F, _F, _F, _F,
                                     _F, _F, _F, _F, _F, _F, C.c_int, C.c_void_p]),
    "bsr_backward_ex": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F, C.c_int, C.c_int, _F, _F, _F, _F, C.c_float,
                                  _F, _F, _F, _F, _F, C.c_float, C.c_float, _F, _F, _F, _F, _F, _F, _F, _F, _F, _F,
                                  _F, _F, _F, _F, _F, _F, C.c_int, C.c_void_p, C.c_uint]),
    "bsr_read_counts": (C.c_int, [_F, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bsr_check_deferred": (C.c_int, []),
    "bsr_geometry_bytes": (C.c_size_t, [C.c_int]),
    "bsr_binning_bytes": (C.c_size_t, [C.c_int]),
    "bsr_image_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "bsr_transmittance_offset": (C.c_size_t, [C.c_void_p]),
    "bsr_profile_enable": (C.c_int, [C.c_int]),
    "bsr_profile_only": (C.c_int, [C.c_char_p]),
    "bsr_profile_reset": (C.c_int, []),
    "bsr_profile_read": (C.c_int, [C.POINTER(StageProfile), C.c_int]),
    # include/bloomscene_anchors.h
    "bsr_anchor_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "bsr_anchor_select": (C.c_int, [C.c_int, C.c_int, _F, _F, _F, C.POINTER(C.c_int), C.c_void_p]),
    "bsr_anchor_expand": (C.c_int, [C.c_int, C.c_int, C.c_int] + [_F] * 12 + [C.c_void_p]),
    "bsr_anchor_expand_backward": (C.c_int, [C.c_int, C.c_int, C.c_int] + [_F] * 16 + [C.c_void_p]),
    "bsr_anchor_gaussian_bytes": (C.c_size_t, [C.c_int]),
    "bsr_anchor_gradient_bytes": (C.c_size_t, [C.c_int]),
    "bsr_anchor_render_forward": (C.c_int, [C.c_int, C.c_int] + [_F] * 8 + [ALLOC_FN, C.c_void_p] * 4
                                  + [_F, C.c_int, C.c_int, C.c_float, _F, _F, _F, C.c_float, C.c_float, _F, _F, C.c_int,
                                     C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_uint]),
    "bsr_anchor_render_backward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int] + [_F] * 6 + [_F, _F, _F]
                                   + [_F, C.c_int, C.c_int, C.c_float, _F, _F, _F, C.c_float, C.c_float]
                                   + [_F] * 3 + [_F] * 5 + [_F] + [_F] * 6 + [C.c_int, C.c_void_p, C.c_uint]),
    # include/bloomscene_grid.h
    "bsr_grid_backward_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "bsr_grid_encode_forward": (C.c_int, [C.c_int] * 5 + [_F] * 6 + [C.c_void_p]),
    "bsr_grid_encode_backward": (C.c_int, [C.c_int] * 5 + [_F] * 7 + [C.c_void_p, C.c_void_p]),
    # include/bloomscene_mix_grid.h (host arrays of n_grids device pointers / ints: GridPointers, GridInts)
    "bsr_mix_grid_backward_scratch_bytes": (C.c_size_t, [C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int]),
    "bsr_mix_grid_forward": (C.c_int, [C.c_int] * 4 + [_F, C.c_longlong, _F, _F] + [C.POINTER(C.c_void_p)] * 3
                             + [C.POINTER(C.c_int)] * 4 + [_F, _F, C.c_void_p]),
    "bsr_mix_grid_backward": (C.c_int, [C.c_int] * 4 + [_F, C.c_longlong, _F, C.c_longlong, _F, _F]
                              + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_int)] * 4
                              + [_F, C.POINTER(C.c_void_p), _F, C.c_void_p, C.c_void_p]),
    # include/bloomscene_knn.h
    "bsr_knn_scratch_bytes": (C.c_size_t, [C.c_int]),
    "bsr_knn_mean_dist": (C.c_int, [C.c_int, _F, _F, C.c_void_p, C.c_void_p]),
    # include/bloomscene_densify.h
    "bsr_scatter_max": (C.c_int, [C.c_int] * 4 + [_F, _F, _F, C.c_longlong, C.c_longlong, _F, _F, C.c_void_p]),
    "bsr_voxel_isin_scratch_bytes": (C.c_size_t, [C.c_int]),
    "bsr_voxel_isin": (C.c_int, [C.c_int, C.c_int, _F, _F, _F, C.c_void_p, C.c_void_p]),
    # include/bloomscene_entropy.h
    "bsr_entropy_scratch_bytes": (C.c_size_t, [C.c_int] * 3),
    "bsr_entropy_forward": (C.c_int, [C.c_int] * 3 + [_F, C.c_longlong] * 3 + [_F, C.c_int, _F, _F, _F] + [_F] * 4
                            + [C.c_void_p, C.c_void_p]),
    "bsr_entropy_backward": (C.c_int, [C.c_int] * 3 + [_F, C.c_longlong] * 3 + [_F, C.c_int, _F, _F, _F] + [_F, C.c_int]
                             + [_F] * 5 + [C.c_void_p, C.c_void_p]),
    # include/bloomscene_loss.h
    "bsr_photometric_scratch_bytes": (C.c_size_t, [C.c_int] * 4),
    "bsr_photometric_forward": (C.c_int, [C.c_int] * 4 + [_F, _F, C.c_float, _F, _F, _F, C.c_void_p, C.c_void_p]),
    "bsr_photometric_backward": (C.c_int, [C.c_int] * 4 + [_F, _F, _F, C.c_float, _F, _F, C.c_void_p]),
    # include/bloomscene_depth_loss.h
    "bsr_depth_prior_scratch_bytes": (C.c_size_t, [C.c_int] * 2),
    "bsr_depth_prior_forward": (C.c_int, [C.c_int] * 2 + [_F] * 3 + [C.c_longlong] * 3 + [C.c_int] + [C.c_float] * 3 + [C.c_int]
                                + [_F] * 4 + [C.c_void_p]),
    "bsr_depth_prior_backward": (C.c_int, [C.c_int] * 2 + [_F] * 3 + [C.c_longlong] * 3 + [C.c_int] + [C.c_float] * 3 + [C.c_int]
                                 + [_F] * 4 + [C.c_void_p]),
    # include/bloomscene_heads.h (the two structs of twelve device pointers: HeadsPointers, passed by reference)
    "bsr_anchor_heads_scratch_bytes": (C.c_size_t, [C.c_int] * 3),
    "bsr_anchor_heads_forward": (C.c_int, [C.c_int] * 3 + [_F, C.c_longlong, _F, _F, _F, C.c_void_p] + [_F] * 4 + [C.c_void_p]),
    "bsr_anchor_heads_backward": (C.c_int, [C.c_int] * 3 + [_F, C.c_longlong, _F, _F, _F, C.c_void_p] + [_F] * 7
                                  + [C.c_void_p, C.c_void_p, C.c_void_p]),
    # include/bloomscene_context.h (the two structs of four device pointers: ContextPointers, passed by reference)
    "bsr_context_scratch_bytes": (C.c_size_t, [C.c_int] * 5),
    "bsr_context_head_forward": (C.c_int, [C.c_int] * 5 + [_F, C.c_longlong, C.c_void_p] + [C.c_float] * 3 + [_F, C.c_longlong] * 3
                                 + [_F] * 3 + [_F] * 2 + [_F] * 3 + [_F, C.c_void_p]),
    "bsr_context_head_backward": (C.c_int, [C.c_int] * 5 + [_F, C.c_longlong, C.c_void_p] + [C.c_float] * 3 + [_F] * 3 + [_F] * 5
                                  + [_F, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsr_context_quantise_forward": (C.c_int, [C.c_int] * 5 + [_F, C.c_longlong, C.c_void_p] + [C.c_float] * 3
                                     + [_F, C.c_longlong] * 3 + [_F] * 3 + [_F] + [_F] * 3 + [C.c_void_p]),
    # include/bloomscene_anchor_state.h
    "bsr_anchor_visible_forward": (C.c_int, [C.c_int] * 4 + [_F] * 5 + [C.c_longlong] + [_F] * 3 + [_F] * 7 + [C.c_void_p]),
    "bsr_anchor_visible_backward": (C.c_int, [C.c_int] * 4 + [_F] * 3 + [_F] * 5 + [_F] * 5 + [C.c_void_p]),
    "bsr_anchor_accumulate_scratch_bytes": (C.c_size_t, [C.c_int] * 2),
    "bsr_anchor_accumulate": (C.c_int, [C.c_int] * 4 + [_F] * 4 + [C.c_int] + [_F] * 5 + [C.c_void_p, C.c_void_p]),
    # include/bloomscene_codec.h
    "bsr_codec_stream_bound": (C.c_size_t, [C.c_longlong, C.c_int]),
    "bsr_codec_scratch_bytes": (C.c_size_t, [C.c_longlong, C.c_int]),
    "bsr_codec_encode_gaussian": (C.c_int, [C.c_int] * 3 + [_F, C.c_longlong] * 3 + [_F, C.c_int, _F, C.c_float, C.c_int]
                                  + [_F, C.c_size_t, _F, C.c_void_p, C.c_void_p]),
    "bsr_codec_decode_gaussian": (C.c_int, [C.c_int] * 3 + [_F, C.c_size_t] + [_F, C.c_longlong] * 2
                                  + [_F, C.c_int, _F, C.c_float, _F, _F, C.c_void_p]),
    "bsr_codec_encode_table": (C.c_int, [C.c_int] * 2 + [_F, _F, C.c_longlong, C.c_int, _F, C.c_size_t, _F, C.c_void_p,
                                                         C.c_void_p]),
    "bsr_codec_decode_table": (C.c_int, [C.c_int] * 2 + [_F, C.c_size_t, _F, C.c_longlong, _F, _F, C.c_void_p]),
    # include/bloomscene_anchor_codec.h
    "bsr_anchor_codec_stream_bound": (C.c_size_t, [C.c_int]),
    "bsr_anchor_codec_scratch_bytes": (C.c_size_t, [C.c_int]),
    "bsr_anchor_keys": (C.c_int, [C.c_int, C.c_int, _F, C.c_longlong] + [_F] * 5 + [C.c_void_p]),
    "bsr_anchor_codec_encode": (C.c_int, [C.c_int] + [_F] * 4 + [C.c_size_t, _F, C.c_void_p, C.c_void_p]),
    "bsr_anchor_codec_decode": (C.c_int, [C.c_int, _F, C.c_size_t] + [_F] * 4 + [C.c_void_p]),
    # include/bloomscene_adam.h (a host array of bsr_adam_tensor: AdamTensor)
    "bsr_adam_max_tensors": (C.c_int, []),
    "bsr_adam_step": (C.c_int, [C.c_int, C.POINTER(AdamTensor), C.c_double, C.c_double, C.c_double, C.c_void_p]),
    # include/bloomscene_voxelize.h (the source: form, rule, E, P, src, stride, anchor, scaling, stride, K, rows, voxel_size)
    "bsr_voxel_quantise": (C.c_int, [C.c_int] * 4 + [_F, C.c_longlong, _F, _F, C.c_longlong, C.c_int, _F, C.c_double]
                           + [_F, _F, C.c_void_p]),
    "bsr_voxel_unique_scratch_bytes": (C.c_size_t, [C.c_int]),
    "bsr_voxel_unique": (C.c_int, [C.c_int] * 4 + [_F, C.c_longlong, _F, _F, C.c_longlong, C.c_int, _F, C.c_double]
                         + [_F] * 7 + [C.c_uint, C.c_void_p]),
    # include/bloomscene_adjust.h (a host array of L doubles; a host array of bsr_resize_tensor: ResizeTensor)
    "bsr_adjust_decide_scratch_bytes": (C.c_size_t, [C.c_int]),
    "bsr_adjust_decide": (C.c_int, [C.c_int, C.c_int] + [_F] * 4 + [C.c_int, C.POINTER(C.c_double)] + [C.c_double] * 3
                          + [_F] * 4 + [C.c_void_p, C.c_void_p]),
    "bsr_resize_max_tensors": (C.c_int, []),
    "bsr_rows_resize": (C.c_int, [C.c_int, C.POINTER(ResizeTensor), C.c_int, C.c_int, C.c_int, _F, C.c_void_p]),
    # include/bloomscene_reproject.h (a host array of 21 doubles: the camera)
    "bsr_reproject_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "bsr_warp_points": (C.c_int, [C.c_int] * 3 + [_F, C.c_longlong, C.c_longlong, _F, C.POINTER(C.c_double), C.c_int, C.c_double]
                        + [_F] * 6 + [C.c_void_p]),
    "bsr_lift_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "bsr_lift_count": (C.c_int, [C.c_int, C.c_int, _F, _F, _F, C.c_void_p]),
    "bsr_lift_pixels": (C.c_int, [C.c_int, C.c_int, _F, _F, _F, C.POINTER(C.c_double), _F, _F, C.c_int, _F, _F, C.c_void_p]),
}

HeadsPointers = C.c_void_p * 12   # bsr_heads_weights / bsr_heads_weight_grads: (w1, b1, w2, b2) of opacity, cov, color
ContextPointers = C.c_void_p * 4  # bsr_context_weights / bsr_context_weight_grads: w1, b1, w2, b2

_lib = None
_allow_older_abi = False   # use_library(..., allow_older_abi=True): A/B runs against a library of an earlier round


def build(force: bool = False) -> str:
    """Compile the HIP library for gfx950 (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j8"] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    """Load the library; raises (never falls back) if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `make -C {CSRC}` (or __graft_entry__.build()). "
                "bloomscene_amd has no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        # a stale build of another ABI version would shift arguments silently (several entry points changed their
        # parameter lists in place between versions): refuse it before binding anything
        handle.bsr_version.restype = C.c_int
        # (only 2 -> 3 was additive; a version-1 library bound with these signatures would shift arguments silently)
        older = handle.bsr_version() in OLDER_ABI_ACCEPTED and _allow_older_abi
        if handle.bsr_version() != ABI_VERSION and not older:
            raise RuntimeError(f"{LIB_PATH} is ABI version {handle.bsr_version()}, this binding needs {ABI_VERSION}: "
                               f"rebuild it (make -C {CSRC})")
        for name, (res, args) in SIGNATURES.items():
            if older and not hasattr(handle, name):
                continue   # (an entry point the older library does not have: calling it raises AttributeError)
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def use_library(path: str, allow_older_abi: bool = False):
    """Measurement tools only (A/B runs of two builds on one GPU box, the diagnostic builds of csrc/Makefile): load
    another build of the SAME C ABI instead of the in-tree product library.  Must precede the first native call of
    the process; the product never calls this and reads no environment variable to find its library.
    ``allow_older_abi``: accept a library of an EARLIER ABI version whose entry points kept their parameter lists
    (version 2 -> 3 added symbols and flags only: INTEGRATION.md "ABI versions") -- for A/B runs against an earlier
    round's build; entry points it lacks are simply not bound."""
    global LIB_PATH, _allow_older_abi
    if _lib is not None:
        raise RuntimeError("use_library() must be called before the library is first used")
    LIB_PATH = os.path.abspath(path)
    _allow_older_abi = bool(allow_older_abi)


def last_error() -> str:
    return lib().bsr_last_error().decode("utf-8", "replace")


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {last_error()}")


def call(name: str, *args):
    """Call the entry point ``name`` (an int status) and raise RuntimeError naming it if the status is not 0."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        check(rc, name)


def profile_enable(on):
    """False/0: off; True/1: bracket every stage with events; N > 1: only every Nth forward (+ its backward)."""
    lib().bsr_profile_enable(int(on))


def profile_only(stage=None):
    """Bracket only this stage ("render_bwd", ...); None: all stages again."""
    lib().bsr_profile_only(stage.encode() if stage else None)


def profile_reset():
    lib().bsr_profile_reset()


def profile_read():
    """-> {stage name: (total_ms, launches)} accumulated since the last reset."""
    arr = (StageProfile * 16)()
    n = lib().bsr_profile_read(arr, 16)
    return {arr[i].name.decode(): (arr[i].total_ms, arr[i].launches) for i in range(n)}
