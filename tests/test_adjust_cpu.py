"""Anchor adjustment, CPU side (include/bloomscene_adjust.h): the header / ctypes table / library agreement, the refusals
of the two entry points, the scratch size function, the restatements of tests/adjust_reference.py against torch's CPU
evaluation of the decision lines and of the whole function, and the Python layer's import and error order without a GPU.
Every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adjust_reference as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bsr_adjust_decide", "bsr_adjust_decide_scratch_bytes", "bsr_rows_resize", "bsr_resize_max_tensors"}


def test_header_ctypes_table_and_library_agree():
    from bloomscene_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "bloomscene_adjust.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    declared = set(re.findall(r"\b(bsr_[a-z_]+)\s*\(", flat))
    assert declared == NAMES
    lib = ctypes.CDLL(os.path.join(ROOT, "bloomscene_amd", "libbloomscene_rast.so"))
    for name in declared:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
        params = re.search(name + r"\s*\(([^)]*)\)", flat).group(1)
        count = 0 if params.strip() == "void" else len(params.split(","))
        assert count == len(_capi.SIGNATURES[name][1]), name
    # the struct: one ctypes field per declared member, in order
    body = re.search(r"typedef struct bsr_resize_tensor \{(.*?)\} bsr_resize_tensor;", flat).group(1)
    members = [m.strip().split()[-1].lstrip("*") for m in body.split(";") if m.strip()]
    assert members == [f[0] for f in _capi.ResizeTensor._fields_]
    # the constants the Python layer repeats
    from bloomscene_amd import adjust as A
    consts = {k: int(v, 0) for k, v in re.findall(r"#define (BSR_[A-Z_]+)\s+(0x[0-9a-f]+|\d+)", hdr)}
    assert [consts["BSR_RESIZE_" + n] for n in ("COPY", "ZERO_FLAGGED", "CLAMP_FROM")] == \
        [A.RESIZE_COPY, A.RESIZE_ZERO_FLAGGED, A.RESIZE_CLAMP_FROM] == [0, 1, 2]
    assert (consts["BSR_ADJUST_MAX_K"], consts["BSR_ADJUST_MAX_LEVELS"], consts["BSR_RESIZE_MAX_WIDTH"]) == \
        (A.MAX_K, A.MAX_LEVELS, A.MAX_WIDTH)
    assert (consts["BSR_ADJUST_OFFSET_VALID"], consts["BSR_ADJUST_ANCHOR_PRUNE"], consts["BSR_ADJUST_ANCHOR_VALID"]) == \
        (A.OFFSET_VALID, A.ANCHOR_PRUNE, A.ANCHOR_VALID)
    lib.bsr_resize_max_tensors.restype = ctypes.c_int
    assert lib.bsr_resize_max_tensors() == consts["BSR_RESIZE_MAX_TENSORS"]
    assert lib.bsr_version() == 4                        # purely additive


def test_scratch_bytes_monotone_and_aligned():
    lib = ctypes.CDLL(os.path.join(ROOT, "bloomscene_amd", "libbloomscene_rast.so"))
    fn = lib.bsr_adjust_decide_scratch_bytes
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int]
    prev = 0
    for N in [1, 2, 1023, 1024, 1025, 4096, 100_000, 131_073, 2_600_000, 10 ** 8, 2 ** 31 - 1]:
        b = fn(N)
        blocks = -(-N // 1024)
        assert b % 256 == 0 and b >= prev and b >= 4 * (2 * blocks + -(-N * 16 // 1024)), (N, b)
        assert b <= 4 * 18 * blocks + 256, (N, b)
        prev = b
    assert fn(0) == 0 and fn(-1) == 0 and fn(-2 ** 31) == 0


def _decide(lib, N=4, K=2, L=1, thr=(0.1,), scalars=(40.0, 80.0, 0.005), ptrs=(1,) * 10):
    """A bsr_adjust_decide call with fake non-NULL device pointers (256: aligned): only for calls that are refused."""
    p = [256 if x else None for x in ptrs]
    arr = (ctypes.c_double * max(len(thr), 1))(*thr) if thr is not None else None
    return lib.bsr_adjust_decide(N, K, p[0], p[1], p[2], p[3], L, arr, *scalars, p[4], p[5], p[6], p[7], p[8], None)


def test_decide_refuses_bad_arguments_without_touching_the_gpu():
    from bloomscene_amd import _capi
    lib = _capi.lib()
    err = _capi.last_error
    assert _decide(lib, N=-1) == 1 and "N must be >= 0" in err()
    assert _decide(lib, K=0) == 1 and "K must be in [1, 16]" in err()
    assert _decide(lib, K=17) == 1 and "K must be in [1, 16]" in err()
    assert _decide(lib, N=2 ** 30, K=2) == 1 and "below 2^31" in err()
    assert _decide(lib, L=0) == 1 and "L must be in [1, 7]" in err()
    assert _decide(lib, L=8, thr=(0.1,) * 8) == 1 and "L must be in [1, 7]" in err()
    assert _decide(lib, thr=None) == 1 and "NULL thresholds" in err()
    assert _decide(lib, thr=(float("nan"),)) == 1 and "thresholds[0] is NaN" in err()
    assert _decide(lib, scalars=(float("nan"), 80.0, 0.005)) == 1 and "offset_count_min is NaN" in err()
    assert _decide(lib, scalars=(40.0, float("nan"), 0.005)) == 1 and "anchor_count_min is NaN" in err()
    assert _decide(lib, scalars=(40.0, 80.0, float("nan"))) == 1 and "min_opacity is NaN" in err()
    for k, what in [(0, "NULL statistic"), (3, "NULL statistic"), (4, "NULL output"), (5, "NULL output"), (6, "NULL output"),
                    (7, "NULL status"), (8, "NULL scratch")]:
        ptrs = [1] * 10
        ptrs[k] = 0
        assert _decide(lib, ptrs=ptrs) == 1 and what in err(), (k, err())
    # nothing to decide: no launch, no error
    assert _decide(lib, N=0, ptrs=[0] * 7 + [1, 0, 0]) == 0 and err() == ""


def _tensor(**kw):
    from bloomscene_amd._capi import ResizeTensor
    t = ResizeTensor()
    t.src, t.dst, t.append, t.flags, t.width = 4096, 1 << 20, None, None, 4
    t.flags_per_element, t.flag_mask, t.fill, t.op, t.clamp_col, t.clamp = 0, 0, 0, 0, 0, 0.0
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _resize(lib, tensors, N=8, n_keep=4, A=2, src_of=256):
    from bloomscene_amd._capi import ResizeTensor
    arr = (ResizeTensor * max(len(tensors), 1))(*tensors) if tensors is not None else None
    return lib.bsr_rows_resize(len(tensors) if tensors is not None else 1, arr, N, n_keep, A, src_of, None)


def test_rows_resize_refuses_bad_arguments_without_touching_the_gpu():
    from bloomscene_amd import _capi
    lib = _capi.lib()
    err = _capi.last_error
    assert lib.bsr_rows_resize(-1, None, 8, 4, 2, 256, None) == 1 and "n_tensors >= 0" in err()
    assert _resize(lib, None) == 1 and "NULL tensor array" in err()
    assert _resize(lib, [_tensor()], N=-1) == 1 and "N must be >= 0" in err()
    assert _resize(lib, [_tensor()], n_keep=-1) == 1 and "n_keep must be >= 0" in err()
    assert _resize(lib, [_tensor()], A=-1) == 1 and "A must be >= 0" in err()
    assert _resize(lib, [_tensor()], n_keep=9) == 1 and "n_keep must be <= N" in err()
    assert _resize(lib, [_tensor()], src_of=None) == 1 and "NULL src_of" in err()
    assert _resize(lib, [_tensor(), _tensor(width=0)]) == 1 and "tensor 1: width" in err()
    assert _resize(lib, [_tensor(width=1025)]) == 1 and "width must be in [1, 1024]" in err()
    assert _resize(lib, [_tensor(op=3)]) == 1 and "unknown op 3" in err()
    assert _resize(lib, [_tensor(op=-1)]) == 1 and "unknown op -1" in err()
    assert _resize(lib, [_tensor(width=1024)], N=2 ** 21, n_keep=2 ** 21, A=0) == 1 and "below 2^31" in err()
    assert _resize(lib, [_tensor(dst=None)]) == 1 and "NULL dst" in err()
    assert _resize(lib, [_tensor(src=None)]) == 1 and "NULL src" in err()
    assert _resize(lib, [_tensor(op=1)]) == 1 and "NULL flags" in err()
    assert _resize(lib, [_tensor(op=1, flags=512, flag_mask=0x100)]) == 1 and "flag_mask" in err()
    assert _resize(lib, [_tensor(op=2, clamp_col=5)]) == 1 and "clamp_col" in err()
    assert _resize(lib, [_tensor(src=4098)]) == 1 and "4-byte aligned" in err()
    assert _resize(lib, [_tensor(dst=4096 + 64)]) == 1 and "overlaps" in err()
    assert _resize(lib, [_tensor(), _tensor(src=1 << 21, dst=1 << 22, append=(1 << 20) + 16)]) == 1 and "overlaps" in err()
    # nothing to do: no launch, no error
    assert lib.bsr_rows_resize(0, None, 8, 4, 2, 256, None) == 0
    assert _resize(lib, [_tensor()], N=0, n_keep=0, A=0, src_of=None) == 0
    assert _resize(lib, [_tensor()], N=8, n_keep=0, A=0) == 0
    assert err() == ""


# ---- the restatement of A against torch's CPU evaluation of the decision lines ----

@pytest.mark.parametrize("K,depth,factor", [(1, 1, 4), (10, 3, 4), (16, 7, 4), (10, 3, 6)])
def test_decide_restatement_equals_torch_cpu_on_every_boundary(K, depth, factor):
    ci, st, thr, mo = 100, 0.8, 0.0002, 0.005
    thresholds = [thr * ((factor // 2) ** i) for i in range(depth)]
    s, d, acc, den = AR.boundary_stats(K, thresholds, ci, st, mo)
    flags, aflags, src_of, status = AR.decide_ref(s, d, acc, den, K, thresholds, ci, st, mo)
    # torch, in this test's own lines
    accum, denom = torch.from_numpy(acc).view(-1, 1), torch.from_numpy(den).view(-1, 1)
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    norm = torch.norm(grads, dim=-1)
    offset_mask = (denom > ci * st * 0.5).squeeze(dim=1)
    want = offset_mask.to(torch.uint8) * 128
    for i in range(depth):
        want |= (torch.logical_and(norm >= thr * ((factor // 2) ** i), offset_mask)).to(torch.uint8) << i
    assert np.array_equal(flags, want.numpy())
    opacity_accum, anchor_demon = torch.from_numpy(s).view(-1, 1), torch.from_numpy(d).view(-1, 1)
    prune = (opacity_accum < mo * anchor_demon).squeeze(dim=1)
    anchors_mask = (anchor_demon > ci * st).squeeze(dim=1)
    prune = torch.logical_and(prune, anchors_mask)
    assert np.array_equal(aflags, (prune.to(torch.uint8) | (anchors_mask.to(torch.uint8) << 1)).numpy())
    assert np.array_equal(src_of, (~prune).nonzero().squeeze(1).numpy())
    assert status == [int((~prune).sum()), int(anchors_mask.sum()), int(offset_mask.sum()), 0]
    # the boundaries are where the header says: on the threshold counts, one ulp below does not
    assert not flags[0] & 1 and flags[0] & 128                         # g one ulp below fl32(t0)
    assert flags[3] & 1 and flags[5] & 1 and flags[6] & 1              # g = fl32(t0), -fl32(t0), one ulp above
    assert flags[4] == 0                                               # the same g with a count of 32: not looked at
    assert torch.norm(torch.tensor([[3.3e-23]]), dim=-1).item() == np.float32(3.3e-23)   # |q|, not sqrtf(q q)


# ---- the restatement of the whole function against a torch-CPU run of the same sequence ----

def _compare(model, want):
    got = model.state()
    for name in AR.PARAMS:
        assert AR.F32 == got["params"][name].dtype
        assert np.array_equal(got["params"][name].view(np.uint32), want["params"][name].view(np.uint32)), name
    assert set(got["moments"]) == set(want["moments"])
    for name, pair in want["moments"].items():
        for a, b in zip(got["moments"][name], pair):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    for name in ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom", "max_radii2D"):
        assert got[name].shape == want[name].shape and np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), name


@pytest.mark.parametrize("level0", [True, False])
def test_whole_function_restatement_equals_torch_cpu(level0):
    N, F, K = 300, 8, 4
    state = AR.make_state(N, F, K, seed=3, grow=0.3)
    rng = np.random.default_rng(9)
    rand = [rng.random(N * K).astype(np.float32) for _ in range(3)]
    if not level0:
        rand[0][:] = 0.25                                              # no level-0 candidate: levels 1 and 2 must add nothing
    model = AR.Model(state, "cpu", lambda groups: torch.optim.Adam(groups, lr=0.0, eps=1e-15))
    model.two_steps()
    before = model.state()
    names = before["names"]
    assert set(before["moments"]) == set(AR.PARAMS) - {"opacity", "rotation"} and "mlp_opacity" in names
    want, levels = AR.adjust_anchor_ref(before, model, rand, rule="divide")
    assert (levels[0] > 0) == level0
    if level0:
        assert levels[1] > 0 and levels[2] > 0
    else:
        assert levels == [0, 0, 0]
    AR.eager_adjust(model, rand=[torch.from_numpy(r) for r in rand])
    _compare(model, want)
    after = model.state()
    n_new = after["params"]["anchor"].shape[0]
    assert after["names"] == names and after["steps"] == before["steps"] == {n: 2.0 for n in before["moments"]}
    assert 0 < N - n_new + sum(levels) < N and (n_new == N - (N - n_new + sum(levels)) + sum(levels))
    assert (after["params"]["scaling"][:, 3:] <= np.float32(0.05)).all() and (after["params"]["scaling"][:, 3:] == np.float32(0.05)).any()


def test_resize_restatement_on_a_hand_written_case():
    src = np.arange(12, dtype=np.float32).reshape(4, 3)
    src_of = np.array([3, 0, 9, -1], np.int32)
    out = AR.resize_ref(src, src_of, 4, 2, fill=np.array([7.0], np.float32).view(np.uint32)[0]).view(np.float32)
    assert out.tolist() == [[9, 10, 11], [0, 1, 2], [0, 0, 0], [0, 0, 0], [7, 7, 7], [7, 7, 7]]
    flags = np.array([0, 2, 0, 0, 0, 0, 0, 0, 0, 0x82, 0, 0], np.uint8)
    out = AR.resize_ref(src, src_of, 2, 0, op=("zero_flagged", flags, 0x80, True)).view(np.float32)
    assert out.tolist() == [[0, 10, 11], [0, 1, 2]]
    out = AR.resize_ref(src, src_of, 2, 0, op=("zero_flagged", flags[:4], 2, False)).view(np.float32)
    assert out.tolist() == [[9, 10, 11], [0, 1, 2]]
    src[3] = [np.nan, 10.0, 10.5]
    out = AR.resize_ref(src, src_of, 2, 1, append=np.array([[50, 60, 1]], np.float32), op=("clamp_from", 1, 10.0)).view(np.float32)
    assert np.isnan(out[0, 0]) and out[0, 1:].tolist() == [10, 10] and out[2].tolist() == [50, 10, 1]


def test_module_imports_without_a_gpu_and_raises_in_the_siblings_order():
    import bloomscene_amd.adjust as A
    s, d, acc, den = (torch.zeros(4), torch.zeros(4), torch.zeros(8), torch.zeros(8))
    with pytest.raises(TypeError, match="offset_denom must be float32"):
        A.decide(s[:3], d, acc, den.double(), 2, [0.1])
    with pytest.raises(TypeError, match="K must be an int"):
        A.decide(s[:3], d, acc, den, 2.0, [0.1])
    with pytest.raises(ValueError, match=r"K must be in \[1, 16\]"):
        A.decide(s, d, acc, den, 17, [0.1])
    with pytest.raises(ValueError, match="1 to 7 thresholds"):
        A.decide(s, d, acc, den, 2, [])
    with pytest.raises(ValueError, match=r"anchor_demon must be \[4\]"):
        A.decide(s, d[:3], acc, den, 2, [0.1])
    with pytest.raises(ValueError, match="no CPU path"):
        A.decide(s, d, acc, den, 2, [0.1])
    t, src_of = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(TypeError, match=r"tensors\[0\] must be float32 or int32"):
        A.resize_rows([t.double()], src_of.long(), 9)
    with pytest.raises(TypeError, match="src_of must be int32"):
        A.resize_rows([t], src_of.long(), 9)
    with pytest.raises(TypeError, match=r"appends\[0\] must be float32"):
        A.resize_rows([t], src_of, 9, appends=[torch.zeros(2, 3, dtype=torch.int32)])
    with pytest.raises(TypeError, match="flags must be uint8"):
        A.resize_rows([t], src_of, 9, ops=[("zero_flagged", torch.zeros(4), 1, False)])
    with pytest.raises(ValueError, match="one entry per tensor"):
        A.resize_rows([t], src_of, 2, fills=[0.0, 1.0])
    with pytest.raises(ValueError, match=r"n_keep must be in \[0, 4\]"):
        A.resize_rows([t], src_of, 9)
    with pytest.raises(ValueError, match=r"tensors\[1\] must have 4 rows"):
        A.resize_rows([t, torch.zeros(5, 3)], src_of, 2)
    with pytest.raises(ValueError, match="1 to 1024 elements"):
        A.resize_rows([torch.zeros(4, 1025)], src_of, 2)
    with pytest.raises(ValueError, match="flags must have 12 elements"):
        A.resize_rows([t], src_of, 2, ops=[("zero_flagged", torch.zeros(4, dtype=torch.uint8), 1, True)])
    with pytest.raises(ValueError, match="unknown op"):
        A.resize_rows([t], src_of, 2, ops=[("scale", 2.0)])
    with pytest.raises(ValueError, match="no CPU path"):
        A.resize_rows([t], src_of, 2)
    # quantize_anchor is eager torch: it runs anywhere, and is the lattice of the restatement
    x = torch.from_numpy(AR.make_state(50, 4, 2)["params"]["anchor"])
    lo, hi = x.min(dim=0, keepdim=True)[0] - 0.1, x.max(dim=0, keepdim=True)[0] + 0.1
    from anchor_state_reference import quantize_anchor_np
    assert np.array_equal(A.quantize_anchor(x, lo, hi).numpy(), quantize_anchor_np(x.numpy(), lo.numpy(), hi.numpy()))
    # resize_optimizer on a CPU optimizer: the state moves, step is inherited, a stateless group stays stateless
    model = AR.Model(AR.make_state(6, 4, 2), "cpu", lambda groups: torch.optim.Adam(groups, lr=0.0, eps=1e-15))
    model.two_steps()
    opt = model.optimizer
    new_p = {n: torch.zeros((3,) + tuple(getattr(model, "_" + n).shape[1:])) for n in AR.PARAMS}
    new_m = {n: (torch.ones_like(new_p[n]), torch.ones_like(new_p[n]) * 2) for n in AR.PARAMS}
    mlp_before = opt.param_groups[3]["params"][0]
    out = A.resize_optimizer(opt, new_p, new_m)
    assert set(out) == set(AR.PARAMS) and opt.param_groups[3]["params"][0] is mlp_before and len(opt.state) == 6
    for g in opt.param_groups:
        p = g["params"][0]
        if g["name"] in ("opacity", "rotation"):
            assert p not in opt.state and p.shape[0] == 3
        elif g["name"] in AR.PARAMS:
            st = opt.state[p]
            assert float(st["step"]) == 2.0 and (st["exp_avg"] == 1).all() and (st["exp_avg_sq"] == 2).all() and p is out[g["name"]]
