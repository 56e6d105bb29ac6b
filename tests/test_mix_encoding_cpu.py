"""CPU tests of the fused mixed 3D/2D binary hash-grid encoding (include/bloomscene_mix_grid.h,
bloomscene_amd/mix_encoding.py): the restatement of tests/mix_encoding_reference.py against the composition it claims to
be and against the reference's own lines run in torch, the library's entry points, the python interface's checks in their
order, and the module's state dict -- all before the device is touched."""
import ctypes

import numpy as np
import pytest
import torch

import grid_reference as GR
import mix_encoding_reference as MR
from bloomscene_amd import _capi
from bloomscene_amd import mix_encoding as ME
from bloomscene_amd.grid_encoder import table_offsets

F32 = np.float32
RES_3D = (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514)   # scene/gaussian_model.py:134-135
RES_2D = (130, 258, 514, 1026)
BOUND_MIN, BOUND_MAX = (-3.0, -1.0, 0.5), (2.0, 4.0, 9.0)
HAND_MADE = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(F32(1), F32(2)), -np.nextafter(F32(1), F32(2)), np.nan, np.inf,
                      -np.inf, 1e-45], F32)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _tables(F, seed, res3=(18, 33), res2=(10, 40), spread=1.3):
    """Small tables with values on both sides of the gate (|p| up to `spread`)."""
    rng = np.random.default_rng(seed)
    tables = []
    for D, res, log2 in ((3, res3, 10), (2, res2, 8), (2, res2, 8), (2, res2, 8)):
        offs = np.array(table_offsets(D, res, log2), np.int64)
        tables.append((rng.uniform(-spread, spread, (int(offs[-1]), F)).astype(F32), offs, np.array(res, np.int64)))
    return tables


def _points(n, seed):
    """Points in the box of the bounds, with the grid's edge cases mapped through them: corners of the box, points outside
    in one coordinate (outside for three of the four grids only), border cells."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 1, (n, 3)).astype(F32)
    if n >= 64:
        u[0:4] = 0.0
        u[4:8] = 1.0
        u[8, 0] = -0.25
        u[9, 2] = 1.5
        u[10:20] = rng.uniform(0, 0.004, (10, 3)).astype(F32)
        u[20:30] = 1 - rng.uniform(0, 0.004, (10, 3)).astype(F32)
    lo, hi = np.array(BOUND_MIN, F32), np.array(BOUND_MAX, F32)
    return (lo + u * (hi - lo)).astype(F32)


@pytest.mark.parametrize("F", [1, 2])
def test_restatement_is_the_composition_grid_by_grid(F):
    tables = _tables(F, seed=F)
    n = 300
    x = _points(n, seed=3)
    u = ((x - np.array(BOUND_MIN, F32)) / (np.array(BOUND_MAX, F32) - np.array(BOUND_MIN, F32))).astype(F32)
    out, dy = MR.forward(x, tables, MR.MIX_DIMS, BOUND_MIN, BOUND_MAX)
    g_out = np.random.default_rng(5).normal(0, 1, out.shape).astype(F32)
    grads, grad_x = MR.backward(x, tables, MR.MIX_DIMS, g_out, dy, BOUND_MIN, BOUND_MAX, gated=False)
    gated, _ = MR.backward(x, tables, MR.MIX_DIMS, g_out, dy, BOUND_MIN, BOUND_MAX)
    outs, dys, r = [], [], {}
    c = 0
    for (p, offs, res), d in zip(tables, MR.MIX_DIMS):
        signs = np.where(p >= 0, F32(1), F32(-1))                      # the materialised STE_binary table (no NaN here)
        xg = np.ascontiguousarray(u[:, list(d)])
        o, dyg = GR.forward(xg, signs, offs, res)
        L = len(res)
        outs.append(o.transpose(1, 0, 2).reshape(n, L * F))
        dys.append(dyg.reshape(n, -1))
        g = np.ascontiguousarray(g_out[:, c:c + L * F].reshape(n, L, F).transpose(1, 0, 2))
        ge, gi, _ = GR.backward(xg, offs, res, p.shape[0], g, dyg)
        k = len(outs) - 1
        assert _bits_equal(grads[k], ge)
        assert _bits_equal(gated[k], np.where(np.abs(p) <= 1, ge, F32(0)))
        assert (np.abs(p) > 1).any() and (gated[k][np.abs(p) > 1] == 0).all()
        for j, dd in enumerate(d):
            r.setdefault(dd, []).append(gi[:, j])
        c += L * F
    assert _bits_equal(out, np.concatenate(outs, axis=1)) and _bits_equal(dy, np.concatenate(dys, axis=1))
    assert out.shape == (n, 8 * F) and np.abs(out).max() > 0
    # a point outside in x alone is outside for xyz, xy and xz and inside for yz
    assert (out[8, :6 * F] == 0).all() and np.abs(out[8, 6 * F:]).max() > 0
    for dd in range(3):
        assert len(r[dd]) == 3
        want = ((r[dd][0] + r[dd][1]) + r[dd][2]) / (F32(BOUND_MAX[dd]) - F32(BOUND_MIN[dd]))
        assert _bits_equal(grad_x[:, dd], want.astype(F32))


def test_sign_rule_and_gate_on_a_hand_made_table():
    want_sign = np.array([1, 1, 1, -1, 1, -1, 0, 1, -1, 1], F32)
    want_gate = np.array([1, 1, 1, 1, 0, 0, 0, 0, 0, 1], bool)
    assert _bits_equal(MR.sign_table(HAND_MADE), want_sign)            # bit-equal: the NaN's 0 is +0
    assert (MR.gate(HAND_MADE) == want_gate).all()
    # through the encoding: a one-level dense 1-D table whose rows are the hand-made values
    rows, res = 24, 18
    p = np.zeros((rows, 1), F32)
    p[1:11, 0] = HAND_MADE
    tables = [(p, np.array([0, rows]), np.array([res]))]
    x = np.zeros((10, 3), F32)
    x[:, 0] = (np.arange(1, 11, dtype=F32) - F32(0.5)) / F32(res - 2)   # pos = k exactly: weight 1 on row k, 0 on row k + 1
    out, dy = MR.forward(x, tables, ((0,),))
    assert _bits_equal(out[:10, 0], want_sign)
    g = np.full(out.shape, 1.0, F32)
    g[3] = np.nan
    grads, _ = MR.backward(x, tables, ((0,),), g, dy)
    got = grads[0][1:11, 0]
    assert np.isnan(got[3]) and (got[[0, 1, 2, 9]] == 1).all()
    assert _bits_equal(got[4:9], np.zeros(5, F32))                      # the closed gate writes +0


class _SteBinary(torch.autograd.Function):
    """utils/encodings.py:177-192 from its semantics: clamp, the two compares times +-1 and their sum; the backward passes
    the gradient where clamping left the value unchanged."""

    @staticmethod
    def forward(ctx, p):
        ctx.save_for_backward(p)
        q = torch.clamp(p, min=-1, max=1)
        return (q >= 0) * 1.0 + (q < 0) * -1.0

    @staticmethod
    def backward(ctx, g):
        p, = ctx.saved_tensors
        return g * ((torch.clamp(p, -1, 1) == p) + 0.0)


def test_restatement_agrees_with_the_reference_lines_in_torch():
    p = torch.from_numpy(np.concatenate([HAND_MADE, np.random.default_rng(0).uniform(-2, 2, 500).astype(F32)]))
    p.requires_grad_(True)
    s = _SteBinary.apply(p)
    assert s.dtype == torch.float32
    assert _bits_equal(s.detach().numpy(), MR.sign_table(p.detach().numpy()))
    s.backward(torch.ones_like(s))
    assert ((p.grad.numpy() == 1) == MR.gate(p.detach().numpy())).all() and set(np.unique(p.grad.numpy())) == {0.0, 1.0}
    # scene/gaussian_model.py:417 with its [1, 3] bounds
    x = torch.from_numpy(_points(500, seed=9))
    lo, hi = torch.tensor([BOUND_MIN]), torch.tensor([BOUND_MAX])
    u = (x - lo) / (hi - lo)
    assert _bits_equal(u.numpy(), MR.normalise(x.numpy(), BOUND_MIN, BOUND_MAX))
    assert _bits_equal(MR.normalise(x.numpy()), x.numpy())


def _torch_tables(F=2):
    return [(torch.from_numpy(p), torch.tensor(o, dtype=torch.int32), torch.tensor(r, dtype=torch.int32))
            for p, o, r in _tables(F, seed=1)]


def test_errors_come_in_the_siblings_order():
    t = _torch_tables()
    x = torch.zeros(5, 3)
    lo, hi = torch.tensor([BOUND_MIN]), torch.tensor([BOUND_MAX])
    bad_shape = torch.zeros(5, 2)
    # dtypes first, whatever else is wrong
    with pytest.raises(TypeError, match="x must be float32"):
        ME.mix_encode(bad_shape.double(), t, ME.MIX_DIMS)
    with pytest.raises(TypeError, match="params must be float32"):
        ME.mix_encode(bad_shape, [(t[0][0].half(),) + t[0][1:]] + t[1:], ME.MIX_DIMS)
    with pytest.raises(TypeError, match="offsets must be int32"):
        ME.mix_encode(bad_shape, [(t[0][0], t[0][1].long(), t[0][2])] + t[1:], ME.MIX_DIMS)
    with pytest.raises(TypeError, match="bound_max must be float32"):
        ME.mix_encode(bad_shape, t, ME.MIX_DIMS, lo, hi.double())
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        ME.mix_encode(x, t, ME.MIX_DIMS, lo, [2.0, 4.0, 9.0])
    # then what is not implemented
    with pytest.raises(NotImplementedError, match="bound_min requires a gradient"):
        ME.mix_encode(bad_shape, t, ME.MIX_DIMS, lo.clone().requires_grad_(True), hi)
    with torch.no_grad():   # (nothing asks for that gradient here: the shape is what is wrong)
        with pytest.raises(ValueError, match=r"x must be \[n, 3\]"):
            ME.mix_encode(bad_shape, t, ME.MIX_DIMS, lo.clone().requires_grad_(True), hi)
    for kw in ({"ste_multistep": True}, {"add_noise": True}):
        with pytest.raises(NotImplementedError):
            ME.MixEncoding(2, (18, 33), 10, (10, 40), 8, **kw)
    # then shapes
    for args, word in (((bad_shape, t, ME.MIX_DIMS), r"x must be \[n, 3\]"),
                       ((x, t, ME.MIX_DIMS, lo), "come together"),
                       ((x, t, ME.MIX_DIMS, lo, torch.zeros(4)), r"bound_max must be \[3\] or \[1, 3\]"),
                       ((x, [], ()), "1 to 4 tables"),
                       ((x, t + t[:1], ME.MIX_DIMS + ((0,),)), "1 to 4 tables"),
                       ((x, t, ME.MIX_DIMS[:3]), "one dims entry per table"),
                       ((x, t, ((0, 1, 2), (1, 0), (0, 2), (1, 2))), "distinct ascending"),
                       ((x, t, ((0, 1, 2), (0, 3), (0, 2), (1, 2))), "distinct ascending"),
                       ((x, t, ((0, 1, 2), (), (0, 2), (1, 2))), "distinct ascending"),
                       ((x, [(torch.zeros(8, 3),) + t[0][1:]] + t[1:], ME.MIX_DIMS), "F in"),
                       ((x, [(torch.zeros(8, 4),) + t[0][1:]] + t[1:], ME.MIX_DIMS), "same F"),
                       ((x, [(t[0][0], t[0][1][:-1], t[0][2])] + t[1:], ME.MIX_DIMS), r"offsets \[L \+ 1\]"),
                       ((x, [(t[0][0], torch.zeros(66, dtype=torch.int32), torch.zeros(65, dtype=torch.int32))], ((0, 1, 2),)),
                        "at most 64 levels"),
                       ((x, [t[0][:2]], ((0, 1, 2),)), "list of")):
        with pytest.raises(ValueError, match=word):
            ME.mix_encode(*args)
    # and the device last
    with pytest.raises(ValueError, match="x must be on the GPU"):
        ME.mix_encode(x, t, ME.MIX_DIMS, lo, hi)
    with pytest.raises(ValueError, match="must be on the GPU"):
        ME.mix_encode_maps(x, t[:1], ((0, 1, 2),), binary=False)


def test_entry_points_exist_with_the_registered_signatures():
    lib = _capi.lib()
    names = ("bsr_mix_grid_forward", "bsr_mix_grid_backward", "bsr_mix_grid_backward_scratch_bytes")
    for name in names:
        assert hasattr(lib, name) and name in _capi.SIGNATURES
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert len(_capi.SIGNATURES["bsr_mix_grid_forward"][1]) == 18 and len(_capi.SIGNATURES["bsr_mix_grid_backward"][1]) == 22
    hdr = open(_capi.os.path.join(_capi.os.path.dirname(_capi.CSRC), "..", "include", "bloomscene_mix_grid.h")).read()
    assert all(name in hdr for name in names) and "BSR_VERSION stays 4" in hdr and lib.bsr_version() == 4
    size = lib.bsr_mix_grid_backward_scratch_bytes
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    full = size(4, ints(1000, 200, 200, 200), 2, 24)
    assert full % 256 == 0 and full >= (1600 * 2) * 8 + 1600 * 2 // 8 + 24 * 4
    # a frozen table takes no room; with every table frozen only the per-level maxima are left
    assert size(4, ints(1000, 0, 200, 200), 2, 24) < full
    assert size(4, ints(0, 0, 0, 0), 2, 24) == 256
    # the refusals the C entry decides before anything is launched name their argument
    seen = []

    def calls():   # (the error string belongs to the calling thread)
        one = lambda t, v: (t * 1)(v)
        ptr, i = one(ctypes.c_void_p, None), lambda v: one(ctypes.c_int, v)
        dims = ints(0, 1, 2)
        fwd = lambda n, G, F, levels=4, D=3, d=dims: lib.bsr_mix_grid_forward(
            n, G, F, 1, None, 3, None, None, ptr, ptr, ptr, i(levels), i(8), i(D), d, None, None, None)
        for args, word in (((1, 0, 2), "n_grids"), ((1, 5, 2), "n_grids"), ((1, 1, 3), "n_features"), ((-1, 1, 2), "N >= 0"),
                           ((1, 1, 2, 65), "bad n_levels"), ((1, 1, 2, 4, 4), "1 to 3 coordinates"),
                           ((1, 1, 2, 4, 3, ints(0, 2, 1)), "ascending"), ((1, 1, 2, 4), "NULL buffer"),
                           ((2 ** 31 // 8 + 1, 1, 2, 0), None)):
            rc = fwd(*args)
            seen.append((args, rc, word is None or word in _capi.last_error()))
        seen.append(("n == 0", 1 - fwd(0, 1, 2, 0), True))             # n == 0: nothing is launched, success

    import threading
    th = threading.Thread(target=calls)
    th.start()
    th.join()
    assert len(seen) == 10
    for what, rc, named in seen[:-2]:
        assert rc == 1 and named, what
    assert seen[-2][1] == 0 and seen[-1][1] == 1                        # (no levels: a no-op, and so is n == 0)


def test_state_dict_has_the_reference_names_and_shapes():
    enc = ME.MixEncoding(2, RES_3D, 19, RES_2D, 17, ste_binary=True, ste_multistep=False, add_noise=False, Q=1)
    sd = enc.state_dict()
    names = ("encoding_xyz", "encoding_xy", "encoding_xz", "encoding_yz")
    assert list(sd) == [f"{n}.{k}" for n in names for k in ("params", "offsets_list", "resolutions_list")]

    def rows(D, res, log2):   # utils/encodings.py:381-387
        return [int(np.ceil(min(2 ** log2, r ** D) / 8) * 8) for r in res]

    for n in names:
        D, res, log2 = (3, RES_3D, 19) if n == "encoding_xyz" else (2, RES_2D, 17)
        total = sum(rows(D, res, log2))
        assert tuple(sd[f"{n}.params"].shape) == (total, 2) and sd[f"{n}.params"].dtype == torch.float32
        assert sd[f"{n}.offsets_list"].dtype == torch.int32 and sd[f"{n}.resolutions_list"].dtype == torch.int32
        assert sd[f"{n}.offsets_list"].tolist() == [0] + np.cumsum(rows(D, res, log2)).tolist()
        assert sd[f"{n}.resolutions_list"].tolist() == list(res)
    assert enc.output_dim == 2 * (12 + 3 * 4) == 48
    assert sum(p.numel() for p in enc.parameters()) > 10_000_000
    # a state dict with those keys loads key for key
    enc.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    assert [tuple(d) for d in ME.MIX_DIMS] == [(0, 1, 2), (0, 1), (0, 2), (1, 2)]
