"""The fused mixed 3D/2D binary hash-grid encoding on the GPU (include/bloomscene_mix_grid.h).  Two yardsticks:
(1) tests/mix_encoding_reference.py: out, dy_dx, every table gradient and grad_x bit-equal;
(2) the eager composition this call replaces, built on the same device from grid_encode on STE_binary-materialised tables,
    the normalisation line, the three cats and the output cat: out and dy_dx bit-equal, table gradients torch.equal,
    grad_x within the bound that the order of at most three additions allows.
Then the paths: partial waves and workgroups, one grid, no quantiser, no bounds, no x gradient, frozen tables, strided x and
upstream, a non-finite upstream, run-to-run and graph-replay identity, torch's memory pool, the shipped level lists."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mix_encoding_reference as MR

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = "cuda:0"
RES_3D_SMALL, LOG2_3D_SMALL = (18, 33, 80, 201), 10       # small hashmaps: dense and collision-heavy levels both occur
RES_2D_SMALL, LOG2_2D_SMALL = (10, 40, 130, 514), 8
RES_3D = (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514)   # scene/gaussian_model.py:134-135
RES_2D = (130, 258, 514, 1026)
BOUND_MIN, BOUND_MAX = (-3.0, -1.0, 0.5), (2.0, 4.0, 9.0)
BOUNDS = (BOUND_MIN, BOUND_MAX)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _tables(F, seed, G=4, res3=RES_3D_SMALL, log3=LOG2_3D_SMALL, res2=RES_2D_SMALL, log2=LOG2_2D_SMALL, spread=1.3):
    """numpy tables [(params, offsets, resolutions)] with |p| up to `spread`: values on both sides of STE_binary's gate."""
    from bloomscene_amd.grid_encoder import table_offsets
    rng = np.random.default_rng(seed)
    tables = []
    for D, res, lg in ((3, res3, log3), (2, res2, log2), (2, res2, log2), (2, res2, log2))[:G]:
        offs = np.array(table_offsets(D, res, lg), np.int64)
        tables.append((rng.uniform(-spread, spread, (int(offs[-1]), F)).astype(F32), offs, np.array(res, np.int64)))
    return tables


def _unit_points(n, seed):
    """The point generator of tests/test_grid_encoder_gpu.py (`_points`, D = 3), restated: corners, points outside in one
    coordinate, border cells of every level."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 1, (n, 3)).astype(F32)
    if n >= 64:
        u[0:4] = 0.0
        u[4:8] = 1.0
        u[8, 0] = -0.25
        u[9, -1] = 1.5
        u[10:20] = rng.uniform(0, 0.004, (10, 3)).astype(F32)
        u[20:30] = 1 - rng.uniform(0, 0.004, (10, 3)).astype(F32)
    return u


def _points(n, seed, bounds=BOUNDS):
    u = _unit_points(n, seed)
    if bounds is None:
        return u
    lo, hi = np.array(bounds[0], F32), np.array(bounds[1], F32)
    return (lo + u * (hi - lo)).astype(F32)


def _upstream(n, C, seed):
    return np.random.default_rng(seed).normal(0, 1, (n, C)).astype(F32)


def _device(tables, train=True):
    train = [train] * len(tables) if isinstance(train, bool) else train
    return [(torch.from_numpy(p).to(DEV).requires_grad_(t), torch.tensor(o, dtype=torch.int32, device=DEV),
             torch.tensor(r, dtype=torch.int32, device=DEV)) for (p, o, r), t in zip(tables, train)]


def _bounds(bounds):
    if bounds is None:
        return None, None
    return torch.tensor([bounds[0]], device=DEV), torch.tensor([bounds[1]], device=DEV)      # [1, 3] as the model keeps them


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _fused(x, tables, dims, g_out, bounds=BOUNDS, binary=True, x_grad=True, train=True, with_dy=True):
    """mix_encode forward + backward -> numpy out, dy_dx, [grad_params_g], grad_x."""
    from bloomscene_amd.mix_encoding import mix_encode, mix_encode_maps
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(DEV)
    xt = xt.detach().requires_grad_(x_grad) if not xt.requires_grad else xt
    tt = _device(tables, train)
    lo, hi = _bounds(bounds)
    out = mix_encode(xt, tt, dims, lo, hi, binary)
    gt = g_out if isinstance(g_out, torch.Tensor) else torch.from_numpy(g_out).to(DEV)
    leaves = [xt] * x_grad + [p for p, _, _ in tt if p.requires_grad]
    if leaves:
        got = list(torch.autograd.grad(out, leaves, gt))
    gx = got.pop(0) if x_grad else None
    grads = [got.pop(0) if p.requires_grad else None for p, _, _ in tt]
    dy = mix_encode_maps(xt.detach(), tt, dims, lo, hi, binary)[1] if with_dy else None
    torch.cuda.synchronize()
    return _np(out), _np(dy), [_np(g) for g in grads], _np(gx)


class _SteBinary(torch.autograd.Function):
    """utils/encodings.py:177-192 from its semantics, as the eager composition applies it to a whole table."""

    @staticmethod
    def forward(ctx, p):
        ctx.save_for_backward(p)
        q = torch.clamp(p, min=-1, max=1)
        return (q >= 0) * 1.0 + (q < 0) * -1.0

    @staticmethod
    def backward(ctx, g):
        p, = ctx.saved_tensors
        return g * ((torch.clamp(p, -1, 1) == p) + 0.0)


def _eager(x, tables, dims, g_out, bounds=BOUNDS, binary=True):
    """What the fused call replaces: scene/gaussian_model.py:417, :98-104 and utils/encodings.py:417-418 over the existing
    grid_encode -> numpy out, dy_dx (per row, the grids' blocks side by side), [grad_params_g], grad_x."""
    from bloomscene_amd.grid_encoder import forward_into, grid_encode
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    tt = _device(tables)
    lo, hi = _bounds(bounds)
    u = xt if bounds is None else (xt - lo) / (hi - lo)
    cols = torch.chunk(u, 3, dim=-1)
    outs, dys = [], []
    for (p, o, r), d in zip(tt, dims):
        inp = u if tuple(d) == (0, 1, 2) else torch.cat([cols[k] for k in d], dim=-1)
        emb = _SteBinary.apply(p) if binary else p
        outs.append(grid_encode(inp, emb, o, r))
        L, n, D, F = r.shape[0], x.shape[0], len(d), p.shape[1]
        buf, dy = torch.empty(L, n, F, device=DEV), torch.empty(n, L * D * F, device=DEV)
        forward_into(inp.detach().contiguous(), emb.detach().contiguous(), o, r, buf, dy, L)
        dys.append(dy)
    out = torch.cat(outs, dim=-1)
    got = torch.autograd.grad(out, [xt] + [p for p, _, _ in tt], torch.from_numpy(g_out).to(DEV))
    torch.cuda.synchronize()
    return _np(out), _np(torch.cat(dys, dim=-1)), [_np(g) for g in got[1:]], _np(got[0])


@functools.lru_cache(maxsize=None)
def _case(F, n, G=4, bounds=BOUNDS, binary=True, res3=RES_3D_SMALL):
    """One seeded scene and its restatement, computed once and shared (read-only)."""
    tables = _tables(F, seed=10 * F + G, G=G, res3=res3)
    dims = MR.MIX_DIMS[:G]
    x = _points(n, seed=F + n, bounds=bounds)
    lo, hi = bounds if bounds is not None else (None, None)
    out, dy = MR.forward(x, tables, dims, lo, hi, binary)
    g_out = _upstream(n, out.shape[1], seed=7)
    terms = []
    grads, gx = MR.backward(x, tables, dims, g_out, dy, lo, hi, binary, terms=terms)
    for a in [x, g_out, out, dy, gx] + grads + [t[0] for t in tables]:
        a.setflags(write=False)
    return dict(tables=tables, dims=dims, x=x, g_out=g_out, out=out, dy=dy, grads=grads, gx=gx, terms=terms, bounds=bounds)


def _check_restatement(c, got):
    out, dy, grads, gx = got
    assert _bits_equal(out, c["out"])
    if dy is not None:
        assert _bits_equal(dy, c["dy"])
    for g, ref in zip(grads, c["grads"]):
        if g is not None:
            assert _bits_equal(g, ref)
    if gx is not None:
        assert _bits_equal(gx, c["gx"])


def _check_eager(c, got, eager):
    """Yardstick 2.  grad_x: the two definitions add the same r_g[d] (at most three) in a different order, so each is within
    2 ulp-halves of the exact sum of its own order: |ours - eager| <= 2^-22 * sum_g |r_g[d]| / |max - min|, plus one ulp of
    the result for the division."""
    out, dy, grads, gx = got
    e_out, e_dy, e_grads, e_gx = eager
    assert _bits_equal(out, e_out) and _bits_equal(dy, e_dy)
    for g, e in zip(grads, e_grads):
        assert torch.equal(torch.from_numpy(g), torch.from_numpy(e))
    width = np.ones(3) if c["bounds"] is None else np.abs(np.array(c["bounds"][1], F32) - np.array(c["bounds"][0], F32)).astype(np.float64)
    total = sum(np.abs(t.astype(np.float64)) for t in c["terms"]) if c["terms"] else np.zeros_like(gx, np.float64)
    bound = 2.0 ** -22 * total / width[None, :] + np.spacing(np.abs(gx)).astype(np.float64)
    err = np.abs(gx.astype(np.float64) - e_gx.astype(np.float64))
    print(f"grad_x: max |ours - eager| = {err.max():.3e}, smallest slack = {(bound - err).min():.3e}, "
          f"bit-equal rows = {(gx.view(np.uint32) == e_gx.view(np.uint32)).all(axis=1).mean():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("F", [1, 2, 8])
def test_both_yardsticks_at_1000_points(F):
    c = _case(F, 1000)
    got = _fused(c["x"], c["tables"], c["dims"], c["g_out"])
    _check_restatement(c, got)
    _check_eager(c, got, _eager(c["x"], c["tables"], c["dims"], c["g_out"]))
    assert got[0].shape == (1000, 16 * F) and got[1].shape == (1000, (4 * 3 + 3 * 4 * 2) * F)
    gated = [np.abs(t[0]) > 1 for t in c["tables"]]
    assert all(m.any() and _bits_equal(g[m], np.zeros(int(m.sum()), F32)) for m, g in zip(gated, got[2]))   # +0 behind the gate
    assert all(np.abs(g).max() > 0 for g in got[2])


@pytest.mark.parametrize("n", [0, 1, 65, 257])
def test_partial_waves_and_workgroups(n):
    c = _case(2, n)
    got = _fused(c["x"], c["tables"], c["dims"], c["g_out"])
    _check_restatement(c, got)
    assert got[0].shape == (n, 32) and got[3].shape == (n, 3)
    if n == 0:
        assert all((g == 0).all() and g.shape == t[0].shape for g, t in zip(got[2], c["tables"]))
    else:
        _check_eager(c, got, _eager(c["x"], c["tables"], c["dims"], c["g_out"]))


def test_more_columns_than_one_tile_round():
    """F = 8 with five 3-D levels: C = 136 > 128 columns, the second round of the workgroup's LDS tile."""
    c = _case(8, 130, res3=(18, 33, 80, 201, 275))
    assert c["out"].shape[1] == 136
    _check_restatement(c, _fused(c["x"], c["tables"], c["dims"], c["g_out"]))


def test_one_grid_is_the_model_without_2d_planes():
    c = _case(2, 500, G=1)
    got = _fused(c["x"], c["tables"], c["dims"], c["g_out"])
    _check_restatement(c, got)
    _check_eager(c, got, _eager(c["x"], c["tables"], c["dims"], c["g_out"]))
    assert got[0].shape == (500, 8)


def test_without_the_quantiser_it_is_plain_grid_encode():
    c = _case(2, 500, binary=False)
    got = _fused(c["x"], c["tables"], c["dims"], c["g_out"], binary=False)
    _check_restatement(c, got)
    _check_eager(c, got, _eager(c["x"], c["tables"], c["dims"], c["g_out"], binary=False))
    m = np.abs(c["tables"][0][0]) > 1
    assert np.abs(got[2][0][m]).max() > 0            # no gate without the quantiser


def test_without_bounds():
    c = _case(2, 500, bounds=None)
    got = _fused(c["x"], c["tables"], c["dims"], c["g_out"], bounds=None)
    _check_restatement(c, got)
    _check_eager(c, got, _eager(c["x"], c["tables"], c["dims"], c["g_out"], bounds=None))


def test_module_is_the_one_line_integration():
    from bloomscene_amd.mix_encoding import MixEncoding
    c = _case(2, 500)
    enc = MixEncoding(2, RES_3D_SMALL, LOG2_3D_SMALL, RES_2D_SMALL, LOG2_2D_SMALL).to(DEV)
    with torch.no_grad():
        for name, (p, _, _) in zip(enc.NAMES, c["tables"]):
            getattr(enc, name).params.copy_(torch.from_numpy(p))
    lo, hi = _bounds(BOUNDS)
    x = torch.from_numpy(c["x"]).to(DEV)
    out = enc(x, lo, hi)
    assert _bits_equal(_np(out), c["out"]) and enc.output_dim == 32
    assert tuple(enc(x.view(5, 100, 3), lo, hi).shape) == (5, 100, 32)
    out.backward(torch.from_numpy(c["g_out"]).to(DEV))
    for name, ref in zip(enc.NAMES, c["grads"]):
        assert _bits_equal(_np(getattr(enc, name).params.grad), ref)
    with pytest.raises(RuntimeError):                 # double backward is refused
        xg = x.clone().requires_grad_(True)
        g, = torch.autograd.grad(enc(xg, lo, hi).sum(), xg, create_graph=True)
        g.sum().backward()


def test_no_x_gradient_allocates_no_dy_dx():
    from bloomscene_amd.mix_encoding import mix_encode
    c = _case(2, 1000)
    n, C, W = 1000, 32, 72
    x = torch.from_numpy(c["x"]).to(DEV)
    lo, hi = _bounds(BOUNDS)
    tt = _device(c["tables"])
    with torch.no_grad():                             # the rendering form: out and nothing else
        mix_encode(x, tt, c["dims"], lo, hi)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = mix_encode(x, tt, c["dims"], lo, hi)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    assert peak <= n * C * 4 + 512 and peak < n * C * 4 + n * W * 4, peak
    assert _bits_equal(_np(out), c["out"])
    # training with a detached x: the forward still allocates out alone, the backward gives the tables their gradients
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = mix_encode(x, tt, c["dims"], lo, hi)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before <= n * C * 4 + 512
    grads = torch.autograd.grad(out, [p for p, _, _ in tt], torch.from_numpy(c["g_out"]).to(DEV))
    assert all(_bits_equal(_np(g), ref) for g, ref in zip(grads, c["grads"]))


def test_frozen_tables_pay_no_scratch():
    from bloomscene_amd import _capi
    from bloomscene_amd.mix_encoding import mix_encode
    c = _case(2, 1000)
    got = _fused(c["x"], c["tables"], c["dims"], c["g_out"], train=False, with_dy=False)
    _check_restatement(c, got)
    assert all(g is None for g in got[2])
    x = torch.from_numpy(c["x"]).to(DEV).requires_grad_(True)
    lo, hi = _bounds(BOUNDS)
    out = mix_encode(x, _device(c["tables"], False), c["dims"], lo, hi)
    g = torch.from_numpy(c["g_out"]).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    gx, = torch.autograd.grad(out, x, g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    rows = (ctypes.c_int * 4)(*[t[0].shape[0] for t in c["tables"]])
    assert peak <= 1000 * 3 * 4 + 512 < _capi.lib().bsr_mix_grid_backward_scratch_bytes(4, rows, 2, 16), peak
    assert _bits_equal(_np(gx), c["gx"])


def test_one_frozen_table_among_trainable_ones():
    c = _case(2, 1000)
    for frozen in (0, 2):
        train = [g != frozen for g in range(4)]
        got = _fused(c["x"], c["tables"], c["dims"], c["g_out"], train=train, with_dy=False)
        _check_restatement(c, got)
        assert [g is None for g in got[2]] == [not t for t in train]


def test_strided_x_and_strided_upstream_are_read_in_place():
    c = _case(2, 1000)
    wide = torch.zeros(1000, 7, device=DEV)
    wide[:, 2:5] = torch.from_numpy(c["x"]).to(DEV)
    x = wide[:, 2:5]
    assert not x.is_contiguous()
    wide_g = torch.full((1000, 40), 3.0, device=DEV)
    wide_g[:, 5:37] = torch.from_numpy(c["g_out"]).to(DEV)
    _check_restatement(c, _fused(x, c["tables"], c["dims"], wide_g[:, 5:37], with_dy=False))
    # and through a consumer that splits a wider tensor: autograd hands the node a column slice of the wide gradient
    from bloomscene_amd.mix_encoding import mix_encode
    xt = x.detach().requires_grad_(True)
    tt = _device(c["tables"])
    out = mix_encode(xt, tt, c["dims"], *_bounds(BOUNDS))
    other = torch.zeros(1000, 5, device=DEV, requires_grad=True)
    joined = torch.cat([other, out, other[:, :3]], dim=1)
    head, mid, tail = torch.split(joined, [5, 32, 3], dim=1)
    (head.sum() + (mid * torch.from_numpy(c["g_out"]).to(DEV)).sum() + tail.sum()).backward()
    assert _bits_equal(_np(xt.grad), c["gx"]) and all(_bits_equal(_np(p.grad), ref) for (p, _, _), ref in zip(tt, c["grads"]))


def test_non_finite_upstream_stays_in_the_elements_it_reaches():
    c = _case(2, 1000)
    g_out = c["g_out"].copy()
    g_out[100, 3] = np.inf          # xyz, level 1
    g_out[200, 20] = np.nan         # xz, level 2
    g_out[300, 31] = -np.inf        # yz, level 3
    lo, hi = BOUNDS
    grads_ref, gx_ref = MR.backward(c["x"], c["tables"], c["dims"], g_out, c["dy"], lo, hi)
    _, _, grads, gx = _fused(c["x"], c["tables"], c["dims"], g_out, with_dy=False)
    hit = 0
    for g, ref, clean, (p, _, _) in zip(grads, grads_ref, c["grads"], c["tables"]):
        bad = np.isnan(ref)
        assert (np.isnan(g) == bad).all() and _bits_equal(g[~bad], ref[~bad])
        assert _bits_equal(g[~bad], clean[~bad])                      # every other element is what it was
        assert not bad[np.abs(p) > 1].any() and _bits_equal(g[np.abs(p) > 1], np.zeros(int((np.abs(p) > 1).sum()), F32))
        hit += int(bad.sum())
    assert hit >= 3
    bad = ~np.isfinite(gx_ref)
    assert set(np.nonzero(bad.any(axis=1))[0]) == {100, 200, 300}
    assert (~np.isfinite(gx) == bad).all() and _bits_equal(gx[~bad], gx_ref[~bad])


def test_two_runs_and_a_graph_replay_give_identical_bits():
    from bloomscene_amd.mix_encoding import mix_encode
    c = _case(2, 1000)
    first = _fused(c["x"], c["tables"], c["dims"], c["g_out"], with_dy=False)
    second = _fused(c["x"], c["tables"], c["dims"], c["g_out"], with_dy=False)
    assert _bits_equal(first[0], second[0]) and _bits_equal(first[3], second[3])
    assert all(_bits_equal(a, b) for a, b in zip(first[2], second[2]))
    xt = torch.from_numpy(c["x"]).to(DEV).requires_grad_(True)
    tt = _device(c["tables"])
    lo, hi = _bounds(BOUNDS)
    gt = torch.from_numpy(c["g_out"]).to(DEV)
    leaves = [xt] + [p for p, _, _ in tt]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):   # warm-up outside the capture
            torch.autograd.grad(mix_encode(xt, tt, c["dims"], lo, hi), leaves, gt)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                     # (nothing waits on the host: the capture would fail)
        out = mix_encode(xt, tt, c["dims"], lo, hi)
        got = torch.autograd.grad(out, leaves, gt)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert _bits_equal(_np(out), first[0]) and _bits_equal(_np(got[0]), first[3])
        assert all(_bits_equal(_np(g), ref) for g, ref in zip(got[1:], first[2]))


def test_no_device_memory_outside_torchs_pool():
    from bloomscene_amd import _capi
    from bloomscene_amd.mix_encoding import mix_encode
    tables = _tables(2, seed=3)
    tt = _device(tables)
    lo, hi = _bounds(BOUNDS)
    n = 50_000
    xt = torch.from_numpy(_points(n, seed=1)).to(DEV).requires_grad_(True)
    mix_encode(xt[:1000], tt, MR.MIX_DIMS, lo, hi).sum().backward()    # library loaded, kernels resident
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, total = torch.cuda.mem_get_info()
    outside0 = total - free0 - torch.cuda.memory_reserved()
    alloc0 = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    mix_encode(xt, tt, MR.MIX_DIMS, lo, hi).sum().backward()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    outside1 = total - free1 - torch.cuda.memory_reserved()
    assert outside1 - outside0 < (8 << 20), (outside0, outside1)
    rows = (ctypes.c_int * 4)(*[t[0].shape[0] for t in tables])
    # the backward's scratch and the saved dy_dx are on torch's books
    assert torch.cuda.max_memory_allocated() - alloc0 >= _capi.lib().bsr_mix_grid_backward_scratch_bytes(4, rows, 2, 16) + n * 72 * 4


def test_shipped_level_lists_against_the_eager_composition():
    """12 3-D levels at 2^19 and 3 x 4 2-D levels at 2^17, F = 2: the 24-slot descriptor and the 10 M-element finalize."""
    n = 2048
    tables = _tables(2, seed=4, res3=RES_3D, log3=19, res2=RES_2D, log2=17)
    assert sum(t[0].size for t in tables) > 10_000_000
    x = _points(n, seed=2)
    g_out = _upstream(n, 48, seed=3)
    got = _fused(x, tables, MR.MIX_DIMS, g_out)
    eager = _eager(x, tables, MR.MIX_DIMS, g_out)
    # (the bound's terms r_g[d] from the eager side's own dy_dx, grid by grid)
    terms, c0, w0 = [], 0, 0
    for (p, o, r), d in zip(tables, MR.MIX_DIMS):
        L, D = len(r), len(d)
        g = g_out[:, c0:c0 + L * 2].reshape(n, L, 1, 2).astype(np.float64)
        dy = eager[1][:, w0:w0 + L * D * 2].reshape(n, L, D, 2).astype(np.float64)
        t = np.zeros((n, 3))
        t[:, list(d)] = (g * dy).sum(axis=(1, 3))                      # r_g[d] (its fp32 value is within 2^-20 of this one)
        terms.append(t)
        c0, w0 = c0 + L * 2, w0 + L * D * 2
    _check_eager(dict(bounds=BOUNDS, terms=terms), got, eager)
    assert got[0].shape == (n, 48) and got[1].shape == (n, (12 * 3 + 3 * 4 * 2) * 2)
