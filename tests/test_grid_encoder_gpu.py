"""Hash-grid encoder on the GPU (include/bloomscene_grid.h): forward / dy_dx bit-equal to tests/grid_reference.py, the
fixed-point grad_embeddings bit-equal to the restated rule and stable across runs, streams and a graph replay,
grad_inputs bit-equal, non-finite gradients confined to their rows, the _gridencoder shim on BloomScene's call pattern,
and no device memory outside torch's pool."""
import numpy as np
import pytest
import torch

import grid_reference as GR

pytestmark = pytest.mark.gpu

F32 = np.float32
RES_3D = (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514)
RES_2D = (130, 258, 514, 1026)
DEV = "cuda:0"


def _table(D, F, res, log2, seed=0):
    from bloomscene_amd.grid_encoder import table_offsets
    offs = np.array(table_offsets(D, res, log2), np.int64)
    emb = np.random.default_rng(seed).uniform(-1, 1, (int(offs[-1]), F)).astype(F32)
    return offs, np.array(res, np.int64), emb


def _points(N, D, seed, edges=True):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (N, D)).astype(F32)
    if edges and N >= 64:
        x[0:4] = 0.0
        x[4:8] = 1.0
        x[8, 0] = -0.25
        x[9, -1] = 1.5
        x[10:20] = rng.uniform(0, 0.004, (10, D)).astype(F32)          # border cells of every level
        x[20:30] = 1 - rng.uniform(0, 0.004, (10, D)).astype(F32)
    return x


def _run(x, emb, offs, res, grad, min_level=0, n_levels=None):
    """grid_encode forward + backward on the GPU -> numpy outputs [L, N, F], dy_dx [N, L, D, F], grad_embeddings,
    grad_inputs."""
    from bloomscene_amd.grid_encoder import grid_encode
    N, D = x.shape
    F = emb.shape[1]
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    et = torch.from_numpy(emb).to(DEV).requires_grad_(True)
    ot = torch.tensor(offs, dtype=torch.int32, device=DEV)
    rt = torch.tensor(res, dtype=torch.int32, device=DEV)
    out = grid_encode(xt, et, ot, rt, min_level, n_levels)
    L = out.shape[1] // F
    out.backward(torch.from_numpy(np.ascontiguousarray(grad.transpose(1, 0, 2))).reshape(N, L * F).to(DEV))
    o = out.detach().view(N, L, F).permute(1, 0, 2).cpu().numpy()
    return o, et.grad.cpu().numpy(), xt.grad.cpu().numpy()


def _dy_dx(x, emb, offs, res, n_levels):
    from bloomscene_amd.grid_encoder import forward_into
    N, D = x.shape
    F = emb.shape[1]
    out = torch.empty(n_levels, N, F, device=DEV)
    dy = torch.empty(N, n_levels * D * F, device=DEV)
    forward_into(torch.from_numpy(x).to(DEV), torch.from_numpy(emb).to(DEV),
                 torch.tensor(offs, dtype=torch.int32, device=DEV), torch.tensor(res, dtype=torch.int32, device=DEV),
                 out, dy, n_levels)
    return out.cpu().numpy(), dy.view(N, n_levels, D, F).cpu().numpy()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("D,F", [(1, 1), (1, 2), (1, 8), (2, 1), (2, 2), (2, 8), (3, 1), (3, 2), (3, 8)])
def test_forward_backward_bit_equal_to_restatement(D, F):
    res = {1: (7, 50, 300, 3000), 2: (10, 40, 130, 514), 3: (18, 33, 80, 201)}[D]
    offs, r, emb = _table(D, F, res, 10 if D > 1 else 8, seed=D * 10 + F)   # small hashmaps: collision-heavy levels
    N = 20_000
    x = _points(N, D, seed=F)
    g = np.random.default_rng(7).normal(0, 1, (len(res), N, F)).astype(F32)
    out_ref, dy_ref = GR.forward(x, emb, offs, r)
    ge_ref, gi_ref, _ = GR.backward(x, offs, r, emb.shape[0], g, dy_ref)
    o, ge, gi = _run(x, emb, offs, r, g)
    _, dy = _dy_dx(x, emb, offs, r, len(res))
    assert _bits_equal(o, out_ref)
    assert _bits_equal(dy, dy_ref)
    assert _bits_equal(ge, ge_ref)
    assert _bits_equal(gi, gi_ref)
    s64, bound, cnt = GR.fixed_point_bound(x, offs, r, emb.shape[0], g)
    assert (np.abs(ge.astype(np.float64) - s64) <= bound).all()


@pytest.mark.parametrize("cfg", ["3d", "2d"])
def test_bloomscene_configurations_at_100k(cfg):
    D, res, log2 = (3, RES_3D, 19) if cfg == "3d" else (2, RES_2D, 17)
    offs, r, emb = _table(D, 2, res, log2, seed=5)
    N = 100_000
    x = _points(N, D, seed=11)
    g = np.random.default_rng(8).normal(0, 1e-3, (len(res), N, 2)).astype(F32)
    out_ref, dy_ref = GR.forward(x, emb, offs, r)
    o, ge, gi = _run(x, emb, offs, r, g)
    _, dy = _dy_dx(x, emb, offs, r, len(res))
    assert _bits_equal(o, out_ref) and _bits_equal(dy, dy_ref)
    ge_ref, gi_ref, _ = GR.backward(x, offs, r, emb.shape[0], g, dy_ref)
    assert _bits_equal(ge, ge_ref) and _bits_equal(gi, gi_ref)


def test_int_min_level_slices():
    offs, r, emb = _table(3, 2, RES_3D, 19, seed=2)
    N = 5000
    x = _points(N, 3, seed=3)
    for lo, n in ((0, 4), (6, 3), (10, 2), (3, 9)):
        g = np.random.default_rng(lo).normal(0, 1, (n, N, 2)).astype(F32)
        out_ref, dy_ref = GR.forward(x, emb, offs[lo:lo + n + 1], r[lo:lo + n])
        ge_ref, gi_ref, _ = GR.backward(x, offs[lo:lo + n + 1], r[lo:lo + n], emb.shape[0], g, dy_ref)
        o, ge, gi = _run(x, emb, offs, r, g, min_level=lo, n_levels=n)
        assert _bits_equal(o, out_ref) and _bits_equal(ge, ge_ref) and _bits_equal(gi, gi_ref)
        # rows of the levels not computed are 0
        assert (ge[:offs[lo]] == 0).all() and (ge[offs[lo + n]:] == 0).all()


def _raw_backward(x, offs, r, rows, g, stream=None):
    from bloomscene_amd.grid_encoder import backward_into
    L, N, F = g.shape
    ge = torch.full((rows, F), 7.0, device=DEV)   # fully overwritten
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        backward_into(torch.from_numpy(g).to(DEV), torch.from_numpy(x).to(DEV),
                      torch.tensor(offs, dtype=torch.int32, device=DEV), torch.tensor(r, dtype=torch.int32, device=DEV),
                      ge, None, None, L)
    torch.cuda.synchronize()
    return ge.cpu().numpy()


def test_grad_embeddings_identical_across_runs_streams_and_graph_replay():
    offs, r, emb = _table(3, 2, RES_3D, 19, seed=4)
    N = 200_000
    x = _points(N, 3, seed=5)
    g = np.random.default_rng(9).normal(0, 1, (len(RES_3D), N, 2)).astype(F32)
    ref = _raw_backward(x, offs, r, emb.shape[0], g)
    for _ in range(2):
        assert _bits_equal(_raw_backward(x, offs, r, emb.shape[0], g), ref)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    assert _bits_equal(_raw_backward(x, offs, r, emb.shape[0], g, s1), ref)
    assert _bits_equal(_raw_backward(x, offs, r, emb.shape[0], g, s2), ref)
    # forward + backward of grid_encode captured in one graph on one stream, replayed
    from bloomscene_amd.grid_encoder import grid_encode
    xt = torch.from_numpy(x).to(DEV)
    et = torch.from_numpy(emb).to(DEV).requires_grad_(True)
    ot = torch.tensor(offs, dtype=torch.int32, device=DEV)
    rt = torch.tensor(r, dtype=torch.int32, device=DEV)
    gt = torch.from_numpy(np.ascontiguousarray(g.transpose(1, 0, 2))).reshape(N, -1).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):   # warm-up outside the capture
            et.grad = None
            grid_encode(xt, et, ot, rt).backward(gt)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    et.grad = None
    with torch.cuda.graph(graph):
        out = grid_encode(xt, et, ot, rt)
        out.backward(gt)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert _bits_equal(et.grad.cpu().numpy(), ref)
    out_ref, _ = GR.forward(x, emb, offs, r, with_dy_dx=False)
    assert _bits_equal(out.detach().view(N, -1, 2).permute(1, 0, 2).cpu().numpy(), out_ref)


def test_contended_rows_stay_bit_stable():
    """All points in one small region: thousands of contributions per row of the coarse levels."""
    offs, r, emb = _table(3, 2, RES_3D, 19, seed=6)
    N = 100_000
    x = (0.5 + np.random.default_rng(1).uniform(-0.01, 0.01, (N, 3))).astype(F32)
    g = np.random.default_rng(2).normal(0, 1, (len(RES_3D), N, 2)).astype(F32)
    ge_ref, _, _ = GR.backward(x, offs, r, emb.shape[0], g)
    _, _, cnt = GR.fixed_point_bound(x, offs, r, emb.shape[0], g)
    assert cnt.max() >= 2000
    for _ in range(3):
        assert _bits_equal(_raw_backward(x, offs, r, emb.shape[0], g), ge_ref)


def test_inf_gradient_gives_nan_in_exactly_its_rows():
    offs, r, emb = _table(2, 2, (10, 40), 10, seed=1)
    N = 2000
    x = _points(N, 2, seed=4, edges=False)
    g = np.random.default_rng(3).normal(0, 1, (2, N, 2)).astype(F32)
    g[1, 17, 0] = np.inf
    ge = _raw_backward(x, offs, r, emb.shape[0], g)
    ref, _, _ = GR.backward(x, offs, r, emb.shape[0], g)
    touched = np.zeros(emb.shape[0] * 2, bool)
    for e, v in GR.contributions(x, offs, r, emb.shape[0], g):
        touched[e[~np.isfinite(v)]] = True
    touched = touched.reshape(-1, 2)
    assert touched.sum() >= 1
    assert np.isnan(ge[touched]).all() and np.isfinite(ge[~touched]).all()
    assert _bits_equal(ge[~touched], ref[~touched])


def test_zero_points_is_a_no_op():
    from bloomscene_amd.grid_encoder import grid_encode
    offs, r, emb = _table(3, 2, RES_3D[:3], 19)
    xt = torch.empty(0, 3, device=DEV, requires_grad=True)
    et = torch.from_numpy(emb).to(DEV).requires_grad_(True)
    out = grid_encode(xt, et, torch.tensor(offs, dtype=torch.int32, device=DEV),
                      torch.tensor(r, dtype=torch.int32, device=DEV))
    assert tuple(out.shape) == (0, 6)
    out.sum().backward()
    torch.cuda.synchronize()
    assert (et.grad == 0).all() and tuple(xt.grad.shape) == (0, 3)


def test_shim_on_bloomscene_call_pattern_matches_grid_encode():
    """BloomScene's _grid_encode (utils/encodings.py:230-349) as a caller: int min_level_id -> sliced offsets /
    resolutions, outputs [L, N, F], dy_dx [N, L * D * F], zeroed grad_embeddings, positional arguments."""
    import _gridencoder as backend
    from bloomscene_amd.grid_encoder import grid_encode
    offs, r, emb = _table(2, 2, RES_2D, 17, seed=3)
    N, D, F = 30_000, 2, 2
    x = _points(N, D, seed=6)
    xt = torch.from_numpy(x).to(DEV)
    et = torch.from_numpy(emb).to(DEV)
    ot = torch.tensor(offs, dtype=torch.int32, device=DEV)
    rt = torch.tensor(r, dtype=torch.int32, device=DEV)
    lo, n = 1, 3
    outputs = torch.empty(n, N, F, device=DEV)
    dy_dx = torch.empty(N, n * D * F, device=DEV)
    backend.grid_encode_forward(xt, et, ot[lo:lo + n + 1], rt[lo:lo + n], outputs, N, D, F, n, 0, 128, 0, dy_dx, None,
                                None)
    grad = torch.randn(N, n * F, device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    g = grad.view(N, n, F).permute(1, 0, 2).contiguous()
    grad_embeddings = torch.zeros_like(et)
    grad_inputs = torch.zeros_like(xt)
    backend.grid_encode_backward(g, xt, et, ot[lo:lo + n + 1], rt[lo:lo + n], grad_embeddings, N, D, F, n, 0, 128,
                                 dy_dx, grad_inputs, None, None)
    xr = xt.clone().requires_grad_(True)
    er = et.clone().requires_grad_(True)
    ref = grid_encode(xr, er, ot, rt, lo, n)
    ref.backward(grad)
    torch.cuda.synchronize()
    assert torch.equal(outputs.permute(1, 0, 2).reshape(N, n * F), ref.detach())
    assert torch.equal(grad_embeddings, er.grad) and torch.equal(grad_inputs, xr.grad)


def test_no_device_memory_outside_torch_at_1m():
    from bloomscene_amd.grid_encoder import grid_encode
    offs, r, emb = _table(3, 2, RES_3D, 19)
    N = 1_000_000
    xt = torch.rand(N, 3, device=DEV)
    et = torch.from_numpy(emb).to(DEV).requires_grad_(True)
    ot = torch.tensor(offs, dtype=torch.int32, device=DEV)
    rt = torch.tensor(r, dtype=torch.int32, device=DEV)
    grid_encode(xt[:1000], et, ot, rt).sum().backward()    # library loaded, kernels resident
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, total = torch.cuda.mem_get_info()
    outside0 = total - free0 - torch.cuda.memory_reserved()
    alloc0 = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    grid_encode(xt, et, ot, rt).sum().backward()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    outside1 = total - free1 - torch.cuda.memory_reserved()
    assert outside1 - outside0 < (8 << 20), (outside0, outside1)
    from bloomscene_amd import _capi
    # the backward's scratch is on torch's books
    assert torch.cuda.max_memory_allocated() - alloc0 >= _capi.lib().bsr_grid_backward_scratch_bytes(emb.shape[0], 2, 12)
    assert torch.isfinite(et.grad).all()
