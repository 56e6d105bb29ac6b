"""Anchor adjustment on the GPU (include/bloomscene_adjust.h) against the restatements of tests/adjust_reference.py.
Everything is bit-equal: values are moved, not computed, so there is no tolerance anywhere."""
import numpy as np
import pytest
import torch

import adam_reference as AREF
import adjust_reference as AR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x5A5A5A5A
F32 = np.float32


def _A():
    import bloomscene_amd.adjust as A
    return A


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.int32).cpu().numpy().view(np.uint32)


# ---- decide ----

def _random_stats(N, K, seed, prune="some"):
    """Seeded statistics with the boundary inputs of the CPU test embedded at random positions."""
    rng = np.random.default_rng(seed)
    d = rng.choice(np.array([0, 13, 79, 80, 81, 100, 250], F32), N).astype(F32)
    s = (d * rng.uniform(0.0, 0.012, N)).astype(F32)
    den = rng.choice(np.array([0, 7, 39, 40, 41, 60, 100], F32), N * K).astype(F32)
    acc = (den * rng.uniform(0.0, 0.002, N * K)).astype(F32)
    if prune == "all":
        d[:], s[:] = 100, 0.1
    if prune == "none":
        s[:] = d
    return s, d, acc, den


def _embed(stats, boundary, K, seed):
    s, d, acc, den = stats
    bs, bd, bacc, bden = boundary
    rng = np.random.default_rng(seed)
    rows = rng.permutation(s.shape[0])[:bs.shape[0]]
    s[rows], d[rows] = bs[:rows.shape[0]], bd[:rows.shape[0]]
    at = rng.permutation(acc.shape[0])[:bacc.shape[0]]
    acc[at], den[at] = bacc[:at.shape[0]], bden[:at.shape[0]]
    return s, d, acc, den


def _decide_raw(stats, K, thresholds, scratch_fill):
    """One direct bsr_adjust_decide call with a scratch of the asked size, pre-filled."""
    import ctypes
    from bloomscene_amd import _capi
    lib = _capi.lib()
    s, d, acc, den = (torch.from_numpy(a).to(DEV) for a in stats)
    N = s.shape[0]
    nbytes = lib.bsr_adjust_decide_scratch_bytes(N)
    scratch = torch.full((nbytes + 256,), scratch_fill, dtype=torch.uint8, device=DEV)
    offset_flags = torch.full((N * K + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    anchor_flags = torch.full((N + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    src_of = torch.full((N + 16,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    thr = (ctypes.c_double * len(thresholds))(*thresholds)
    _capi.check(lib.bsr_adjust_decide(N, K, s.data_ptr(), d.data_ptr(), acc.data_ptr(), den.data_ptr(), len(thresholds), thr,
                                      100 * 0.8 * 0.5, 100 * 0.8, 0.005, offset_flags.data_ptr(), anchor_flags.data_ptr(),
                                      src_of.data_ptr(), status.data_ptr(), scratch.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), "bsr_adjust_decide")
    torch.cuda.synchronize()
    assert (scratch[nbytes:] == scratch_fill).all() and (offset_flags[N * K:] == 0x5A).all() and (anchor_flags[N:] == 0x5A).all()
    assert (status[4:] == -7).all()
    return offset_flags[:N * K].cpu().numpy(), anchor_flags[:N].cpu().numpy(), src_of.cpu().numpy(), status[:4].tolist()


@pytest.mark.parametrize("K,L", [(1, 1), (10, 3), (16, 7)])
@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 3 * 1024 + 7])
def test_decide_equals_the_restatement(N, K, L):
    thresholds = [0.0002 * (2 ** i) for i in range(L)]
    stats = _random_stats(N, K, seed=N + K)
    if N > 1:
        stats = _embed(stats, AR.boundary_stats(K, thresholds), K, seed=N)
    want = AR.decide_ref(*stats, K, thresholds)
    runs = [_decide_raw(stats, K, thresholds, fill) for fill in (0x00, 0xFF, 0xFF)]
    for flags, aflags, src_of, status in runs:
        n_keep = want[3][0]
        assert status == want[3]
        assert np.array_equal(flags, want[0]) and np.array_equal(aflags, want[1])
        assert np.array_equal(src_of[:n_keep], want[2]) and (src_of[n_keep:] == -7).all()
    # the Python layer: the same, and no host read is needed to get there
    dev = [torch.from_numpy(a).to(DEV) for a in stats]
    flags, aflags, src_of, status = _A().decide(dev[0].view(-1, 1), dev[1].view(-1, 1), dev[2].view(-1, 1), dev[3].view(-1, 1),
                                                K, thresholds)
    assert status.is_cuda and status.tolist() == want[3]
    assert np.array_equal(flags.cpu().numpy(), want[0]) and np.array_equal(src_of[:want[3][0]].cpu().numpy(), want[2])


@pytest.mark.parametrize("prune", ["all", "none"])
def test_decide_all_pruned_and_none_pruned(prune):
    N, K, thresholds = 2 * 1024 + 5, 10, [0.0002, 0.0004, 0.0008]
    stats = _random_stats(N, K, seed=4, prune=prune)
    want = AR.decide_ref(*stats, K, thresholds)
    assert want[3][0] == (0 if prune == "all" else N)
    flags, aflags, src_of, status = _decide_raw(stats, K, thresholds, 0xFF)
    assert status == want[3] and np.array_equal(aflags, want[1]) and np.array_equal(flags, want[0])
    assert np.array_equal(src_of[:want[3][0]], want[2]) and (src_of[want[3][0]:] == -7).all()


def test_decide_on_an_empty_model_and_what_the_device_norm_gives_for_tiny_values():
    z = torch.zeros(0, 1, device=DEV)
    flags, aflags, src_of, status = _A().decide(z, z, z, z, 10, [0.0002])
    assert status.tolist() == [0, 0, 0, 0] and flags.numel() == aflags.numel() == src_of.numel() == 0
    # torch.norm over one element on this device: recorded in the header's deviation note; it decides nothing
    tiny = torch.tensor([[3.3e-23], [1e-30], [2e-19]], device=DEV)
    got = torch.norm(tiny, dim=-1).cpu().numpy()
    print("device torch.norm of", tiny.view(-1).tolist(), "->", got.tolist())
    assert (got < 1e-10).all()


# ---- resize_rows ----

WIDTHS = (1, 3, 4, 6, 10, 30, 32, 50, 64)


def _keep_rows(N, pattern, rng):
    rows = np.arange(N)
    if pattern == "all":
        return rows
    if pattern == "none":
        return rows[:0]
    if pattern == "every other":
        return rows[::2]
    if pattern == "one long run":
        return rows[N // 5: N // 5 + max(1, N // 2)]
    return rows[rng.random(N) < 0.7]


class _Carved:
    """Outputs of one resize call in ONE block of memory, a guard word behind each (and 256-byte aligned starts)."""

    def __init__(self, sizes):
        self.span, off = [], 64
        for n in sizes:
            self.span.append((off, off + n))
            off = (off + n + 1 + 63) // 64 * 64
        self.block = torch.full((off,), GUARD, dtype=torch.int32, device=DEV)

    def out(self, k, dtype):
        a, b = self.span[k]
        return self.block[a:b].view(dtype)

    def guards_intact(self):
        keep = torch.ones(self.block.shape[0], dtype=torch.bool, device=DEV)
        for a, b in self.span:
            keep[a:b] = False
        return bool((self.block[keep] == GUARD).all())


def _resize_case(N, rng):
    """Tensors of every width at storage offsets 0 and 1, an int32 one among them, and an op for some."""
    tensors, ops, host = [], [], []
    for w in WIDTHS:
        for shift in (0, 1):
            x = (rng.standard_normal((N, w)) * 0.1).astype(F32)
            op = None
            if w in (6, 64):
                x[rng.random((N, w)) < 0.1] = F32(0.05)
                x[rng.random((N, w)) < 0.05] = np.nan
                op = ("clamp_from", 3, 0.05)
            if w in (1, 3):
                op = ("zero_flagged", rng.integers(0, 4, N).astype(np.uint8), 2, False)
            if w in (10, 32):
                op = ("zero_flagged", (rng.integers(0, 2, N * w) * 0x80 + rng.integers(0, 8, N * w)).astype(np.uint8), 0x80, True)
            base = torch.empty(N * w + 1, dtype=torch.float32, device=DEV)
            t = base[shift:shift + N * w].view(N, w)
            t.copy_(torch.from_numpy(x))
            assert t.data_ptr() % 16 == 4 * shift
            tensors.append(t)
            host.append(x)
            ops.append(op)
    xi = rng.integers(-2 ** 31, 2 ** 31, (N, 5), dtype=np.int64).astype(np.int32)
    tensors.append(torch.from_numpy(xi).to(DEV))
    host.append(xi)
    ops.append(None)
    return tensors, host, ops


def _fill_bits(f, dtype):
    return int(np.array([f], dtype).view(np.uint32)[0])


@pytest.mark.parametrize("pattern", ["all", "none", "every other", "one long run", "random"])
@pytest.mark.parametrize("N", [1, 1025, 2500])
def test_resize_rows_equals_the_restatement(N, pattern):
    rng = np.random.default_rng(N + len(pattern))
    tensors, host, ops = _resize_case(N, rng)
    dev_ops = [op if op is None or op[0] != "zero_flagged" else (op[0], torch.from_numpy(op[1]).to(DEV), op[2], op[3])
               for op in ops]
    rows = _keep_rows(N, pattern, rng)
    n_keep = rows.shape[0]
    src_of = torch.from_numpy(rows.astype(np.int32)).to(DEV)
    for A in (0, 1, 333):
        for with_append in (False, True):
            if A == 0 and with_append:
                continue
            appends = [((rng.standard_normal((A,) + h.shape[1:]) * 0.2).astype(h.dtype) if h.dtype == F32 else
                        rng.integers(-99, 99, (A,) + h.shape[1:]).astype(np.int32)) if with_append and k % 3 != 2 else None
                       for k, h in enumerate(host)]
            fills = [(-3 if h.dtype == np.int32 else 0.25 * k) for k, h in enumerate(host)]
            carved = _Carved([(n_keep + A) * int(np.prod(h.shape[1:])) for h in host])
            outs = [carved.out(k, torch.float32 if h.dtype == F32 else torch.int32) for k, h in enumerate(host)]
            got = _A().resize_rows(tensors, src_of, n_keep, [None if a is None else torch.from_numpy(a).to(DEV) for a in appends],
                                   fills, dev_ops, n_append=A, out=outs)
            torch.cuda.synchronize()
            assert carved.guards_intact()
            for k, (h, a, f, op) in enumerate(zip(host, appends, fills, ops)):
                want = AR.resize_ref(h, rows, n_keep, A, a, _fill_bits(f, h.dtype), op)
                assert got[k].data_ptr() == outs[k].data_ptr()
                assert np.array_equal(_bits(got[k]).reshape(want.shape), want), (k, h.shape, A, with_append)


def test_resize_rows_src_of_outside_the_source_writes_zeros_and_many_tensors_take_several_launches():
    rng = np.random.default_rng(0)
    N, A = 37, 3
    host = [rng.standard_normal((N, 1 + k % 5)).astype(F32) for k in range(70)]
    tensors = [torch.from_numpy(h).to(DEV) for h in host]
    rows = np.array([5, -1, 36, 37, 2 ** 31 - 1, -2 ** 31, 0], np.int32)
    from bloomscene_amd import _capi
    assert _capi.lib().bsr_resize_max_tensors() < 70
    got = _A().resize_rows(tensors, torch.from_numpy(rows).to(DEV), 7, fills=[float(k) for k in range(70)], n_append=A)
    for k, h in enumerate(host):
        want = AR.resize_ref(h, rows, 7, A, None, _fill_bits(float(k), F32), None)
        assert np.array_equal(_bits(got[k]).reshape(want.shape), want), k
        assert (want[[1, 3, 4, 5]] == 0).all() and (want[7:].view(F32) == k).all()


def test_resize_rows_captured_and_replayed_gives_the_same_bits():
    rng = np.random.default_rng(1)
    N, A = 1025, 100
    tensors, host, ops = _resize_case(N, rng)
    dev_ops = [op if op is None or op[0] != "zero_flagged" else (op[0], torch.from_numpy(op[1]).to(DEV), op[2], op[3])
               for op in ops]
    rows = _keep_rows(N, "random", rng)
    src_of = torch.from_numpy(rows.astype(np.int32)).to(DEV)
    appends = [torch.from_numpy(rng.standard_normal((A,) + h.shape[1:]).astype(F32)).to(DEV) if h.dtype == F32 else None
               for h in host]
    outs = [torch.zeros((rows.shape[0] + A) * int(np.prod(h.shape[1:])), dtype=t.dtype, device=DEV) for h, t in zip(host, tensors)]
    call = lambda: _A().resize_rows(tensors, src_of, rows.shape[0], appends, None, dev_ops, out=outs)
    call()
    torch.cuda.synchronize()
    eager = [_bits(o).copy() for o in outs]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            call()
        for o in outs:
            o.zero_()
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    for o, e in zip(outs, eager):
        assert np.array_equal(_bits(o), e)
    for k, (h, a, op) in enumerate(zip(host, appends, ops)):
        want = AR.resize_ref(h, rows, rows.shape[0], A, None if a is None else a.cpu().numpy(), 0, op)
        assert np.array_equal(eager[k].reshape(want.shape), want), k


# ---- adjust_anchor end to end ----

def _optimizer(kind):
    if kind == "torch":
        return lambda groups: torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    from bloomscene_amd.optim import Adam
    return lambda groups: Adam(groups, lr=0.0, eps=1e-15, capturable=(kind == "capturable"))


def _on_device(fn):
    return lambda x: fn(torch.from_numpy(np.ascontiguousarray(x, F32)).to(DEV)).cpu().numpy()


def _crafted_state(N, F, K):
    """make_state plus two crafted offsets: j0 = (anchor 0, offset 0) is a level-0 candidate whose voxel (28, 28, 28) of
    level 0 lies outside the anchor cloud, so it becomes a new anchor at 4.48; j1 = (anchor 1, offset 0) is a level-1
    candidate at 4.485, in the level-1 voxel (112, 112, 112) that ONLY that level-0 addition occupies."""
    state = AR.make_state(N, F, K, seed=F)
    rng = np.random.default_rng(F + 1)
    rand = [rng.random(N * K).astype(F32) for _ in range(3)]
    P = state["params"]
    from anchor_state_reference import quantize_anchor_np
    lattice = quantize_anchor_np(P["anchor"], state["bound_min"], state["bound_max"]).astype(np.float64)
    scale = np.exp(P["scaling"][:, :3].astype(np.float64))
    for a, target, g in ((0, 4.5, 0.0003), (1, 4.485, 0.0006)):
        P["offset"][a, 0] = ((target - lattice[a]) / scale[a]).astype(F32)
        state["offset_denom"][a * K] = 100
        state["offset_gradient_accum"][a * K] = F32(g) * F32(100)
    rand[0][0], rand[0][K], rand[1][K], rand[2][K] = 0.9, 0.1, 0.9, 0.1
    return state, rand


def _compare(model, want, what):
    got = model.state()
    for name in AR.PARAMS:
        assert got["params"][name].shape == want["params"][name].shape, (what, name)
        assert np.array_equal(got["params"][name].view(np.uint32), want["params"][name].view(np.uint32)), (what, name)
    assert set(got["moments"]) == set(want["moments"]), what
    for name, pair in want["moments"].items():
        for a, b in zip(got["moments"][name], pair):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, name)
    for name in ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom", "max_radii2D"):
        assert got[name].shape == want[name].shape, (what, name)
        assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), (what, name)
    return got


@pytest.mark.parametrize("kind", ["default", "capturable", "torch"])
@pytest.mark.parametrize("F", [32, 50])
def test_adjust_anchor_end_to_end(F, kind):
    N, K = 2000, 10
    state, rand = _crafted_state(N, F, K)
    fused, eager = (AR.Model(state, DEV, _optimizer(kind)) for _ in range(2))
    for m in (fused, eager):
        m.two_steps()
    before = fused.state()
    assert set(before["moments"]) == set(AR.PARAMS) - {"opacity", "rotation"}
    fns = dict(rule="reciprocal", exp_fn=_on_device(torch.exp), log_fn=_on_device(torch.log))
    want, levels = AR.adjust_anchor_ref(before, fused, rand, **fns)
    # every branch occurs: all three levels add, rows are pruned, reset but kept, untouched; a candidate voxel is occupied by
    # an old anchor; and one only by a level-0 addition (without the level-0 candidate j0, level 1 adds one anchor more)
    n_new = want["params"]["anchor"].shape[0]
    d, s = before["anchor_demon"].reshape(-1), before["opacity_accum"].reshape(-1)
    pruned = (d > 80) & (s < F32(0.005) * d)
    assert all(v > 0 for v in levels) and 0 < pruned.sum() < N and n_new == N - pruned.sum() + sum(levels)
    assert ((d > 80) & ~pruned).any() and (d <= 80).any()
    without_j0 = [r.copy() for r in rand]
    without_j0[0][0] = 0.1
    assert AR.adjust_anchor_ref(before, fused, without_j0, **fns)[1] == [levels[0] - 1, levels[1] + 1, levels[2]]
    rand_dev = [torch.from_numpy(r).to(DEV) for r in rand]
    _A().adjust_anchor(fused, rand=rand_dev)
    after = _compare(fused, want, "fused")
    assert after["names"] == before["names"] and after["steps"] == before["steps"] == {n: 2.0 for n in before["moments"]}
    assert fused._offset.shape == (n_new, K, 3) and fused._mask.shape == (n_new, K, 1) and fused.max_radii2D.shape == (n_new,)
    for g in fused.optimizer.param_groups:
        if g["name"] in AR.PARAMS:
            assert g["params"][0] is getattr(fused, "_" + g["name"]) and g["params"][0].requires_grad
            assert (g["params"][0] in fused.optimizer.state) == (g["name"] in before["moments"])
    if kind == "capturable":
        assert all(st["step"].is_cuda for st in fused.optimizer.state.values())
    # the eager GM sequence on the device gives the same (no decision of this case lies near a threshold)
    AR.eager_adjust(eager, rand=rand_dev)
    _compare(eager, want, "eager")
    # one optimizer step on the new arrays
    gen = torch.Generator().manual_seed(5)
    grads = {}
    for g in fused.optimizer.param_groups:
        p = g["params"][0]
        grads[g["name"]] = torch.randn(p.shape, generator=gen) * 0.01
        p.grad = grads[g["name"]].to(DEV)
    lrs = {g["name"]: float(g["lr"]) for g in fused.optimizer.param_groups}
    fused.optimizer.step()
    stepped = fused.state()
    for name in AR.PARAMS:
        m, v = want["moments"].get(name, (np.zeros_like(want["params"][name]),) * 2)
        t = 3 if name in want["moments"] else 1
        p1, m1, v1 = AREF.adam_step(want["params"][name], grads[name].numpy(), m, v, lrs[name], t, eps=1e-15)
        assert stepped["steps"][name] == float(t)
        if kind != "torch":       # (torch's own Adam is within the deviations include/bloomscene_adam.h lists, not bit-equal)
            assert AREF.bits_equal(stepped["params"][name], p1), name
            assert AREF.bits_equal(stepped["moments"][name][0], m1) and AREF.bits_equal(stepped["moments"][name][1], v1), name
        else:
            assert np.allclose(stepped["params"][name], p1, rtol=1e-5, atol=1e-7), name
