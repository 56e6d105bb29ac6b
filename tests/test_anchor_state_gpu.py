"""The anchor state on the GPU (include/bloomscene_anchor_state.h, bloomscene_amd/anchor_state.py) against
tests/anchor_state_reference.py: every output of ``visible`` bit for bit with the numpy restatement, the exact ones equal
to the eager lines on the same GPU, the dense gradients bit for bit from the upstream rows (``d_mask`` against float64
autograd by the siblings' rule, kernel error <= 2 x eager error + 2^-23 of the tensor's scale), and ``accumulate`` bit
for bit with its restatement on pre-filled accumulators.

Shapes (N, F, K): (300, 32, 10), (129, 5, 3), (64, 1, 1) with n in 0, 1, 65, N (65 only where N allows it): 16 rows a wave
and 64 a workgroup, so 65 and 129 leave partial waves and 300 spans five workgroups; n K = 3000 spans three scan blocks
of 1024 candidates.  Every case is evaluated once and shared."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import anchor_state_reference as AR
import helpers as Hh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((300, 32, 10), (129, 5, 3), (64, 1, 1))
CASES = [(N, F, K, n) for N, F, K in SHAPES for n in sorted({0, 1, 65, N}) if n <= N]
FLOOR = 2.0 ** -23
IN_NAMES = ("anchor", "feat", "offset", "scaling", "mask")
f32 = np.float32


def _A():
    import bloomscene_amd.anchor_state as AS
    return AS


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _leaves(s, grad=IN_NAMES, feat_pad=0):
    d = lambda t, g=False: torch.from_numpy(t).to(DEV).clone().requires_grad_(g)
    l = SimpleNamespace(idx=d(s.idx), bmin=d(s.bmin)[None], bmax=d(s.bmax)[None])
    for name in IN_NAMES:
        setattr(l, name, d(getattr(s, name), name in grad))
    l.feat_arg = l.feat
    if feat_pad:
        wide = torch.cat([l.feat, torch.zeros(s.N, feat_pad, device=DEV)], dim=1)
        l.feat_arg = wide[:, :s.F]
        assert l.feat_arg.stride(0) == s.F + feat_pad
    return l


def _args(l):
    return l.idx, l.anchor, l.bmin, l.bmax, l.feat_arg, l.offset, l.scaling, l.mask


def _grads(l):
    return [None if getattr(l, name).grad is None else getattr(l, name).grad.detach().cpu().numpy() for name in IN_NAMES]


def _run(s, fn, **kw):
    """forward + backward with all five upstreams -> outputs (numpy), dense gradients"""
    l = _leaves(s, **kw)
    outs = fn(*_args(l))
    sum((outs[i] * torch.from_numpy(s.ups[i]).to(DEV)).sum() for i in range(5)).backward()
    torch.cuda.synchronize()
    return [o.detach().cpu().numpy() for o in outs], _grads(l)


@functools.lru_cache(maxsize=None)
def _case(N, F, K, n):
    s = AR.scene(N, F, K, n)
    ref = AR.visible_np(s.idx, s.anchor, s.bmin, s.bmax, s.feat, s.offset, s.scaling, s.mask)
    outs, grads = _run(s, _A().visible)
    return SimpleNamespace(s=s, ref=ref, outs=outs, grads=grads)


@functools.lru_cache(maxsize=None)
def _eager(N, F, K, n):
    s = AR.scene(N, F, K, n)
    outs, grads = _run(s, AR.eager_visible)
    return SimpleNamespace(outs=outs, grads=grads)


@pytest.mark.parametrize("N,F,K,n", CASES)
def test_forward_is_the_restatement_bit_for_bit(N, F, K, n):
    c = _case(N, F, K, n)
    assert n < 2 or (c.s.idx[0] == 0 and c.s.idx[-1] == N - 1)
    for i, name in enumerate(("anchor", "feat", "grid_offsets", "grid_scaling", "binary_grid_masks")):
        assert c.outs[i].shape == c.ref[i].shape and (_bits(c.outs[i]) == _bits(c.ref[i])).all(), name
    assert c.outs[5].dtype == np.bool_ and np.array_equal(c.outs[5], c.ref[5])
    assert c.outs[6].shape == () and c.outs[6].dtype == f32
    assert _bits(c.outs[6]) == _bits(c.ref[6]) or (n == 0 and np.isnan(c.outs[6]))
    if n >= 65:
        b = c.outs[4]
        assert 0.3 < b.mean() < 0.7 and 0 < c.outs[5].sum() < n          # half of the decisions 0, some anchors all zero


@pytest.mark.parametrize("N,F,K,n", CASES)
def test_forward_against_the_eager_lines_on_the_gpu(N, F, K, n):
    c, e = _case(N, F, K, n), _eager(N, F, K, n)
    for i in (0, 1, 2):
        assert (_bits(c.outs[i]) == _bits(e.outs[i])).all(), i
    assert np.array_equal(c.outs[4] > 0.5, e.outs[4] > 0.5)
    assert np.array_equal(c.outs[5], e.outs[5])
    assert _bits(c.outs[6]) == _bits(e.outs[6]) or (n == 0 and np.isnan(c.outs[6]) and np.isnan(e.outs[6]))
    got, ref = c.outs[3].astype(np.float64), e.outs[3].astype(np.float64)
    assert (np.abs(got - ref) <= 3 * np.spacing(np.abs(e.outs[3])).astype(np.float64)).all()    # 3 ulp


def test_a_feature_view_with_a_wider_row_stride_gives_the_same():
    N, F, K, n = 129, 5, 3, 65
    c = _case(N, F, K, n)
    outs, grads = _run(c.s, _A().visible, feat_pad=3)
    for a, b in zip(outs, c.outs):
        assert np.array_equal(a, b, equal_nan=True)
    for a, b in zip(grads, c.grads):
        assert (_bits(a) == _bits(b)).all()


@pytest.mark.parametrize("N,F,K,n", CASES)
def test_backward_writes_the_dense_gradients(N, F, K, n):
    c = _case(N, F, K, n)
    s = c.s
    outside = np.setdiff1d(np.arange(N), s.idx)
    shapes = ((N, 3), (N, F), (N, K, 3), (N, 6), (N, K, 1))
    for g, shape in zip(c.grads, shapes):
        assert g.shape == shape and not _bits(g[outside]).any()                  # exactly +0 outside idx
    for i in (0, 1, 2):
        assert (_bits(c.grads[i][s.idx]) == _bits(s.ups[i])).all(), IN_NAMES[i]
    assert (_bits(c.grads[3][s.idx]) == _bits((s.ups[3] * c.outs[3]).astype(f32))).all()
    # the header's d_mask in numpy: (g * s) * (1 - s) on the library's sigmoid
    sg = AR.sigmoid_form(s.mask[s.idx])
    assert (_bits(c.grads[4][s.idx]) == _bits(((s.ups[4] * sg).astype(f32) * (f32(1) - sg)).astype(f32))).all()
    if n == 0:
        return
    ref = AR.mask_gradient64(s.idx, s.mask, s.ups[4])
    e = _eager(N, F, K, n)
    err, eager_err = Hh.max_err_over_scale(c.grads[4], ref), Hh.max_err_over_scale(e.grads[4], ref)
    print(f"d_mask N={N} K={K} n={n}: kernel {err:.3e} eager {eager_err:.3e}")
    assert err <= 2 * eager_err + FLOOR


def test_backward_is_bit_identical_from_run_to_run_and_skips_what_is_not_asked_for():
    N, F, K, n = 300, 32, 10, 65
    c = _case(N, F, K, n)
    _, again = _run(c.s, _A().visible)
    for a, b in zip(again, c.grads):
        assert (_bits(a) == _bits(b)).all()
    _, some = _run(c.s, _A().visible, grad=("scaling", "mask"))
    assert some[0] is None and some[1] is None and some[2] is None
    assert (_bits(some[3]) == _bits(c.grads[3])).all() and (_bits(some[4]) == _bits(c.grads[4])).all()
    l = _leaves(c.s)
    with torch.no_grad():
        outs = _A().visible(*_args(l))
    assert not any(o.requires_grad for o in outs)
    outs = _A().visible(*_args(l))
    assert not outs[5].requires_grad and not outs[6].requires_grad
    g, = torch.autograd.grad(outs[3].sum(), l.scaling, create_graph=True)
    with pytest.raises(RuntimeError):         # double backward is refused: there is no graph behind the gradient
        g.sum().backward()


def test_check_refuses_a_bad_index_list_and_the_default_path_never_reads_it():
    N, F, K, n = 129, 5, 3, 65
    c = _case(N, F, K, n)
    s = c.s
    l = _leaves(s, grad=())
    for bad in ((3, N), (3, -1), (10, int(s.idx[9]))):                          # out of range twice, then not ascending
        idx = l.idx.clone()
        idx[bad[0]] = bad[1]
        with pytest.raises(ValueError, match="strictly ascending"):
            _A().visible(idx, *_args(l)[1:], check=True)
    _A().visible(*_args(l), check=True)
    # without the check an index out of range is not dereferenced: a zero row that counts for nothing
    idx = s.idx.copy()
    idx[3], idx[40] = -1, N
    ref = AR.visible_np(idx, s.anchor, s.bmin, s.bmax, s.feat, s.offset, s.scaling, s.mask)
    outs = _A().visible(torch.from_numpy(idx).to(DEV), *_args(l)[1:])
    torch.cuda.synchronize()
    for a, b in zip(outs, ref):
        assert np.array_equal(a.cpu().numpy(), b)
    e = AR.epilogue_scene(N, K, n, seed=3)
    got = _accumulate(e, idx=idx)
    want = AR.accumulate_np(e.acc, idx, e.opacity, e.selection, e.radii, e.grad, K)
    for a, b in zip(got, want):
        assert (_bits(a) == _bits(b)).all()


# ---- B ----
def _accumulate(e, idx=None, acc=None):
    d = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(DEV)
    acc = [d(a).clone() for a in (e.acc if acc is None else acc)]
    _A().accumulate(*acc, d(e.idx if idx is None else idx), d(e.opacity), d(e.selection), d(e.radii), d(e.grad))
    torch.cuda.synchronize()
    return [a.cpu().numpy().reshape(-1) for a in acc]


B_CASES = {
    "three_blocks": dict(N=300, K=10, n=300, blocks=("none", "all", "mixed")),
    "short_m": dict(N=300, K=10, n=300, blocks=("all", "mixed", "none"), M=700),
    "padded": dict(N=300, K=10, n=290, blocks=("mixed", "none", "all"), padded=333),
    "bool_filter": dict(N=300, K=10, n=300, bool_filter=True),
    "partial": dict(N=129, K=3, n=65),
    "one": dict(N=64, K=1, n=1),
    "all_k_one": dict(N=64, K=1, n=64),
}


@pytest.mark.parametrize("name", sorted(B_CASES))
def test_accumulate_is_the_restatement_bit_for_bit(name):
    kw = dict(B_CASES[name])
    N, K, n = kw.pop("N"), kw.pop("K"), kw.pop("n")
    e = AR.epilogue_scene(N, K, n, **kw)
    if name == "three_blocks":
        sel = e.selection
        assert sel.size > 2 * AR.SCAN_BLOCK and not sel[:1024].any() and sel[1024:2048].all() and 0 < sel[2048:].sum() < sel.size - 2048
        assert (e.radii == 0).any() and (e.radii > 0).any()
    if name == "short_m":
        assert e.M < e.count
    got = _accumulate(e)
    want = AR.accumulate_np(e.acc, e.idx, e.opacity, e.selection, e.radii, e.grad, K)
    for a, b, label in zip(got, want, ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")):
        assert (_bits(a) == _bits(b)).all(), label
    assert (got[2] != e.acc[2].reshape(-1)).any() or n == 1
    if name == "short_m":       # the selected candidates beyond M are untouched
        cnd = np.nonzero(e.selection)[0][e.M:]
        target = e.idx[cnd // K] * K + cnd % K
        assert (got[2][target] == e.acc[2].reshape(-1)[target]).all() and (got[3][target] == e.acc[3].reshape(-1)[target]).all()


def test_accumulate_norms_are_within_three_ulp_of_float64():
    N, K, n = 300, 10, 300
    e = AR.epilogue_scene(N, K, n, seed=9)
    zero = [np.zeros_like(a) for a in e.acc]
    got = _accumulate(e, acc=zero)
    cnd = np.nonzero(e.selection)[0]
    keep = e.radii[:cnd.size] > 0
    target = (e.idx[cnd // K] * K + cnd % K)[keep]
    g = e.grad[:cnd.size][keep].astype(np.float64)
    norm = np.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2)
    assert norm.min() > 1e-12                                                    # far from underflow
    inc = got[2][target].astype(np.float64)
    assert (np.abs(inc - norm) <= 3 * np.spacing(norm.astype(f32)).astype(np.float64)).all()
    assert (got[3][target] == 1).all() and got[3].sum() == keep.sum()


def test_n_zero_leaves_the_accumulators_alone():
    e = AR.epilogue_scene(64, 1, 0)
    got = _accumulate(e)
    for a, b in zip(got, e.acc):
        assert (_bits(a) == _bits(b.reshape(-1))).all()


def test_one_iteration_is_captured_into_a_graph_and_replayed():
    N, F, K, n = 300, 32, 10, 65
    c = _case(N, F, K, n)
    s = c.s
    e = AR.epilogue_scene(N, K, n, seed=5)
    d = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(DEV)
    l = _leaves(s)
    ups = [d(u) for u in s.ups]
    acc = [d(a).clone() for a in e.acc]
    stat = [d(t) for t in (e.opacity, e.selection, e.radii, e.grad)]
    leaves = [getattr(l, name) for name in IN_NAMES]

    def step():
        outs = _A().visible(*_args(l))
        sum((outs[i] * ups[i]).sum() for i in range(5)).backward()
        _A().accumulate(*acc, l.idx, *stat)
        return outs

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in leaves:
        t.grad = None
    for a, orig in zip(acc, e.acc):
        a.copy_(d(orig))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, c.outs):
        assert np.array_equal(a.detach().cpu().numpy(), b, equal_nan=True)
    for t, b in zip(leaves, c.grads):
        assert (_bits(t.grad) == _bits(b)).all()
    want = _accumulate(e, idx=s.idx)          # (the iteration's index list is the prologue's)
    for a, b in zip(acc, want):
        assert (_bits(a.reshape(-1)) == _bits(b)).all()
