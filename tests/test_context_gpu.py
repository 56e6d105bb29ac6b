"""The context head on the GPU (include/bloomscene_context.h, bloomscene_amd/context.py) against tests/context_reference.py:
context and pre1 bit for bit with the numpy evaluation of the header's chains, the elementwise tails bit for bit (or, past
a tanh, within its stated ulps) from the kernel's own Q, and everything that holds a transcendental of a chain or a sum
over rows against float64 autograd of the restatement (with the gate of the fp32 chain), with the fp32 eager lines on the
same GPU as the measure of what fp32 can do:

    kernel error <= 2 x eager error + 2^-23        (helpers.max_err_over_scale, pooled over the small n per shape)

Rows, relative to the kernels' tiles (64 rows a workgroup, ranges of 256 rows in the weight sums): 1, 2, 63, 64, 65, 127,
255, 256, 257; the product shape once at 4099 rows, 17 ranges.  Every case is evaluated once and shared."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import context_reference as CR
import helpers as Hh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((48, 100, 50, 10), (1, 1, 1, 1), (7, 9, 3, 2), (128, 128, 64, 16))
SMALL_N = (1, 2, 63, 64, 65, 127, 255, 256, 257)
BIG = (48, 100, 50, 10, 4099)
FLOOR = 2.0 ** -23
OUT_NAMES = ("context", "Q", "feat", "grid_scaling", "grid_offsets")


def _C():
    import bloomscene_amd.context as Cx
    return Cx


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _leaves(s, grad=True, weights_grad=True):
    d = lambda t, g: t.to(DEV).clone().requires_grad_(g)
    return SimpleNamespace(enc=d(s.enc, grad), feat=d(s.feat, grad), gs=d(s.grid_scaling, grad), go=d(s.grid_offsets, grad),
                           weights=[d(w, grad and weights_grad) for w in s.weights], noise=tuple(t.to(DEV) for t in s.noise),
                           means=[m.to(DEV) for m in s.means])


def _grads(l):
    g = lambda t: None if t.grad is None else t.grad.detach().cpu().numpy()
    return [g(t) for t in (l.enc, l.feat, l.gs, l.go, *l.weights)]       # CR.GRAD_NAMES


def _head(l, s):
    return _C().context_head_tensors(l.enc, l.weights, s.F, s.K, l.feat, l.gs, l.go, l.noise, s.q)


def _kernel(s, use=(0, 1, 2, 3, 4), **kw):
    """forward + backward of the fused call -> outputs (numpy), gradients"""
    l = _leaves(s, **kw)
    outs = _head(l, s)
    sum((outs[i] * s.ups[i].to(DEV)).sum() for i in use).backward()
    torch.cuda.synchronize()
    return [o.detach().cpu().numpy() for o in outs], _grads(l)


def _eager(s, gate, use=(0, 1, 2, 3, 4)):
    l = _leaves(s)
    outs = CR.restatement(l.enc, l.weights, s.F, s.K, l.feat, l.gs, l.go, l.noise, s.q, torch.as_tensor(gate, device=DEV))
    sum((outs[i] * s.ups[i].to(DEV)).sum() for i in use).backward()
    return [o.detach().cpu().numpy() for o in outs], _grads(l)


def _quantise(s, enc=None):
    l = _leaves(s, grad=False)
    out = _C().context_quantise_tensors(l.enc if enc is None else enc.to(DEV), l.weights, s.F, s.K, l.feat, l.gs, l.go, *l.means,
                                        q=s.q, steps=True)
    return [t.cpu().numpy() for t in out]                               # feat, grid_scaling, grid_offsets, Q


@functools.lru_cache(maxsize=None)
def _case(D, H, F, K, n):
    """the numpy chains, float64 autograd, the eager fp32 lines and the kernels for one call, computed once"""
    s = CR.scene(n, D, H, F, K, seed=n)
    c = SimpleNamespace(s=s)
    c.np = CR.forward_np(s.enc.numpy(), [w.numpy() for w in s.weights], F, K, s.q)
    c.ref = CR.autograd64(s, gate=c.np.gate)
    l = _leaves(s, grad=False)
    c.maps = [t.cpu().numpy() for t in _C().context_head_maps(l.enc, l.weights, F, K, l.feat, l.gs, l.go, l.noise, s.q)]
    c.out, c.grad = _kernel(s)
    c.eager_out, c.eager_grad = _eager(s, c.np.gate.astype(np.float32))
    c.quant = _quantise(s)
    return c


def _cases(D, H, F, K):
    return [_case(D, H, F, K, n) for n in SMALL_N]


def _with_big(shape):
    return _cases(*shape) + ([_case(*BIG)] if shape == BIG[:4] else [])


def _rule(label, got, eager, ref):
    err, eager_err = Hh.max_err_over_scale(got, ref), Hh.max_err_over_scale(eager, ref)
    print(f"[context] {label:40s} kernel {err:.3e} eager {eager_err:.3e}")
    assert np.isfinite(got).all(), label
    assert err <= 2 * eager_err + FLOOR, (label, err, eager_err)


def _cat(xs):
    return np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in xs])


def _gradient_rule(label, cases):
    for i, name in enumerate(CR.GRAD_NAMES):
        if name in ("d_feat", "d_scaling", "d_offsets"):
            continue                                    # (the identity: pinned bit for bit below)
        _rule(f"{label} {name}", _cat(c.grad[i] for c in cases), _cat(c.eager_grad[i] for c in cases), _cat(c.ref.grads[i] for c in cases))
    for c in cases:                                     # the gradient to x is the upstream itself
        for i in (1, 2, 3):
            assert (_bits(c.grad[i]) == _bits(c.s.ups[i + 1])).all(), (c.s.n, CR.GRAD_NAMES[i])


@pytest.mark.parametrize("D,H,F,K", SHAPES)
def test_context_and_pre1_are_the_headers_chains_bit_for_bit(D, H, F, K):
    for c in _with_big((D, H, F, K)):
        n = c.s.n
        context, Q, pre1 = c.maps[0], c.maps[1], c.maps[5]
        assert context.shape == (n, CR.outputs(F, K)) and pre1.shape == (n, H) and Q.shape == (n, 3)
        assert (_bits(pre1) == _bits(c.np.pre1)).all(), (n, "pre1")
        assert (_bits(context) == _bits(c.np.pre2)).all(), (n, "context")
        assert (_bits(Q) == _bits(c.np.Q)).all(), (n, "Q")                 # (the same form on the same bits)
        for got, again in zip(c.out, c.maps[:5]):      # the differentiable call writes the same outputs
            assert got.shape == again.shape and (_bits(got) == _bits(again)).all()
        assert c.out[4].shape == (n, K, 3)
        # the inference form runs the same chain on three rows: the training form's Q
        assert (_bits(c.quant[3]) == _bits(Q)).all(), (n, "the quantiser's Q")


@pytest.mark.parametrize("D,H,F,K", SHAPES)
def test_step_sizes_against_float64(D, H, F, K):
    cases = _cases(D, H, F, K)
    _rule(f"({D}, {H}, {F}, {K}) Q", _cat(c.out[1] for c in cases), _cat(c.eager_out[1] for c in cases), _cat(c.ref.outs[1] for c in cases))
    adj = np.concatenate([c.np.adj.reshape(-1) for c in cases])
    if D > 1:
        assert (np.abs(adj) < 0.25).any() and (np.abs(adj) > 1.0).any()     # both branches of the tanh form


@pytest.mark.parametrize("D,H,F,K", SHAPES)
def test_noised_outputs_are_the_source_order_bit_for_bit(D, H, F, K):
    for c in _with_big((D, H, F, K)):
        s = c.s
        for i, (x, noise) in enumerate(zip((s.feat, s.grid_scaling, s.grid_offsets), s.noise)):
            want = CR.noised_np(x.numpy(), noise.numpy(), c.out[1][:, i])
            assert (_bits(c.out[2 + i]) == _bits(want)).all(), (s.n, OUT_NAMES[2 + i])


def _quantiser_holds(s, quant):
    """From the kernel's own Q numpy reproduces lo, hi, the clamp, x / Q, rint, Qq and d = x - Qq exactly; what is left is
    out = Qq + tanh(d) Q: 4 ulp of tanh (|tanh| <= 1: 4 * 2^-24 |Q| at most), one rounding of the product (2^-24 |Q|), one
    of the sum (2^-24 |out|) -- 6 * 2^-24 |Q| + 2^-24 |out| with the slack of one more rounding of Q's size.  Every element."""
    binds = 0
    for i, x in enumerate((s.feat, s.grid_scaling, s.grid_offsets)):
        z = CR.quantise_np(x.numpy(), quant[3][:, i], s.means[i].numpy())
        got = quant[i]
        assert got.shape == z.out64.shape
        nan = np.isnan(z.out64)
        assert (np.isnan(got) == nan).all(), OUT_NAMES[2 + i]
        err = np.abs(got.astype(np.float64) - z.out64)
        tol = 6 * 2.0 ** -24 * np.abs(z.Q.astype(np.float64)) + 2.0 ** -24 * np.abs(z.out64)
        worst = float(np.max((err / np.maximum(tol, 1e-300))[~nan], initial=0.0))
        print(f"[context] quantiser n = {s.n:5d} {OUT_NAMES[2 + i]:13s} worst error / bound {worst:.3f}  clamped {int(z.bound.sum())}")
        assert (err[~nan] <= tol[~nan]).all(), (s.n, OUT_NAMES[2 + i], worst)
        binds += int(z.bound[~nan].sum())
    return binds


@pytest.mark.parametrize("D,H,F,K", SHAPES)
def test_quantiser_from_the_kernels_own_step_sizes(D, H, F, K):
    binds = 0
    for c in _with_big((D, H, F, K)):
        binds += _quantiser_holds(c.s, c.quant)
        assert not np.isnan(c.quant[3]).any()
    if D > 1:
        assert binds > 0                                # rows where the clamp binds
        ratio = np.abs(_case(D, H, F, K, 257).s.grid_scaling.numpy() / _case(D, H, F, K, 257).quant[3][:, 1:2])
        assert ratio.max() > 1000.0                     # thousands of steps in the scaling column
    # a NaN row: its three outputs and its Q are NaN, no other row is touched
    c = _case(D, H, F, K, 65)
    enc = c.s.enc.clone()
    enc[3] = float("nan")
    quant = _quantise(c.s, enc)
    _quantiser_holds(c.s, quant)
    keep = np.arange(65) != 3
    for got, full in zip(quant, c.quant):
        assert np.isnan(got[3]).all()
        assert (_bits(got[keep]) == _bits(full[keep])).all()


@pytest.mark.parametrize("D,H,F,K", SHAPES)
def test_gradients_against_float64_autograd(D, H, F, K):
    _gradient_rule(f"({D}, {H}, {F}, {K})", _cases(D, H, F, K))


def test_gradients_where_several_ranges_meet():
    c = _case(*BIG)
    _gradient_rule("product n = 4099", [c])
    _rule("product n = 4099 Q", c.out[1], c.eager_out[1], c.ref.outs[1])


def test_rows_are_pure_functions_of_their_row():
    D, H, F, K, n = 48, 100, 50, 10, 257
    c = _case(D, H, F, K, n)
    s = c.s
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    p = SimpleNamespace(**vars(s))
    p.enc, p.feat, p.grid_scaling, p.grid_offsets = (t[perm] for t in (s.enc, s.feat, s.grid_scaling, s.grid_offsets))
    p.noise, p.ups = tuple(t[perm] for t in s.noise), tuple(t[perm] for t in s.ups)
    out, grad = _kernel(p)
    for got, full in zip(out, c.out):
        assert (_bits(got) == _bits(full[perm.numpy()])).all()
    assert (_bits(grad[0]) == _bits(c.grad[0][perm.numpy()])).all()
    quant = _quantise(p)
    for got, full in zip(quant, c.quant):
        assert (_bits(got) == _bits(full[perm.numpy()])).all()
    # enc and feat as views with a wider row stride: the bits of the contiguous copies, a dense gradient to the view's base
    wide = torch.randn(n, 2 * D)
    wide[:, :D] = s.enc
    base = wide.to(DEV).requires_grad_(True)
    widef = torch.randn(n, F + 3)
    widef[:, 3:] = s.feat
    basef = widef.to(DEV).requires_grad_(True)
    l = _leaves(s)
    view, viewf = base[:, :D], basef[:, 3:]
    assert view.stride() == (2 * D, 1) and viewf.stride() == (F + 3, 1)
    outs = _C().context_head_tensors(view, l.weights, F, K, viewf, l.gs, l.go, l.noise, s.q)
    sum((o * u.to(DEV)).sum() for o, u in zip(outs, s.ups)).backward()
    for got, full in zip(outs, c.out):
        assert (_bits(got) == _bits(full)).all()
    assert (_bits(base.grad[:, :D]) == _bits(c.grad[0])).all() and not base.grad[:, D:].any()
    assert (_bits(basef.grad[:, 3:]) == _bits(s.ups[2])).all() and not basef.grad[:, :3].any()
    for got, full in zip(l.weights, c.grad[4:]):
        assert (_bits(got.grad) == _bits(full)).all()
    quant = _C().context_quantise_tensors(view.detach(), l.weights, F, K, viewf.detach(), l.gs.detach(), l.go.detach(), *l.means, q=s.q)
    for got, full in zip(quant, c.quant):
        assert (_bits(got) == _bits(full)).all()


def test_two_runs_give_the_same_bits():
    c = _case(*BIG)
    out, grad = _kernel(c.s)
    for a, b in zip(out, c.out):
        assert (_bits(a) == _bits(b)).all()
    for name, a, b in zip(CR.GRAD_NAMES, grad, c.grad):
        assert (_bits(a) == _bits(b)).all(), name
    for a, b in zip(_quantise(c.s), c.quant):
        assert (_bits(a) == _bits(b)).all()


def test_absent_upstreams_and_frozen_weights():
    D, H, F, K, n = 48, 100, 50, 10, 257
    c = _case(D, H, F, K, n)
    s = c.s
    O = CR.outputs(F, K)
    # the noised feat alone: the others' upstreams are None.  It reaches the weights through Q[0] = column O - 3 only
    out, grad = _kernel(s, use=(2,))
    ref = CR.autograd64(s, gate=c.np.gate, use=(2,))
    _, eager = _eager(s, c.np.gate.astype(np.float32), use=(2,))
    assert (_bits(grad[1]) == _bits(s.ups[2])).all() and grad[2] is None and grad[3] is None
    others = np.arange(O) != O - 3
    assert not grad[6][others].any() and not grad[7][others].any() and grad[6][O - 3].any()
    for i in (0, 4, 5, 6, 7):
        _rule(f"feat only {CR.GRAD_NAMES[i]}", grad[i], eager[i], ref.grads[i])
    # context alone (no upstream reaches Q)
    out, grad = _kernel(s, use=(0,))
    ref = CR.autograd64(s, gate=c.np.gate, use=(0,))
    _, eager = _eager(s, c.np.gate.astype(np.float32), use=(0,))
    assert grad[1] is None and grad[2] is None and grad[3] is None
    for i in (0, 4, 5, 6, 7):
        _rule(f"context only {CR.GRAD_NAMES[i]}", grad[i], eager[i], ref.grads[i])
    # frozen weights: only enc (and the attributes) receive a gradient -- the same bits, without the sums or their scratch
    l = _leaves(s, weights_grad=False)
    outs = _head(l, s)
    ups = [u.to(DEV) for u in s.ups]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    d_enc, d_feat = torch.autograd.grad(outs, (l.enc, l.feat), ups)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert (_bits(d_enc) == _bits(c.grad[0])).all() and (_bits(d_feat) == _bits(s.ups[2])).all()
    assert peak <= n * D * 4 + 4 * 512, peak           # d enc alone: no scratch (it would be n * 440 * 4 bytes)
    assert all(w.grad is None for w in l.weights)


def test_no_grad_allocates_the_outputs_only():
    D, H, F, K, n = BIG
    s = _case(*BIG).s
    l = _leaves(s, grad=False)
    with torch.no_grad():
        _head(l, s)                                     # (loads everything)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        outs = _head(l, s)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    outputs = sum(o.numel() * 4 for o in outs)
    assert outputs == n * (CR.outputs(F, K) + 3 + F + 6 + 3 * K) * 4
    assert peak <= outputs + 5 * 512, (peak, outputs)   # (the allocator's rounding per tensor)
    assert peak < outputs + n * H * 4


def test_no_rows():
    Cx = _C()
    D, H, F, K = 48, 100, 50, 10
    s = CR.scene(0, D, H, F, K)
    l = _leaves(s)
    outs = _head(l, s)
    assert [tuple(o.shape) for o in outs] == [(0, CR.outputs(F, K)), (0, 3), (0, F), (0, 6), (0, K, 3)]
    sum(o.sum() for o in outs).backward()
    assert l.enc.grad.shape == (0, D) and l.feat.grad.shape == (0, F) and l.go.grad.shape == (0, K, 3)
    for w in l.weights:
        assert w.grad is not None and w.grad.shape == w.shape and not w.grad.any()
    maps = Cx.context_head_maps(l.enc.detach(), [w.detach() for w in l.weights], F, K)
    assert maps[5].shape == (0, H) and maps[2] is None and maps[3] is None and maps[4] is None
    quant = Cx.context_quantise_tensors(l.enc.detach(), [w.detach() for w in l.weights], F, K, l.feat.detach(), l.gs.detach(),
                                        l.go.detach(), *l.means, steps=True)
    assert [tuple(t.shape) for t in quant] == [(0, F), (0, 6), (0, K, 3), (0, 3)]


def test_outputs_for_absent_attributes_are_none_and_the_module_is_the_function():
    Cx = _C()
    D, H, F, K, n = 7, 9, 3, 2, 65
    c = _case(D, H, F, K, n)
    s = c.s
    l = _leaves(s, grad=False)
    context, Q, feat, gs, go = Cx.context_head_tensors(l.enc, l.weights, F, K, grid_scaling=l.gs, noise=(None, l.noise[1], None))
    assert feat is None and go is None
    assert (_bits(context) == _bits(c.out[0])).all() and (_bits(Q) == _bits(c.out[1])).all() and (_bits(gs) == _bits(c.out[3])).all()
    only = Cx.context_quantise_tensors(l.enc, l.weights, F, K, None, None, l.go, None, None, l.means[2])
    assert only[0] is None and only[1] is None and (_bits(only[2]) == _bits(c.quant[2])).all()
    mlp = torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.ReLU(True), torch.nn.Linear(H, CR.outputs(F, K))).to(DEV)
    with torch.no_grad():
        for p, w in zip((mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias), l.weights):
            p.copy_(w)
    head = Cx.ContextHead(mlp, F, K)
    for got, full in zip(head(l.enc, l.feat, l.gs, l.go, l.noise), c.out):
        assert (_bits(got) == _bits(full)).all()
    for got, full in zip(head.quantise(l.enc, l.feat, l.gs, l.go, *l.means), c.quant):
        assert (_bits(got) == _bits(full)).all()
    assert not head.quantise(l.enc, l.feat, l.gs, l.go, *l.means)[0].requires_grad


def test_double_backward_is_refused():
    s = CR.scene(5, 7, 9, 3, 2)
    l = _leaves(s)
    out = _head(l, s)[0]
    g, = torch.autograd.grad(out.sum(), l.enc, create_graph=True)
    with pytest.raises(RuntimeError):         # (no graph behind the gradient: it is never treated as a constant silently)
        g.sum().backward()


def test_context_rates_takes_the_heads_step_sizes():
    """entropy.context_rates(steps=Q) against context_rates evaluating GR:82-84 itself (torch's tanh), both against the
    float64 restatement of tests/entropy_reference.py.  Q comes from the kernel for the SAME adjustment bits: a head with
    D = 3, H = 6 whose layers are +-identity gives pre2 = relu(a) - relu(-a) = a exactly."""
    import entropy_reference as ER
    from bloomscene_amd import entropy as E
    Cx = _C()
    n, F, K = 257, 50, 10
    gen = torch.Generator().manual_seed(11)
    randn = lambda *s: torch.randn(s, generator=gen)
    widths = CR.split_sizes(F, K)
    at = np.cumsum([0] + widths)
    context = randn(n, sum(widths))
    for i in (1, 3, 5):                                   # the three scale blocks: positive
        context[:, at[i]:at[i + 1]] = 0.3 * torch.exp(context[:, at[i]:at[i + 1]])
    context[:, at[2]:at[4]] *= 1e-3                        # scaling and offsets live on their own quantisation steps
    context[:, at[4]:at[6]] *= 0.2
    context[:, at[6]:] *= 0.5
    feat = (context[:, :F] + randn(n, F) * context[:, at[1]:at[2]]).contiguous()
    grid_scaling = (context[:, at[2]:at[3]] + randn(n, 6) * context[:, at[3]:at[4]]).contiguous()
    grid_offsets = (context[:, at[4]:at[5]] + randn(n, 3 * K) * context[:, at[5]:at[6]]).reshape(n, K, 3).contiguous()
    choose = torch.rand(n, generator=gen) <= 0.2
    choose[-1] = True
    grid_masks = (torch.rand(n, K, 1, generator=gen) < 0.6).float()
    args = [feat, grid_scaling, grid_offsets, context, choose, grid_masks, torch.tensor(0.83), feat.mean(), grid_scaling.mean(),
            grid_offsets.mean()]
    ref = ER.rate_terms(*[a.double() if a.is_floating_point() else a for a in args], F, K)
    eye = torch.eye(3)
    O1 = CR.outputs(1, 1)
    W2 = torch.zeros(O1, 6)
    W2[-3:] = torch.cat([eye, -eye], dim=1)
    weights = [torch.cat([eye, -eye], dim=0), torch.zeros(6), W2, torch.zeros(O1)]
    adj = context[:, at[6]:].contiguous()
    pre2, Q = Cx.context_head_tensors(adj.to(DEV), [w.to(DEV) for w in weights], 1, 1)[:2]
    assert (_bits(pre2[:, -3:]) == _bits(adj)).all()
    dev = [a.to(DEV) for a in args]
    with_steps = E.context_rates(*dev, F, K, steps=Q)
    without = E.context_rates(*dev, F, K)
    vec = lambda ts: np.array([float(t) for t in ts], np.float64)
    _rule("context_rates(steps=Q)", vec(with_steps), vec(without), vec(ref))
    with pytest.raises(ValueError, match=r"steps must be \[257, 3\]"):
        E.context_rates(*dev, F, K, steps=Q[:, :2])


@pytest.mark.parametrize("D,H,F,K", ((48, 100, 50, 10), (128, 128, 64, 16)))
def test_both_forms_replay_from_a_graph_without_a_host_wait(D, H, F, K):
    """Forward + backward of the training form and the inference form captured with torch.cuda.graph after one warm-up call
    (capture raises on any host wait), on one stream, and replayed on new input values: bit-equal to the direct call.
    (128, 128, 64, 16): the row pass asks for 129 KB of LDS."""
    Cx = _C()
    n = 257
    s, s2 = CR.scene(n, D, H, F, K, seed=31), CR.scene(n, D, H, F, K, seed=32)
    l = _leaves(s)
    ups = [u.to(DEV) for u in s.ups]
    noise = list(l.noise)
    leaves = [l.enc, l.feat, l.gs, l.go] + l.weights

    def step():
        outs = Cx.context_head_tensors(l.enc, l.weights, F, K, l.feat, l.gs, l.go, tuple(noise), s.q)
        grads = torch.autograd.grad(outs, leaves, ups)
        quant = Cx.context_quantise_tensors(l.enc.detach(), [w.detach() for w in l.weights], F, K, l.feat.detach(), l.gs.detach(),
                                            l.go.detach(), *l.means, q=s.q)
        return tuple(outs) + tuple(grads) + tuple(quant)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = step()[0].clone()                        # the warm-up: loads the library, asks for the LDS
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    l2 = _leaves(s2)
    with torch.no_grad():                                # new values in the captured tensors
        for dst, src in zip(leaves + ups + noise + l.means,
                            [l2.enc, l2.feat, l2.gs, l2.go] + l2.weights + [u.to(DEV) for u in s2.ups] + list(l2.noise) + l2.means):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    direct = step()
    torch.cuda.synchronize()
    assert not torch.equal(replayed[0], first)
    for a, b in zip(replayed, direct):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
