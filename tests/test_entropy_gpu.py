"""The rate term on the GPU (include/bloomscene_entropy.h, bloomscene_amd/entropy.py) against the restatement of
tests/entropy_reference.py: float64 on the CPU is the reference, the same restatement in fp32 eager torch on the GPU is what
the kernels replace, and the kernels must be no further from float64 than that.

Shapes: n in {1, 3, 257} x C in {1, 6, 30, 50, 67} (one lane a row up to more columns than lanes; one row, fewer rows than
a workgroup holds, several workgroups with a ragged last one), operands as split views of one wider matrix, q as one value,
per row and per element.  The two error comparisons order two error DISTRIBUTIONS, which a sample of one element cannot do:
for every (C, q) they are made once over the elements of all three n together.  Everything else is checked per shape."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import entropy_reference as ER
import helpers as Hh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
NS = (1, 3, 257)
CS = (1, 6, 30, 50, 67)
Q_KINDS = ("single", "row", "element")
UNIT = 2.0 ** -24
BAND = 0.25          # |l64 / 1e-6 - 1| <= BAND: the lower-bound gate may fall either way in fp32


def _E():
    import bloomscene_amd.entropy as E
    return E


def _split_views(mat, C):
    return mat[:, 0:C], mat[:, C:2 * C], mat[:, 2 * C:3 * C]


def _width(C):
    return max(175, 3 * C + 7)     # BloomScene's context is 175 wide; wider where three operands do not fit


def _device_matrix(inp, n, C):
    """x, mean, scale side by side in one [n, width] matrix on the GPU: the row stride of each view is not C."""
    mat = torch.zeros(n, _width(C))
    for view, key in zip(_split_views(mat, C), ("x", "mean", "scale")):
        view.copy_(inp[key])
    return mat.to(DEV)


@functools.lru_cache(maxsize=None)
def _case(n, C, q_kind):
    """Inputs, the float64 reference, the fp32 eager evaluation and the kernels' results for one shape, computed once.
    Gradients are for the upstream g ("all") and for g restricted to the elements with l64 >= 1e-3 ("well")."""
    E = _E()
    inp = ER.make_inputs(n, C, seed=1000 * n + 10 * C + Q_KINDS.index(q_kind), q_kind=q_kind)
    c = SimpleNamespace(n=n, C=C, q_kind=q_kind, inp=inp)
    i64 = {k: v.to(F64) for k, v in inp.items()}
    c.l64 = ER.likelihood(i64["x"], i64["mean"], i64["scale"], i64["q"], i64["x_mean"])
    c.band = (c.l64 / ER.FLOOR - 1).abs() <= BAND
    c.well = c.l64 >= 1e-3
    mat = _device_matrix(inp, n, C)
    q_dev, xm_dev = inp["q"].to(DEV), inp["x_mean"].to(DEV)
    x, mean, scale = _split_views(mat, C)
    assert n == 1 or x.stride(0) != C
    c.l_eager = ER.likelihood(x, mean, scale, q_dev, xm_dev).cpu().to(F64)
    c.l_kernel = E.gaussian_likelihood(x, mean, scale, q_dev, xm_dev).cpu().to(F64)
    c.bits_kernel = E.gaussian_bits(x, mean, scale, q_dev, xm_dev).cpu()
    c.bits64 = ER.gaussian_bits(i64["x"], i64["mean"], i64["scale"], i64["q"], i64["x_mean"])
    c.grads = {}
    for which, g in (("all", inp["g"]), ("well", inp["g"] * c.well.to(torch.float32))):
        leaves = {k: i64[k].clone().requires_grad_(True) for k in ("x", "mean", "scale", "q")}
        ER.gaussian_bits(leaves["x"], leaves["mean"], leaves["scale"], leaves["q"], i64["x_mean"]).backward(g.to(F64))
        ref = {k: leaves[k].grad for k in leaves}
        out = {}
        for name, fn in (("eager", ER.gaussian_bits), ("kernel", E.gaussian_bits)):
            m = mat.clone().requires_grad_(True)
            qd = q_dev.clone().requires_grad_(True)
            xv, mv, sv = _split_views(m, C)
            fn(xv, mv, sv, qd, xm_dev).backward(g.to(DEV))
            gx, gm, gs = (t.cpu().to(F64) for t in _split_views(m.grad, C))
            assert float(m.grad[:, 3 * C:].abs().sum()) == 0.0
            assert qd.grad.shape == qd.shape
            out[name] = {"x": gx, "mean": gm, "scale": gs, "q": qd.grad.cpu().to(F64)}
        c.grads[which] = SimpleNamespace(ref=ref, eager=out["eager"], kernel=out["kernel"])
    torch.cuda.synchronize()
    return c


@pytest.mark.parametrize("q_kind", Q_KINDS)
@pytest.mark.parametrize("C", CS)
def test_likelihood_is_no_further_from_float64_than_eager_fp32(C, q_kind):
    """E = |l - l64| / 2^-24 over the elements of n = 1, 3 and 257 together: max and mean of the kernel no larger than those
    of the fp32 eager formula, without a margin.  The bits follow from l by one log2."""
    cases = [_case(n, C, q_kind) for n in NS]
    e_kernel = torch.cat([((c.l_kernel - c.l64).abs() / UNIT).reshape(-1) for c in cases])
    e_eager = torch.cat([((c.l_eager - c.l64).abs() / UNIT).reshape(-1) for c in cases])
    print(f"\nlikelihood error in units of 2^-24, C={C} q={q_kind}: kernel max {float(e_kernel.max()):.3f} mean "
          f"{float(e_kernel.mean()):.4f}; eager fp32 max {float(e_eager.max()):.3f} mean {float(e_eager.mean()):.4f}")
    assert float(e_kernel.max()) <= float(e_eager.max())
    assert float(e_kernel.mean()) <= float(e_eager.mean())
    for c in cases:
        assert c.bits_kernel.shape == (c.n, C) and c.bits_kernel.dtype == torch.float32
        # bits = -log2(max(l, 1e-6)) of the kernel's own l, rounded once (the device log2 is within 2 units in the last place)
        own = -torch.log2(torch.clamp(c.l_kernel, min=ER.FLOOR))
        assert float((c.bits_kernel.to(F64) - own).abs().max()) <= 3 * 2.0 ** -23 * 20
        assert float(c.bits_kernel.min()) >= 0.0 and float(c.bits_kernel.max()) <= 19.94


@pytest.mark.parametrize("q_kind", Q_KINDS)
@pytest.mark.parametrize("C", CS)
def test_gradients_are_no_further_from_float64_than_eager_fp32(C, q_kind):
    """helpers.max_err_over_scale per tensor against float64 autograd of the restatement, over n = 1, 3, 257 together: the
    kernel's no larger than fp32 eager autograd's -- once for the upstream g over everything outside the band around the
    floor (for a per-row q: rows without a band element; a single q only where no element is in the band), once with g
    restricted to l64 >= 1e-3.  Outside the band the gate agrees with float64."""
    cases = [_case(n, C, q_kind) for n in NS]
    band_share = sum(int(c.band.sum()) for c in cases) / sum(c.n * C for c in cases)
    print(f"\nC={C} q={q_kind}: {100 * band_share:.3f} % of the elements within {BAND} of the floor")
    assert band_share <= 0.01
    for c in cases:
        out = ~c.band
        assert torch.equal((c.l_kernel >= ER.FLOOR)[out], (c.l64 >= ER.FLOOR)[out])
        closed = out & (c.l64 < ER.FLOOR)
        for k in ("x", "mean", "scale"):
            assert (c.grads["all"].kernel[k][closed] == 0).all()
    for which in ("all", "well"):
        for k in ("x", "mean", "scale", "q"):
            ref, eager, kernel = [], [], []
            for c in cases:
                gr = c.grads[which]
                if which == "well":
                    keep = torch.ones_like(gr.ref[k], dtype=torch.bool)
                elif k != "q" or q_kind == "element":
                    keep = ~c.band
                elif q_kind == "row":
                    keep = ~c.band.any(dim=1, keepdim=True)
                else:
                    keep = ~c.band.any().reshape(gr.ref[k].shape)
                assert gr.kernel[k].shape == gr.ref[k].shape
                ref.append(gr.ref[k][keep]); eager.append(gr.eager[k][keep]); kernel.append(gr.kernel[k][keep])
            ref, eager, kernel = torch.cat(ref), torch.cat(eager), torch.cat(kernel)
            if ref.numel() == 0:
                continue
            assert torch.isfinite(kernel).all()
            err_k, err_e = Hh.max_err_over_scale(kernel.numpy(), ref.numpy()), Hh.max_err_over_scale(eager.numpy(), ref.numpy())
            print(f"gradient error over scale, C={C} q={q_kind} {which:4s} d{k:5s}: kernel {err_k:.3e}  eager fp32 {err_e:.3e}")
            assert err_k <= err_e, (which, k, err_k, err_e)


def _fused_inputs(n, C, r, q_kind, seed, rows):
    inp = ER.make_inputs(n, C, seed=seed, q_kind=q_kind)
    gen = torch.Generator().manual_seed(seed + 1)
    weight = None
    if r > 1 or seed % 2:
        weight = (torch.rand(n, C // r, generator=gen) < 0.7).float() * (0.5 + torch.rand(n, C // r, generator=gen))
    if rows == "random":
        rows_t = torch.rand(n, generator=gen) <= 0.05
    else:
        rows_t = {"none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool),
                  "last": torch.arange(n) == n - 1}[rows]
    return inp, weight, rows_t


@pytest.mark.parametrize("n,C,r,q_kind,rows", [
    (257, 30, 3, "row", "random"), (257, 30, 3, "single", "all"), (257, 30, 3, "element", "last"),
    (257, 30, 3, "row", "none"), (257, 50, 1, "row", "random"), (257, 6, 1, "row", "all"), (257, 67, 1, "single", "last"),
    (3, 30, 3, "row", "last"), (1, 1, 1, "single", "all"), (3, 50, 1, "element", "none"),
    (4096 * 4 + 5, 50, 1, "row", "random"),      # more row tiles than workgroups: the grid-stride path
])
def test_rate_sum_equals_bits_of_the_gathered_rows_summed_in_float64(n, C, r, q_kind, rows):
    """rate_sum with a row mask against gaussian_bits on the gathered rows, times the gathered weight, summed in float64.
    The header's bound: the total is the fp32 rounding of an fp64 sum of the same fp32 terms,
    |total - sum| <= 2^-24 |sum| + N 2^-53 T.  count is exact.  The gradients of the chosen rows are the same kernel
    arithmetic with the same upstream, so x, mean, scale and a per-element q agree bit for bit; the row sum of a per-row q
    is taken in fp64 in another lane order and the three-term weight sums in another order: one rounding each.  Rows not
    chosen get exact zeros."""
    E = _E()
    inp, weight, rows_t = _fused_inputs(n, C, r, q_kind, seed=n + C + r, rows=rows)
    mat = _device_matrix(inp, n, C).requires_grad_(True)
    q = inp["q"].to(DEV).requires_grad_(True)
    xm = inp["x_mean"].to(DEV)
    w = None if weight is None else weight.to(DEV).requires_grad_(True)
    rows_d = rows_t.to(DEV)
    x, mean, scale = _split_views(mat, C)
    total, count = E.rate_sum(x, mean, scale, q, xm, rows=rows_d, weight=w, weight_repeat=r)
    assert total.shape == () and total.dtype == torch.float32 and count.shape == () and count.dtype == torch.int64
    assert count.device.type == "cuda" and not count.requires_grad
    m = int(rows_t.sum())
    assert int(count) == m * C
    total.backward()
    # the gathered form
    mat2 = mat.detach().clone().requires_grad_(True)
    q2 = q.detach().clone().requires_grad_(True)
    w2 = None if w is None else w.detach().clone().requires_grad_(True)
    x2, mean2, scale2 = _split_views(mat2, C)
    qg = q2 if q_kind == "single" else q2[rows_d]
    bits = E.gaussian_bits(x2[rows_d], mean2[rows_d], scale2[rows_d], qg, xm)
    terms = bits if w2 is None else bits * ER.expand_weight(w2[rows_d], r)
    ref = terms.double().sum()
    ref.backward()
    T = float(terms.detach().abs().double().sum())
    got, want = float(total.detach()), float(ref.detach())
    assert abs(got - want) <= UNIT * abs(want) + terms.numel() * 2.0 ** -53 * T
    if m == 0:
        assert got == 0.0
    unchosen = ~rows_d
    for got, want in zip(_split_views(mat.grad, C), _split_views(mat2.grad, C)):
        assert torch.equal(got[rows_d], want[rows_d])
        assert (got[unchosen] == 0).all()
    assert float(mat.grad[:, 3 * C:].abs().sum()) == 0.0
    assert q.grad.shape == q.shape
    if q_kind == "element":
        assert torch.equal(q.grad, q2.grad)
    else:
        scale_q = float(q2.grad.abs().max())
        assert float((q.grad - q2.grad).abs().max()) <= 2.0 ** -23 * scale_q
        if q_kind == "row":
            assert (q.grad[unchosen] == 0).all()
    if w is not None:
        assert w.grad.shape == w.shape and (w.grad[unchosen] == 0).all()
        assert float((w.grad - w2.grad).abs().max()) <= 2 * 2.0 ** -23 * max(float(w2.grad.abs().max()), 1e-30)


def _context_inputs(n, feat_dim, K, seed):
    gen = torch.Generator().manual_seed(seed)

    def randn(*s):
        return torch.randn(s, generator=gen)

    widths = [feat_dim, feat_dim, 6, 6, 3 * K, 3 * K, 1, 1, 1]
    context = randn(n, sum(widths))
    at = np.cumsum([0] + widths)
    for i in (1, 3, 5):                                   # the three scale blocks: positive
        context[:, at[i]:at[i + 1]] = 0.3 * torch.exp(context[:, at[i]:at[i + 1]])
    context[:, at[2]:at[3]] *= 1e-3                        # scaling and offsets live on their own quantisation steps
    context[:, at[3]:at[4]] *= 1e-3
    context[:, at[4]:at[6]] *= 0.2
    context[:, at[6]:] *= 0.5                              # keeps 1 + tanh away from 0, where torch's fp32 tanh (no kernel of ours) decides q
    feat = context[:, :feat_dim] + randn(n, feat_dim) * context[:, at[1]:at[2]]
    grid_scaling = context[:, at[2]:at[3]] + randn(n, 6) * context[:, at[3]:at[4]]
    grid_offsets = (context[:, at[4]:at[5]] + randn(n, 3 * K) * context[:, at[5]:at[6]]).reshape(n, K, 3)
    choose = torch.rand(n, generator=gen) <= 0.2
    choose[-1] = True
    grid_masks = (torch.rand(n, K, 1, generator=gen) < 0.6).float()
    rate = torch.tensor(0.83)
    means = (feat.mean(), grid_scaling.mean(), grid_offsets.mean())
    return [feat.contiguous(), grid_scaling.contiguous(), grid_offsets.contiguous(), context, choose, grid_masks, rate, *means]


def test_context_rates_against_the_restated_renderer_lines_in_float64():
    """The four bit_per_* values of gaussian_renderer/__init__.py:123-127 from context_rates against the restatement with its
    gathers in float64.  Tolerance: a kernel bit count is -log2 of an l that is a few units in ITS last place off (about
    (8 + t^2) 2^-24 / ln 2 < 4e-6 for |t| <= 6) plus one fp32 rounding of a number below 20 (1.2e-6); a mean of such terms is
    no further off, and the three fp32 operations behind the sum add 2e-7 of the value: 1e-5 max(1, |value|)."""
    E = _E()
    n, feat_dim, K = 257, 50, 10
    args = _context_inputs(n, feat_dim, K, seed=3)
    ref = ER.rate_terms(*[a.to(F64) if a.is_floating_point() else a for a in args], feat_dim, K)
    dev = [a.to(DEV) for a in args]
    dev[0].requires_grad_(True)
    dev[3].requires_grad_(True)
    got = E.context_rates(*dev, feat_dim, K)
    assert len(got) == 4
    for name, g, r in zip(("param", "feat", "scaling", "offsets"), got, ref):
        assert g.shape == () and g.dtype == torch.float32
        value = float(g.detach())
        assert abs(value - float(r)) <= 1e-5 * max(1.0, abs(float(r))), (name, value, float(r))
    got[0].backward()
    choose = args[4]
    assert dev[0].grad.shape == dev[0].shape and dev[3].grad.shape == dev[3].shape
    assert (dev[0].grad[~choose.to(DEV)] == 0).all() and (dev[3].grad[~choose.to(DEV)] == 0).all()
    assert float(dev[0].grad[choose.to(DEV)].abs().sum()) > 0 and torch.isfinite(dev[3].grad).all()


@pytest.mark.parametrize("q_kind", ["single", "row"])
def test_two_runs_give_the_same_bits(q_kind):
    E = _E()
    n, C, r = 4096 * 4 + 5, 30, 3
    inp, weight, rows_t = _fused_inputs(n, C, r, q_kind, seed=11, rows="random")
    mat0 = _device_matrix(inp, n, C)
    outs = []
    for _ in range(2):
        mat = mat0.clone().requires_grad_(True)
        q = inp["q"].to(DEV).requires_grad_(True)
        w = weight.to(DEV).requires_grad_(True)
        x, mean, scale = _split_views(mat, C)
        total, count = E.rate_sum(x, mean, scale, q, inp["x_mean"].to(DEV), rows=rows_t.to(DEV), weight=w, weight_repeat=r)
        total.backward()
        bits = E.gaussian_bits(x.detach(), mean.detach(), scale.detach(), q.detach(), None)
        outs.append((total.detach(), count, mat.grad, q.grad, w.grad, bits))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_forward_and_backward_replay_from_a_graph_without_a_host_wait():
    """rate_sum forward and backward captured with torch.cuda.graph after one warm-up call (capture raises on any host
    wait) and replayed on new operand values: bit-equal to the direct call."""
    E = _E()
    n, C, r = 257, 30, 3
    inp, weight, rows_t = _fused_inputs(n, C, r, "row", seed=21, rows="random")
    inp2, weight2, rows2 = _fused_inputs(n, C, r, "row", seed=22, rows="random")
    mat = _device_matrix(inp, n, C).requires_grad_(True)
    q = inp["q"].to(DEV).requires_grad_(True)
    q_one = torch.tensor(0.21, device=DEV, requires_grad=True)
    w = weight.to(DEV).requires_grad_(True)
    rows_d = rows_t.to(DEV)

    def step():
        x, mean, scale = _split_views(mat, C)
        x_mean = x.detach().mean()
        total, count = E.rate_sum(x, mean, scale, q, x_mean, rows=rows_d, weight=w, weight_repeat=r)
        total_one, _ = E.rate_sum(x, mean, scale, q_one, x_mean, rows=rows_d)
        grads = torch.autograd.grad(total + total_one, [mat, q, q_one, w])
        return (total, count, total_one) + tuple(grads)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                           # the warm-up: loads the library
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():                                # new values in the captured tensors
        mat.copy_(_device_matrix(inp2, n, C))
        q.copy_(inp2["q"].to(DEV))
        w.copy_(weight2.to(DEV))
        rows_d.copy_(rows2.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    direct = step()
    torch.cuda.synchronize()
    assert int(replayed[1]) == int(rows2.sum()) * C
    for a, b in zip(replayed, direct):
        assert torch.equal(a, b)


def test_no_rows():
    E = _E()
    C = 6
    empty = torch.zeros(0, C, device=DEV, requires_grad=True)
    q = torch.tensor(0.3, device=DEV, requires_grad=True)
    bits = E.gaussian_bits(empty, empty, empty, q, None)
    assert bits.shape == (0, C)
    total, count = E.rate_sum(empty, empty, empty, q, torch.zeros((), device=DEV), rows=torch.zeros(0, dtype=torch.bool, device=DEV))
    assert float(total.detach()) == 0.0 and int(count) == 0
    total.backward()
    assert empty.grad.shape == (0, C) and float(q.grad) == 0.0
    m = E.EntropyGaussian(Q=0.5)
    assert m(empty.detach(), empty.detach(), empty.detach()).shape == (0, C)


def test_module_is_the_reference_argument_list():
    E = _E()
    c = _case(257, 6, "row")
    mat = _device_matrix(c.inp, 257, 6)
    x, mean, scale = _split_views(mat, 6)
    q, xm = c.inp["q"].to(DEV), c.inp["x_mean"].to(DEV)
    m = E.EntropyGaussian()
    assert torch.equal(m(x, mean, scale, q, xm).cpu(), c.bits_kernel)
    assert torch.equal(m.forward(x, mean, scale, Q=q, x_mean=xm).cpu(), c.bits_kernel)
    # Q = None: the module's own; x_mean = None: x.mean() on the device; a python number and a 0-dim tensor are one q
    a = E.EntropyGaussian(Q=0.5)(x, mean, scale)
    b = E.gaussian_bits(x, mean, scale, torch.tensor(0.5, device=DEV), x.mean())
    assert torch.equal(a, b)
    # operands the kernel cannot read in place are made dense: same bits
    xt = x.t().contiguous().t()
    assert xt.stride(1) != 1 and torch.equal(E.gaussian_bits(xt, mean, scale, q, xm).cpu(), c.bits_kernel)
    # a NaN operand gives NaN bits and a backward that does not fault
    xn = x.clone().requires_grad_(True)
    with torch.no_grad():
        xn[0, 0] = float("nan")
    bits = E.gaussian_bits(xn, mean, scale, q, xm)
    assert torch.isnan(bits[0, 0]) and torch.isfinite(bits[1:]).all()
    bits.sum().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(xn.grad[1:]).all()


def test_errors():
    E = _E()
    t = torch.zeros(4, 6, device=DEV)
    xm = torch.zeros((), device=DEV)
    with pytest.raises(TypeError):
        E.gaussian_bits(t.double(), t, t, 1.0)
    with pytest.raises(TypeError):
        E.gaussian_bits(t, t, t.half(), 1.0)
    with pytest.raises(TypeError):
        E.gaussian_bits(t, t, t, torch.ones(4, 1, device=DEV, dtype=F64))
    with pytest.raises(TypeError):
        E.gaussian_bits(t, t, t, "1")
    with pytest.raises(TypeError):
        E.rate_sum(t, t, t, 1.0, xm, rows=torch.zeros(4, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        E.gaussian_bits(t.cpu(), t, t, 1.0)
    with pytest.raises(ValueError):
        E.rate_sum(t, t, t, 1.0, xm, rows=torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError):
        E.gaussian_bits(t, t[:, :5], t, 1.0)
    with pytest.raises(ValueError):
        E.gaussian_bits(t[0], t[0], t[0], 1.0)
    with pytest.raises(ValueError):
        E.gaussian_bits(t, t, t, torch.ones(3, 1, device=DEV))
    with pytest.raises(ValueError):
        E.gaussian_bits(t, t, t, 1.0, x_mean=torch.zeros(2, device=DEV))
    with pytest.raises(ValueError):
        E.rate_sum(t, t, t, 1.0, xm, rows=torch.zeros(5, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        E.rate_sum(t, t, t, 1.0, xm, weight=torch.ones(4, 2, device=DEV), weight_repeat=4)
    with pytest.raises(ValueError):
        E.rate_sum(t, t, t, 1.0, xm, weight=torch.ones(4, 3, device=DEV), weight_repeat=3)
    with pytest.raises(ValueError):
        E.rate_sum(t, t, t, 1.0, xm, weight_repeat=3)
    with pytest.raises(ValueError):
        E.context_rates(t, t, t, t, None, None, 1.0, xm, xm, xm, 50, 10)


# ---------------------------------------------------------------- the sweep over the kernel's own regimes
SWEEP_SEED = 7          # (the seed of the table in test_entropy_cpu.py)
FLOOR_BITS = -np.log2(1e-6)
GRADS = ("x", "mean", "scale", "q")


def _bits_of(t):
    return t.contiguous().view(torch.int32)


def _sweep_run(sub, q, g, xm):
    """likelihood, bits and the backward for the dense upstream g on the rows of ``sub`` with q as given (0-dim, [n, 1] or
    [n, C]) -> dict l, bits, x, mean, scale, q on the CPU"""
    E = _E()
    n, C = sub["x"].shape
    mat = _device_matrix(sub, n, C).requires_grad_(True)
    qd = q.to(DEV).clone().requires_grad_(True)
    x, mean, scale = _split_views(mat, C)
    out = {"l": E.gaussian_likelihood(x.detach(), mean.detach(), scale.detach(), qd.detach(), xm).cpu()}
    bits = E.gaussian_bits(x, mean, scale, qd, xm)
    bits.backward(g.to(DEV))
    out["bits"] = bits.detach().cpu()
    out["x"], out["mean"], out["scale"] = (t.cpu() for t in _split_views(mat.grad, C))
    assert float(mat.grad[:, 3 * C:].abs().sum()) == 0.0 and qd.grad.shape == qd.shape
    out["q"] = qd.grad.cpu()
    return out


@functools.lru_cache(maxsize=None)
def _sweep():
    """ER.make_regime_inputs once: float64, the fp32 CPU yardstick, and the kernels with q per element, per row and -- on
    the rows that share a value -- as one number; rate_sum over all rows."""
    inp = ER.make_regime_inputs(SWEEP_SEED)
    n, C = inp["x"].shape
    c = SimpleNamespace(inp=inp, n=n, C=C, ref=ER.regime_reference(inp))
    c.yard = ER.regime_yardstick(inp, c.ref)
    c.band = (c.ref["l"] / ER.FLOOR - 1).abs() <= BAND
    xm = inp["x_mean"].to(DEV)
    c.element = _sweep_run(inp, inp["q"].expand(n, C).contiguous(), inp["g"], xm)
    c.row = _sweep_run(inp, inp["q"], inp["g"], xm)
    c.single = {k: torch.empty(n, C) for k in ("l", "bits", "x", "mean", "scale")}
    c.single["q"] = torch.empty(n)
    values = inp["q"][:, 0]
    c.groups = [torch.nonzero(values == v)[:, 0] for v in torch.unique(values)]
    for rows in c.groups:
        out = _sweep_run({k: inp[k][rows] for k in ("x", "mean", "scale")}, values[rows[0]].reshape(()), inp["g"][rows], xm)
        for k in c.single:
            c.single[k][rows] = out[k]
    mat = _device_matrix(inp, n, C)
    x, mean, scale = _split_views(mat, C)
    total, count = _E().rate_sum(x, mean, scale, inp["q"].to(DEV), xm)
    c.total, c.count = float(total), int(count)
    torch.cuda.synchronize()
    return c


def test_sweep_is_finite_wherever_float64_is():
    """l, bits, the four gradients (q per element, per row, one number) and rate_sum's total: the float64 restatement is
    finite on the whole sweep (test_entropy_cpu.py), so everything the kernels return is.  Before the guard of
    cdf_difference this failed on the narrow bins with |m| above about 6.6e4, d = 0 among them: 0 * inf in the series."""
    c = _sweep()
    narrow_far = (c.ref["real"]["d"].abs() <= ER.NARROW) & (c.ref["real"]["m"].abs() > 6.5e4)
    assert int(narrow_far.sum()) >= 500
    for mode in ("element", "row", "single"):
        out = getattr(c, mode)
        for k, v in out.items():
            bad = ~torch.isfinite(v)
            assert not bad.any(), (mode, k, int(bad.sum()), int((bad & narrow_far).sum()) if bad.shape == narrow_far.shape else None)
    assert np.isfinite(c.total) and c.count == c.n * c.C


def test_sweep_modes_of_q_are_one_arithmetic():
    """q per row and q as one number give the bits of q per element: l, bits and the gradients of x, mean, scale bit for
    bit, the gradient of q as the fp64 sum of the per-element ones rounded once."""
    c = _sweep()
    assert len(c.groups) >= 40 and max(len(g) for g in c.groups) >= 4
    for mode in ("row", "single"):
        out = getattr(c, mode)
        for k in ("l", "bits", "x", "mean", "scale"):
            assert torch.equal(out[k], c.element[k]), (mode, k)
    dq = c.element["q"].double()

    def rounded_once(got, want, mag, terms):
        return abs(float(got) - float(want)) <= 2.0 ** -24 * abs(float(want)) + 2.0 ** -149 + terms * 2.0 ** -53 * float(mag)

    for i in range(c.n):
        assert rounded_once(c.row["q"][i, 0], dq[i].sum(), dq[i].abs().sum(), c.C), i
    for rows in c.groups:
        got = c.single["q"][rows]
        assert (got == got[0]).all()
        assert rounded_once(got[0], dq[rows].sum(), dq[rows].abs().sum(), len(rows) * c.C)


def test_sweep_below_the_floor():
    """l64 < 1e-6 outside the band: one bit pattern for the bits, within a unit of -log2(1e-6); no gradient at all; and
    the kernel's own l, which nothing downstream reads there, no more than twice the float64 value (taken from the tail:
    test_entropy_cpu.py) plus the smallest fp32 number."""
    c = _sweep()
    closed = ~c.band & (c.ref["l"] < ER.FLOOR)
    assert int(closed.sum()) >= 5000
    bits = c.element["bits"][closed]
    assert (_bits_of(bits) == _bits_of(bits)[0]).all()
    assert abs(float(bits[0]) - FLOOR_BITS) <= float(np.spacing(np.float32(FLOOR_BITS)))
    for k in GRADS:
        assert (c.element[k][closed] == 0).all(), k
    over = c.element["l"].double()[closed] - (2 * c.ref["l_tail"][closed] + 2.0 ** -149)
    assert float(over.max()) <= 0, float(over.max())


def test_sweep_above_the_floor_per_region():
    """l64 >= 1e-6 outside the band, per region (narrow | wide bin) x (|m| in [0, 1), [1, 4), [4, 6), >= 6) of the REALISED
    (m, d): the kernel's maximum error of l in units in the last place of l, and of each gradient in units of 2^-24 of the
    yardstick's scale, is at most max(2 x the fp32 CPU figure of that region, 16) -- ER.regime_bar.  The 16 is the accuracy
    OpenCL specifies for erf and erfc, to which the device library is written; the factor 2 is for the device exp and erfc
    rounding differently from libm's.  The CPU figures and the mutants that this bar catches: test_entropy_cpu.py.
    The kernel's figures are printed beside the yardstick and the bar.  Measured on an MI355X with seed 7, kernel /
    yardstick (the bar is max(2 x yardstick, 16) and is not tightened to these):

    region                   l              dx = -dmean     dscale          dq
    narrow |m| in [0,1)    2.54 /  2.54    5.31 /  5.31    3.89 /  3.82    3.84 /  4.95
    narrow |m| in [1,4)   11.01 / 11.01   16.11 / 16.11   10.16 / 10.16   13.69 / 13.69
    narrow |m| in [4,6)   31.87 / 31.87   50.55 / 50.55   31.19 / 31.19   45.49 / 45.49
    wide   |m| in [0,1)    3.65 /  3.56   14.66 / 14.66   14.74 / 14.74   17.64 / 17.64
    wide   |m| in [1,4)   13.20 / 13.20   13.57 / 13.57   12.56 / 11.88   16.59 / 12.76
    wide   |m| in [4,6)   51.45 / 51.45   28.33 / 28.33   70.80 / 70.80   31.20 / 31.20
    wide   |m| >= 6       24.63 / 25.63   24.09 / 24.09   21.91 / 23.05   24.09 / 24.09

    The kernel is at the yardstick nearly everywhere: what there is of error is the header's arithmetic in fp32."""
    c = _sweep()
    keep = ~c.band & (c.ref["l"] >= ER.FLOOR)
    assert torch.equal((c.element["l"] >= ER.FLOOR)[~c.band], (c.ref["l"] >= ER.FLOOR)[~c.band])
    got = ER.regime_errors({k: c.element[k].double() for k in ("l",) + GRADS}, c.ref, keep)
    print("\nkernel / fp32 CPU yardstick / bar, per region (l: units in the last place; gradients: units of 2^-24)")
    failures = []
    for k, (width, edge) in enumerate(ER.REGIONS):
        cells = []
        for name in ("l",) + GRADS:
            if c.yard[name][k] is None:
                assert got[name][k] is None
                continue
            bar = ER.regime_bar(c.yard[name][k])
            cells.append(f"{name} {got[name][k]:.2f} / {c.yard[name][k]:.2f} / {bar:.1f}")
            if not got[name][k] <= bar:
                failures.append((width, edge, name, got[name][k], bar))
        print(f"{width:6s} |m| from {ER.M_EDGES[edge]:3.0f}: " + "   ".join(cells))
    assert not failures, failures


def test_sweep_is_continuous_across_the_threshold_of_the_series():
    """|d| = 0.25 and its two fp32 neighbours AS THE KERNEL FORMS d (ER.kernel_d): the series on one side, the erf / erfc
    forms on the other, and l off float64 by no more than the bar of its region on either."""
    c = _sweep()
    kd = np.abs(ER.kernel_d(c.inp["q"].numpy(), c.inp["scale"].numpy()[:, :1]))
    keep = ~c.band & (c.ref["l"] >= ER.FLOOR)
    ulp = torch.from_numpy(np.spacing(c.ref["l"].numpy().astype(np.float32)).astype(np.float64))
    err = (c.element["l"].double() - c.ref["l"]).abs() / ulp
    bar = torch.tensor([ER.regime_bar(f) if f is not None else 0.0 for f in c.yard["l"]], dtype=F64)[c.ref["real"]["region"]]
    for target in ER.REGIME_D[5:8]:
        rows = torch.from_numpy(kd[:, 0] == np.float32(target))
        sel = keep & rows[:, None]
        assert int(sel.sum()) >= 50, target
        print(f"kernel d = {target!r}: {int(sel.sum())} elements, max error {float(err[sel].max()):.2f} units of l, "
              f"max error / bar {float((err / bar)[sel].max()):.3f}")
        assert (err[sel] <= bar[sel]).all(), target


def test_sweep_total_is_the_float64_sum_of_the_kernels_own_bits():
    """rate_sum over every row of the sweep against the fp64 sum of gaussian_bits: the header's bound."""
    c = _sweep()
    terms = c.row["bits"].double()
    want, T = float(terms.sum()), float(terms.abs().sum())
    assert abs(c.total - want) <= UNIT * abs(want) + terms.numel() * 2.0 ** -53 * T


def test_operands_that_overflow_the_arguments_of_phi_close_the_gradient():
    """The operand-domain rule of the header: tu or tl may overflow (a finite mean of 1e30 over a scale at its floor);
    where l is under the floor -- always, when both overflow to one side -- the bits are -log2(1e-6) and every gradient is
    exactly 0, as the reference's autograd gives, not inf * 0."""
    E = _E()
    mean = torch.tensor([[1e30, -1e30, 3e38, 1e30, 1e25, -1e30]])
    scale = torch.tensor([[1e-9, 0.0, 1e-9, 5e-10, 1e-9, 1e-3]])
    x = torch.tensor([[0.0, 1.0, -2.0, 0.5, 0.0, 3.0]])
    for q in (torch.tensor(0.25), torch.tensor(0.0), torch.full((1, 1), 1e-3), torch.full((1, 6), -0.5)):
        leaves = [t.to(DEV).requires_grad_(True) for t in (x, mean, scale, q)]
        xm = torch.zeros((), device=DEV)
        assert (E.gaussian_likelihood(*[t.detach() for t in leaves], xm) == 0).all()
        bits = E.gaussian_bits(*leaves, xm)
        assert float((bits.detach().cpu().double() - FLOOR_BITS).abs().max()) <= float(np.spacing(np.float32(FLOOR_BITS)))
        bits.backward(torch.ones_like(bits))
        for t in leaves:
            assert t.grad.shape == t.shape and (t.grad == 0).all()
