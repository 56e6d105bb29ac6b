"""The restatement the GPU tests of the rate term compare with (tests/entropy_reference.py), checked on the CPU: its analytic
gradient against torch float64 autograd of the plain formula, its lower-bound gate against the rule of
utils/entropy_models.py:43-50 evaluated word for word, the weight-repeat column mapping, the clamp with lo > hi, the
input generator, and that importing bloomscene_amd.entropy needs no GPU."""
import math

import numpy as np
import pytest
import torch

import entropy_reference as ER

F64 = torch.float64


def _as64(inp, requires_grad=True):
    out = {k: v.to(F64) for k, v in inp.items()}
    if requires_grad:
        for k in ("x", "mean", "scale", "q"):
            out[k].requires_grad_(True)
    return out


@pytest.mark.parametrize("q_kind", ["single", "row", "element"])
def test_analytic_gradient_equals_float64_autograd(q_kind):
    n, C, r = 37, 30, 3
    inp = _as64(ER.make_inputs(n, C, seed=5, q_kind=q_kind))
    weight = torch.rand(n, C // r, dtype=F64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    bits = ER.gaussian_bits(inp["x"], inp["mean"], inp["scale"], inp["q"], inp["x_mean"], weight, r)
    bits.backward(inp["g"])
    with torch.no_grad():
        ana = ER.analytic_gradients(inp["x"], inp["mean"], inp["scale"], inp["q"], inp["x_mean"], inp["g"], weight, r)
    dq = ana["q"] if q_kind == "element" else (ana["q"].sum(dim=1, keepdim=True) if q_kind == "row" else ana["q"].sum())
    for name, got, ref in (("x", ana["x"], inp["x"].grad), ("mean", ana["mean"], inp["mean"].grad),
                           ("scale", ana["scale"], inp["scale"].grad), ("q", dq, inp["q"].grad),
                           ("weight", ana["weight"], weight.grad)):
        assert got.shape == ref.shape, name
        assert torch.isfinite(ref).all(), name
        scale = float(ref.abs().max())
        assert scale > 0, name
        assert float((got - ref).abs().max()) <= 1e-12 * scale, (name, float((got - ref).abs().max()), scale)
    # the special elements of the generator took their branches
    lo, hi = ER.clamp_bounds(inp["q"], inp["x_mean"], F64)
    outside = (inp["x"] < lo) | (inp["x"] > hi)
    assert int(outside.sum()) == 4 and (inp["x"].grad[outside] == 0).all() and (inp["mean"].grad[outside] != 0).any()
    small = inp["scale"] < ER.SCALE_FLOOR
    assert int(small.sum()) == 4 and (inp["scale"].grad[small] == 0).all()


def test_lower_bound_gate_is_the_rule_as_written():
    rng = np.random.default_rng(0)
    l = np.concatenate([10.0 ** rng.uniform(-9, 0, 500), [0.0, 1e-6, np.nextafter(1e-6, 0), np.nextafter(1e-6, 1)]])
    g = np.concatenate([rng.standard_normal(500), [1.0, -1.0, -2.0, 3.0]])
    lt = torch.tensor(l, dtype=F64, requires_grad=True)
    ER.LowerBound.apply(lt).backward(torch.tensor(g, dtype=F64))
    assert np.array_equal(lt.grad.numpy(), ER.gate_literal(l, g))
    assert (lt.grad.numpy()[l < 1e-6] == 0).all() and np.array_equal(lt.grad.numpy()[l >= 1e-6], g[l >= 1e-6])
    assert torch.equal(ER.LowerBound.apply(lt).detach(), torch.clamp(lt.detach(), min=1e-6))


def test_weight_repeat_maps_column_j_to_entry_j_over_r():
    n, K = 5, 10
    masks = torch.arange(n * K, dtype=F64).reshape(n, K, 1)
    repeated = masks.repeat(1, 1, 3).view(-1, 3 * K)            # gaussian_renderer/__init__.py:114
    expanded = ER.expand_weight(masks.reshape(n, K), 3)
    assert torch.equal(expanded, repeated)
    j = torch.arange(3 * K)
    assert torch.equal(expanded, masks.reshape(n, K)[:, j // 3])


def test_clamp_with_crossed_bounds_gives_the_upper_bound():
    # q < 0 crosses the bounds: torch.clamp(x, lo, hi) with lo > hi is hi for every x, and no x is "inside"
    x = torch.tensor([[-5.0, 0.0, 7.0]], dtype=F64, requires_grad=True)
    q = torch.tensor(-1e-4, dtype=F64)
    x_mean = torch.tensor(0.25, dtype=F64)
    lo, hi = ER.clamp_bounds(q, x_mean, F64)
    assert float(lo) > float(hi)
    mean = torch.full((1, 3), float(hi) + 1e-5, dtype=F64)
    scale = torch.full((1, 3), 1e-4, dtype=F64)
    bits = ER.gaussian_bits(x, mean, scale, q, x_mean)
    clamped = torch.clamp(x.detach(), min=lo, max=hi)
    assert torch.equal(clamped, hi.expand(1, 3))
    assert torch.equal(bits, ER.gaussian_bits(hi.expand(1, 3), mean, scale, q, x_mean))
    bits.sum().backward()
    assert (x.grad == 0).all()
    ana = ER.analytic_gradients(x.detach(), mean, scale, q, x_mean, torch.ones(1, 3, dtype=F64))
    assert (ana["x"] == 0).all() and (ana["mean"] != 0).all()
    # upper < lower here: the likelihood is the absolute value and the sign goes into the gradient
    upper, lower, _, _ = ER.upper_lower(x.detach(), mean, scale, q, x_mean)
    assert (upper < lower).all()


def test_bounds_are_the_fp32_product_then_sum():
    q = torch.tensor([[0.3337], [1e-6], [0.5]], dtype=torch.float32)
    x_mean = torch.tensor(0.0123, dtype=torch.float32)
    lo, hi = ER.clamp_bounds(q.to(F64), x_mean.to(F64), F64)
    assert torch.equal(lo, (x_mean - 15_000 * q).to(F64)) and torch.equal(hi, (x_mean + 15_000 * q).to(F64))


@pytest.mark.parametrize("n,C", [(257, 50), (257, 67), (257, 30)])
def test_generator_puts_the_stated_shares_at_the_floor_and_in_the_band(n, C):
    inp = _as64(ER.make_inputs(n, C, seed=n + C, q_kind="row"), requires_grad=False)
    l = ER.likelihood(inp["x"], inp["mean"], inp["scale"], inp["q"], inp["x_mean"])
    assert torch.isfinite(l).all()
    at_floor = float((l < ER.FLOOR).double().mean())
    band = float(((l / ER.FLOOR - 1).abs() <= 0.25).double().mean())
    assert 0.04 <= at_floor <= 0.12, at_floor
    assert band <= 0.01, band
    lo, hi = ER.clamp_bounds(inp["q"], inp["x_mean"], F64)
    assert int(((inp["x"] < lo) | (inp["x"] > hi)).sum()) == 4 and int((inp["scale"] < ER.SCALE_FLOOR).sum()) == 4


def test_importing_the_module_needs_no_gpu():
    import bloomscene_amd.entropy as E
    assert callable(E.gaussian_bits) and callable(E.rate_sum) and callable(E.context_rates)
    m = E.EntropyGaussian()
    assert m.Q == 1 and E.EntropyGaussian(Q=0.5).Q == 0.5
    # there is no CPU path: dtype errors are TypeError, CPU tensors and shapes ValueError, before any native call
    t = torch.zeros(3, 6)
    with pytest.raises(ValueError, match="GPU"):
        E.gaussian_bits(t, t, t, 1.0)
    with pytest.raises(TypeError, match="float32"):
        E.gaussian_bits(t.double(), t, t, 1.0)
    with pytest.raises(TypeError, match="float32"):
        E.rate_sum(t, t, t.half(), 1.0, torch.zeros(()))
    with pytest.raises(TypeError, match="bool"):
        E.rate_sum(t, t, t, 1.0, torch.zeros(()), rows=torch.zeros(3, dtype=torch.uint8))
    assert math.isclose(E.Q_SINGLE, 0) and E.Q_ROW == 1 and E.Q_ELEMENT == 2
