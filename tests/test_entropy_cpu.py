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


# ---------------------------------------------------------------- the sweep over the kernel's regimes (ER.make_regime_inputs)
SWEEP_SEED = 7
_sweep_cache = {}


def _sweep():
    if not _sweep_cache:
        inp = ER.make_regime_inputs(SWEEP_SEED)
        _sweep_cache.update(inp=inp, ref=ER.regime_reference(inp))
    return _sweep_cache["inp"], _sweep_cache["ref"]


def _unguarded_series_fp32(m, d):
    """the narrow-bin lines of csrc/entropy.hip as they were before the guard, in numpy fp32"""
    with np.errstate(all="ignore"):
        m, d = np.float32(m), np.float32(d)
        u, d2 = m * m, d * d
        he2 = u - np.float32(1)
        he4 = (u - np.float32(6)) * u + np.float32(3)
        he6 = ((u - np.float32(15)) * u + np.float32(45)) * u - np.float32(15)
        he8 = (((u - np.float32(28)) * u + np.float32(210)) * u - np.float32(420)) * u + np.float32(105)
        s = np.float32(1) + d2 * (he2 * np.float32(1 / 6) + d2 * (he4 * np.float32(1 / 120) + d2 * (
            he6 * np.float32(1 / 5040) + d2 * (he8 * np.float32(1 / 362880)))))
        return (np.float32(2) * d) * (np.exp(np.float32(-0.5) * u) * np.float32(0.3989422804014327)) * s


def test_regime_sweep_enters_every_branch_and_stays_out_of_the_band():
    """What the GPU sweep relies on, so that it cannot pass vacuously: shape (several workgroups of 8 rows, a ragged
    last one), every (narrow | wide) x |m| region populated on both sides of the floor where the function has elements
    there at all (a narrow bin with |m| >= 6 is under the floor by 2 d phi(6) < 4e-9, a wide one with |m| < 4 above it), the three kernel_d values around
    the threshold, straddling bins, q < 0, q = 0, all floored scales, the elements whose series was a NaN before the
    guard -- and at most 5 % of the elements within 25 % of the floor, where the gate may fall either way in fp32."""
    inp, ref = _sweep()
    n, C = inp["x"].shape
    assert C == ER.REGIME_C == 30 and n % 8 != 0 and n // 8 >= 32 and inp["q"].shape == (n, 1)
    assert float(inp["x"].abs().max()) <= 1e6 and float(inp["mean"].abs().max()) <= 1e6 and float(inp["x_mean"]) == 0
    for k in ("l", "l_tail", "x", "mean", "scale", "q"):
        assert torch.isfinite(ref[k]).all(), k
    real, l = ref["real"], ref["l"]
    band = (l / ER.FLOOR - 1).abs() <= 0.25
    print(f"\n{n} x {C}: {100 * float(band.double().mean()):.2f} % in the band, {100 * float((l >= ER.FLOOR).double().mean()):.1f} % "
          f"at or above the floor")
    assert float(band.double().mean()) <= 0.05
    for k, (width, edge) in enumerate(ER.REGIONS):
        sel = (real["region"] == k) & ~band
        above, below = int((sel & (l >= ER.FLOOR)).sum()), int((sel & (l < ER.FLOOR)).sum())
        print(f"{width:6s} |m| in [{ER.M_EDGES[edge]}, {ER.M_EDGES[edge + 1]}): {above} above, {below} below the floor")
        assert below >= 100 or (width == "wide" and edge < 2)      # (a wide bin with |m| < 4 holds more than 2e-5)
        assert above >= 100 or (width, edge) == ("narrow", 3)
    kd = ER.kernel_d(inp["q"].numpy(), inp["scale"].numpy()[:, :1])[:, 0]
    for target in ER.REGIME_D[5:8]:
        assert (np.abs(kd) == np.float32(target)).sum() >= 6, target
    assert int((real["m"].abs() < real["d"].abs()).sum()) >= 300            # the bin straddles the mean
    assert 10 <= int((inp["q"] < 0).sum()) <= 30 and int((inp["q"] == 0).sum()) >= 20
    for floored in (0.0, -1.0, 5e-10):
        assert int((inp["scale"] == floored).sum()) >= 30 * 50
    # the finding: the series without its guard is a NaN exactly where the bin is narrow and |m| is past ~6.6e4
    m32, d32 = (inp["x"] * 0 + real["m"]).numpy().astype(np.float32), (inp["x"] * 0 + real["d"]).numpy().astype(np.float32)
    narrow = np.abs(d32) <= np.float32(ER.NARROW)
    nan = np.isnan(_unguarded_series_fp32(m32, d32)) & narrow
    assert nan.sum() >= 500 and (np.abs(m32[nan]) > 6.5e4).all() and (nan[narrow & (np.abs(m32) > 7e4 - 1)]).all()
    assert (nan & (d32 == 0)).any() and (l.numpy()[nan] < 1e-300).all()
    for m, d, want_nan in ((6e4, 0.1, False), (7e4, 0.1, True), (7e4, 0.0, True), (1e5, 1e-3, True), (1e9, 0.2, True)):
        assert bool(np.isnan(_unguarded_series_fp32(m, d))) == want_nan
    guarded = ER.header_evaluation(inp["x"], inp["mean"], inp["scale"], inp["q"], inp["x_mean"], inp["g"])
    for k, v in guarded.items():
        assert torch.isfinite(v).all(), k
    assert (guarded["l"].numpy()[nan] == 0).all()


def test_float64_likelihood_from_the_tail_is_the_restatement_where_that_has_digits():
    """ER.likelihood in float64 is a difference of two numbers up to 1: right to 2^-52 absolute, so worth nothing as a
    reference for an l below that.  The below-the-floor bound of the GPU sweep (l_kernel <= 2 l64 + 2^-149) therefore
    takes l64 from the same three forms the header uses, in float64; here the two agree to that absolute error."""
    inp, ref = _sweep()
    assert float((ref["l_tail"] - ref["l"]).abs().max()) <= 2.0 ** -52
    tiny = ref["l_tail"] < 2.0 ** -60
    assert int(tiny.sum()) > 1000 and int((tiny & (ref["l_tail"] > 0)).sum()) > 100


YARDSTICK = """
region                 l      dx   dmean  dscale      dq
narrow |m| in [0,1)   2.54    5.31    5.31    3.82    3.75
narrow |m| in [1,4)  11.01   16.11   16.11   10.16   13.69
narrow |m| in [4,6)  31.87   50.55   50.55   31.19   45.49
wide   |m| in [0,1)   3.56   14.66   14.66   14.74   17.64
wide   |m| in [1,4)  13.20   13.57   13.57   11.88   12.76
wide   |m| in [4,6)  51.45   28.33   28.33   70.80   31.20
wide   |m| >= 6      25.63   24.09   24.09   23.05   24.09
"""


def _print_table(title, table):
    print(f"\n{title}")
    for k, (width, edge) in enumerate(ER.REGIONS):
        cells = ["      -" if table[name][k] is None else f"{table[name][k]:7.2f}" for name in ("l", "x", "mean", "scale", "q")]
        print(f"{width:6s} |m| from {ER.M_EDGES[edge]:3.0f}: " + " ".join(cells))


def test_header_arithmetic_in_fp32_against_float64_per_region():
    """The yardstick of the GPU sweep (test_entropy_gpu.py): the header's own arithmetic in fp32 with libm on the CPU
    against float64, maximum per region over the elements at or above the floor and outside the band; l in units in the
    last place of l, the gradients in units of 2^-24 of their own magnitude (of |gl| (|tu| du + |tl| dl) for scale).
    Measured with seed 7 (x86-64 glibc; the GPU test recomputes it where it runs):
""" + YARDSTICK + """
    "A few units in the last place" holds for |m| < 1 only.  Further out the roundings of c = xc - mean, of the two
    divisions by s and of m m are multiplied by t^2 (d ln phi(t) / d ln t), 20 to 36 at |m| in [4, 6): that is the
    arithmetic of the header, not the device library, and what the bar of the GPU test is built from.  Here: every figure
    stays under the first-order bound of that arithmetic, so a change of the evaluation that loses digits shows.  The
    bound: exp(-t t / 2) moves by t^2 times the relative error of t -- one unit of 2^-24 each from c and from the division
    by s -- and by t^2 / 2 for the rounding of t t, 2.5 t^2 in all; wherever a bin with |m| < 6 is above the floor the
    side that carries the result has |t| <= |m| + d <= 6.5 (d = 0.5 at |m| = 5.2 is the widest such bin of the lattice
    whose far side still counts), so 2.5 x 6.5^2 = 106, plus the 16 units of erf / erfc / exp themselves: 122."""
    inp, ref = _sweep()
    table = ER.regime_yardstick(inp, ref)
    _print_table("fp32 on the CPU against float64 (l: units in the last place; gradients: units of 2^-24)", table)
    for name, column in table.items():
        for k, figure in enumerate(column):
            assert (figure is None) == (ER.REGIONS[k] == ("narrow", 3)), (name, k)
            assert figure is None or figure <= 2.5 * 6.5 ** 2 + 16, (name, ER.REGIONS[k], figure)


def test_mutants_of_the_header_arithmetic_exceed_the_bar_of_the_gpu_sweep():
    """Without this the bar of the GPU sweep proves nothing: each mutant of ER.header_evaluation must be over
    regime_bar(yardstick) in at least one (quantity, region).  Series coefficients times 10 (the last times 100: its
    term is d^8 He_8(m) / 9! <= 6e-7 of the sum wherever l is above the floor, so times 10 stays inside the bar; that
    coefficient is pinned to a factor of about 30, no better); the threshold moved DOWN to 0.01 (erf differences that
    cancel); the a >= 0 and the b <= 0 branch taking the erf form; exp(x) - 1 for expm1(x).
    The threshold moved UP to 0.5 adds the term d^10 He_10(m) / 11!: with d <= 0.3 that stays inside the bar (0.9 of it),
    which is why the lattice has d = 0.5 as well -- there it is 7e-6 of l at |m| = 5.2, about twice the bar."""
    inp, ref = _sweep()
    base = ER.regime_yardstick(inp, ref)
    for mutant in ER.MUTANTS:
        table = ER.regime_yardstick(inp, ref, mutant)
        over = max((table[name][k] / ER.regime_bar(base[name][k]), name, ER.REGIONS[k]) for name in table
                   for k in range(len(ER.REGIONS)) if base[name][k] is not None)
        print(f"{mutant:16s}: {over[0]:12.1f} times the bar at {over[1]} {over[2]}")
        assert over[0] > 1, (mutant, over)
