"""CPU tests of the fused Adam step (include/bloomscene_adam.h, bloomscene_amd/optim.py): the restatement of
tests/adam_reference.py against a float64 Adam and against torch.optim.Adam(foreach=False) on CPU tensors, bpow against
beta ** t, the state dict in both directions, the python interface's checks in their order and the native entry point's
refusals -- all before the device is touched."""
import copy
import math

import numpy as np
import pytest
import torch

import adam_reference as AR
from bloomscene_amd import _capi
from bloomscene_amd.optim import Adam

F32 = np.float32
U = 2.0 ** -24          # the unit roundoff of fp32
STEPS = 5
LR, BETA1, BETA2, EPS = 1e-2, 0.9, 0.999, 1e-8


def _five_step_case(seed=0, n=4099):
    """Gradients whose sizes spread over three decades between elements, so that a bound relative to the tensor's largest
    value would hide the small ones: every bound below is per element."""
    rng = np.random.default_rng(seed)
    size = 10.0 ** rng.uniform(-3, 0, n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    grads = [(sign * size * rng.uniform(0.5, 1.0, n) * (1 if k != 2 else -1)).astype(F32) for k in range(STEPS)]
    return rng.standard_normal(n).astype(F32), grads


def _bounds(grads, p64, lr=LR, steps=STEPS):
    """Per-element bounds on |fp32 formula - float64 Adam| after `steps` steps, from the operation count alone
    (u = 2^-24; G = the element's largest |g| so far; the errors a step inherits are not amplified: both decay factors are < 1):
      m'   4 roundings a step (w1, g - m, the product, the sum), each of a value <= G:           4 t u G
      v'   6 roundings a step (b2, b2 v, g g, w2, the product, the sum), all terms positive, so the error stays
           RELATIVE:                                                                                6 t u v'
      den  half of v's relative error through the square root, + 4 roundings (sqrtf, bc2s, the division, the sum with
           eps; eps itself is rounded too but only adds to a positive sum):                        (3 t + 5) u den
      q = m' / den:  |dq| <= |dm'| / den + |q| (3 t + 5) u + |q| u.  The element's largest gradient alone gives
           v' >= w2 b2^(t-1) G^2 and bc2s^2 = 1 - b2^t <= t w2, so den >= G sqrt(b2^(t-1) / t), and |m'| <= G:
           |dm'| / den <= 4 t u sqrt(t / b2^(t-1)),  |q| <= sqrt(t / b2^(t-1))
      p'   a step adds ss |dq| + 2 u ss |q| (ss rounded, the product rounded) + u |p| (the subtraction), ss = lr / (1 - b1^t).
    Every step is charged with the last step's (largest) factors."""
    t = steps
    G = np.max(np.abs(np.stack(grads).astype(np.float64)), axis=0)
    r = math.sqrt(t / BETA2 ** (t - 1))
    dq = 4 * t * U * r + r * (3 * t + 5) * U + r * U
    ss_sum = sum(lr / (1 - BETA1 ** k) for k in range(1, t + 1))
    bound_p = ss_sum * (dq + 2 * U * r) + t * U * (np.abs(p64) + ss_sum * r)
    return bound_p, 4 * t * U * G, 6 * t * U


def _run_restatement(p0, grads):
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(p0.shape), np.zeros(p0.shape)
    for t, g in enumerate(grads, 1):
        p, m, v = AR.adam_step(p, g, m, v, LR, t, BETA1, BETA2, EPS)
        p64, m64, v64 = AR.adam_step_f64(p64, g, m64, v64, LR, t, BETA1, BETA2, EPS)
    return (p, m, v), (p64, m64, v64)


def test_restatement_is_a_float64_adam_within_the_rounding_of_its_operations():
    p0, grads = _five_step_case()
    (p, m, v), (p64, m64, v64) = _run_restatement(p0, grads)
    bp, bm, bv = _bounds(grads, p64)
    ep, em, ev = np.abs(p - p64), np.abs(m - m64), np.abs(v - v64) / v64
    print(f"restatement vs float64 after {STEPS} steps: p {ep.max():.3e} (largest share of its bound {np.max(ep / bp):.3f}), "
          f"m {em.max():.3e} ({np.max(em / bm):.3f}), v relative {ev.max():.3e} ({ev.max() / bv:.3f})")
    assert (ep <= bp).all() and (em <= bm).all() and (ev <= bv).all()
    # ... and it is Adam at all: a wrong formula is orders of magnitude outside (one step's change is ~lr)
    assert np.abs(p64 - p0).max() > 1000 * bp.max()


def test_restatement_matches_torch_adam_on_cpu_tensors():
    """torch.optim.Adam(foreach=False) on CPU tensors is the same formula with another association in the last line
    ((-ss m') / den) and libm's pow: both sides are within the bound above of the float64 Adam, so within twice it of
    each other."""
    p0, grads = _five_step_case(seed=1)
    (p, m, v), (p64, _, _) = _run_restatement(p0, grads)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=LR, betas=(BETA1, BETA2), eps=EPS, foreach=False)
    for g in grads:
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
    st = opt.state[tp]
    bp, bm, bv = _bounds(grads, p64)
    ep = np.abs(p - tp.detach().numpy())
    em = np.abs(m - st["exp_avg"].numpy())
    ev = np.abs(v - st["exp_avg_sq"].numpy()) / v
    print(f"restatement vs torch CPU after {STEPS} steps: p {ep.max():.3e}, m {em.max():.3e}, v relative {ev.max():.3e}; "
          f"bit-equal elements p {np.mean(ep == 0):.3f} m {np.mean(em == 0):.3f} v {np.mean(ev == 0):.3f}")
    assert (ep <= 2 * bp).all() and (em <= 2 * bm).all() and (ev <= 2 * bv).all()
    assert float(st["step"]) == STEPS


def _ulps_apart(a, b):
    return np.abs(np.asarray(a, F32).view(np.int32).astype(np.int64) - np.asarray(b, F32).view(np.int32).astype(np.int64))


def test_bpow_against_pow_for_every_step_up_to_thirty_thousand():
    """bpow is within (t + 1) fp64 roundings of beta ** t (a squaring doubles the error it inherits), and the two scalars
    formed from it are within one fp32 ulp of torch's expressions at every step; the share of steps that differ at all is
    printed (docs/EXPERIMENTS.md records it), not fixed."""
    T = 30_000
    worst = 0.0
    ss, ss_t, bc, bc_t = (np.empty(T, F32) for _ in range(4))
    for t in range(1, T + 1):
        for b in (BETA1, BETA2):
            exact = b ** t
            got = AR.bpow(b, t)
            if exact > 1e-300:
                worst = max(worst, abs(got - exact) / exact / (2.0 ** -53))
                assert abs(got - exact) <= (t + 1) * 2.0 ** -53 * exact, (b, t)
        ss[t - 1], bc[t - 1] = AR.step_scalars(0.0075, BETA1, BETA2, t)
        ss_t[t - 1] = F32(0.0075 / (1 - BETA1 ** t))          # torch: step_size = lr / bias_correction1
        bc_t[t - 1] = F32((1 - BETA2 ** t) ** 0.5)            # torch: bias_correction2 ** 0.5
    d_ss, d_bc = _ulps_apart(ss, ss_t), _ulps_apart(bc, bc_t)
    print(f"bpow vs beta ** t, t = 1..{T}: at most {worst:.1f} fp64 ulp apart; ss differs from torch's on "
          f"{np.mean(d_ss > 0):.5%} of the steps, bc2s on {np.mean(d_bc > 0):.5%}, never by more than one fp32 ulp")
    assert d_ss.max() <= 1 and d_bc.max() <= 1
    assert AR.bpow(0.5, 0) == 1.0 and AR.bpow(0.5, 1) == 0.5 and AR.bpow(0.5, 10) == 2.0 ** -10 and AR.bpow(0.0, 3) == 0.0


def _groups(params):
    return [{"params": [params[0]], "lr": 0.01, "name": "anchor"}, {"params": [params[1]], "lr": 0.002, "name": "mlp_opacity"}]


def test_state_dict_round_trip_with_torch_adam_in_both_directions():
    torch.manual_seed(0)
    init = [torch.randn(7, 3), torch.randn(5)]
    grads = [[torch.randn(7, 3), torch.randn(5)] for _ in range(4)]
    theirs_params = [torch.nn.Parameter(t.clone()) for t in init]
    theirs = torch.optim.Adam(_groups(theirs_params), lr=0.0, eps=1e-15, foreach=False)
    for gs in grads[:2]:
        for p, g in zip(theirs_params, gs):
            p.grad = g.clone()
        theirs.step()
    # torch -> this optimizer: the layout is kept, step is a 0-dim float32 CPU tensor
    ours_params = [torch.nn.Parameter(p.detach().clone()) for p in theirs_params]
    ours = Adam(_groups(ours_params), lr=0.0, eps=1e-15)
    ours.load_state_dict(copy.deepcopy(theirs.state_dict()))
    for p, q in zip(ours_params, theirs_params):
        a, b = ours.state[p], theirs.state[q]
        assert set(a) == {"step", "exp_avg", "exp_avg_sq"}
        assert a["step"].shape == () and a["step"].dtype == torch.float32 and a["step"].device.type == "cpu"
        assert float(a["step"]) == 2.0
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    assert [g["name"] for g in ours.param_groups] == ["anchor", "mlp_opacity"]
    assert [g["lr"] for g in ours.param_groups] == [0.01, 0.002] and ours.param_groups[0]["eps"] == 1e-15
    # this optimizer -> torch: a fresh torch.optim.Adam loaded from OUR state dict continues exactly as the first one does
    again_params = [torch.nn.Parameter(p.detach().clone()) for p in theirs_params]
    again = torch.optim.Adam(_groups(again_params), lr=0.5, eps=1e-3, foreach=False)
    again.load_state_dict(copy.deepcopy(ours.state_dict()))
    assert set(ours.state_dict()["param_groups"][0]) == set(theirs.state_dict()["param_groups"][0])
    for gs in grads[2:]:
        for opt_params in (theirs_params, again_params):
            for p, g in zip(opt_params, gs):
                p.grad = g.clone()
        theirs.step()
        again.step()
    for p, q in zip(again_params, theirs_params):
        assert torch.equal(p, q) and float(again.state[p]["step"]) == 4.0


def test_groups_keep_their_names_and_set_lrs_addresses_them():
    params = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))]
    opt = Adam(_groups(params), lr=0.0, eps=1e-15)
    assert [g["name"] for g in opt.param_groups] == ["anchor", "mlp_opacity"]
    assert opt.defaults["lr"] == 0.0 and opt.param_groups[0]["betas"] == (0.9, 0.999)
    opt.set_lrs({"anchor": 0.5, 1: 0.25})
    assert [g["lr"] for g in opt.param_groups] == [0.5, 0.25]
    opt.param_groups[0]["lr"] = 0.125          # update_learning_rate's own assignment
    assert opt.param_groups[0]["lr"] == 0.125
    with pytest.raises(KeyError):
        opt.set_lrs({"no_such_group": 1.0})
    with pytest.raises(KeyError):
        opt.set_lrs({2: 1.0})
    assert isinstance(opt, torch.optim.Optimizer)


def test_a_parameter_without_a_gradient_gets_no_state():
    params = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))]
    opt = Adam(_groups(params), lr=0.0, eps=1e-15)
    assert opt.step() is None                  # nothing has a gradient: nothing to do, on any device
    assert len(opt.state) == 0
    params[1].grad = torch.ones(2)             # (a CPU gradient: refused below, and still no state for either)
    with pytest.raises(ValueError, match="no CPU path"):
        opt.step()
    assert len(opt.state) == 0


def test_errors_come_in_the_siblings_order():
    def one(t, grad=True, **kw):
        p = torch.nn.Parameter(t)
        if grad:
            p.grad = torch.ones_like(t)
        return p, Adam([p], **kw)

    # TypeError first: a float64 parameter, although weight decay, amsgrad, the layout and the device are all wrong too
    p, opt = one(torch.zeros(4, 4, dtype=torch.float64).t(), weight_decay=0.1, amsgrad=True)
    with pytest.raises(TypeError, match="float32"):
        opt.step()
    # NotImplementedError next, naming the thing
    for kw, word in (({"weight_decay": 0.1}, "weight_decay"), ({"amsgrad": True}, "amsgrad")):
        p, opt = one(torch.zeros(4, 4).t(), **kw)
        with pytest.raises(NotImplementedError, match=word):
            opt.step()
    p, opt = one(torch.zeros(4, 4).t())
    opt.param_groups[0]["maximize"] = True
    with pytest.raises(NotImplementedError, match="maximize"):
        opt.step()
    p, opt = one(torch.zeros(4, 4), grad=False)
    p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 4))
    with pytest.raises(NotImplementedError, match="sparse"):
        opt.step()
    p, opt = one(torch.zeros(3))
    with pytest.raises(NotImplementedError, match="closure"):
        opt.step(lambda: 0.0)
    # ValueError: the layout and the shapes before the device
    p, opt = one(torch.zeros(4, 4).t())
    with pytest.raises(ValueError, match="contiguous"):
        opt.step()
    p, opt = one(torch.zeros(6))
    opt.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.zeros(5), "exp_avg_sq": torch.zeros(5)}   # botched surgery
    with pytest.raises(ValueError, match="exp_avg"):
        opt.step()
    # the device last: there is no CPU path
    p, opt = one(torch.zeros(6))
    with pytest.raises(ValueError, match="no CPU path"):
        opt.step()
    assert len(opt.state) == 0
    with pytest.raises(ValueError, match="no CPU path"):
        Adam([torch.nn.Parameter(torch.zeros(2))], capturable=True)
    for kw in ({"lr": -1.0}, {"eps": -1.0}, {"betas": (1.0, 0.999)}, {"betas": (0.9, -0.1)}):
        with pytest.raises(ValueError):
            Adam([torch.nn.Parameter(torch.zeros(2))], **kw)


def test_native_entry_point_refuses_before_any_launch():
    lib = _capi.lib()
    assert lib.bsr_adam_max_tensors() >= 1
    assert lib.bsr_adam_max_tensors() * 56 + 260 + 48 <= 4096      # the capturable form's descriptors fit the argument block
    ok = dict(p=16, g=32, m=48, v=64, numel=5, lr=0.01, step=1)     # (pointers that are never followed: every call below is refused)

    def call(n=1, b1=0.9, b2=0.999, eps=1e-15, **kw):
        arr = (_capi.AdamTensor * 1)()
        for k, val in {**ok, **kw}.items():
            setattr(arr[0], k, val)
        return lib.bsr_adam_step(n, arr, b1, b2, eps, None), _capi.last_error()

    def refused(words, **kw):
        rc, err = call(**kw)
        assert rc != 0 and err.startswith("bsr_adam_step: ") and words in err, (kw, err)

    refused("need n_tensors >= 0", n=-1)
    refused("NULL buffer", p=None)
    refused("NULL buffer", v=None)
    refused("numel must be in [0, 2^31)", numel=1 << 31)
    refused("numel must be in [0, 2^31)", numel=-1)
    refused("beta1 must be in [0, 1)", b1=1.0)
    refused("beta2 must be in [0, 1)", b2=-0.5)
    refused("need eps >= 0", eps=-1e-8)
    refused("must be finite", eps=float("inf"))
    refused("must be finite", b1=float("nan"))
    refused("lr must be finite", lr=float("nan"))
    refused("need step >= 1", step=0)
    refused("lr_dev and step_dev come together", lr_dev=16)
    arr = (_capi.AdamTensor * 2)()
    for d, cap in zip(arr, (None, 128)):
        for k, val in ok.items():
            setattr(d, k, val)
        d.lr_dev = d.step_dev = cap
    assert lib.bsr_adam_step(2, arr, 0.9, 0.999, 1e-15, None) != 0 and "cannot share a call" in _capi.last_error()
    assert lib.bsr_adam_step(1, None, 0.9, 0.999, 1e-15, None) != 0 and "NULL tensor array" in _capi.last_error()
    # nothing to do is not an error, and launches nothing: no tensors, or none with elements (its pointers are not looked at)
    assert lib.bsr_adam_step(0, None, 0.9, 0.999, 1e-15, None) == 0 and _capi.last_error() == ""
    empty = (_capi.AdamTensor * 1)()
    assert lib.bsr_adam_step(1, empty, 0.9, 0.999, 1e-15, None) == 0 and _capi.last_error() == ""
