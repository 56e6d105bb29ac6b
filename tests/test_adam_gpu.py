"""The fused Adam step on the GPU (include/bloomscene_adam.h, bloomscene_amd/optim.py).  Every case is compared BIT FOR BIT
with tests/adam_reference.py for the parameter and both moments (any NaN equals any NaN: the header leaves its sign and
payload open); the last tests hold it against eager torch.optim.Adam on the same device by the siblings' rule, and check
that the library owns no device memory and waits for nothing."""
import numpy as np
import pytest
import torch

import adam_reference as AR
from bloomscene_amd import _capi
from bloomscene_amd.optim import Adam

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = "cuda:0"
C = 4096                      # BSR_ADAM_CHUNK of include/bloomscene_adam.h (test_chunk_size_is_the_headers checks it)
BETAS, EPS = (0.9, 0.999), 1e-15


class Mirror:
    """The restatement's side of an optimizer: numpy copies of every parameter, its moments and its step count."""

    def __init__(self, params, betas=BETAS, eps=EPS):
        self.p = [p.detach().cpu().numpy().copy() for p in params]
        self.m = [np.zeros_like(a) for a in self.p]
        self.v = [np.zeros_like(a) for a in self.p]
        self.t = [0] * len(self.p)
        self.betas, self.eps = betas, eps

    def step(self, grads, lrs):
        """grads[i] is None for a parameter without a gradient: it is not stepped."""
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.t[i] += 1
            self.p[i], self.m[i], self.v[i] = AR.adam_step(self.p[i], g, self.m[i], self.v[i], lrs[i], self.t[i],
                                                           self.betas[0], self.betas[1], self.eps)

    def assert_equals(self, opt, params, what=""):
        torch.cuda.synchronize()
        for i, p in enumerate(params):
            st = opt.state.get(p)
            if self.t[i] == 0:
                assert not st, (what, i, "a parameter that never had a gradient has state")
                assert AR.bits_equal(p.detach().cpu().numpy(), self.p[i]), (what, i)
                continue
            assert float(st["step"]) == self.t[i], (what, i, float(st["step"]), self.t[i])
            for name, got, ref in (("p", p.detach(), self.p[i]), ("exp_avg", st["exp_avg"], self.m[i]),
                                   ("exp_avg_sq", st["exp_avg_sq"], self.v[i])):
                assert AR.bits_equal(got.cpu().numpy(), ref), (what, i, name, tuple(ref.shape))


def _grads(rng, params, skip=()):
    return [None if i in skip else (rng.standard_normal(tuple(p.shape)) * 10.0 ** rng.uniform(-3, 0)).astype(F32)
            for i, p in enumerate(params)]


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else torch.from_numpy(g).to(DEV)


def _param(rng, shape):
    return torch.nn.Parameter(torch.from_numpy(rng.standard_normal(shape).astype(F32)).to(DEV))


def test_chunk_size_is_the_headers():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bloomscene_adam.h")).read()
    assert int(re.search(r"#define BSR_ADAM_CHUNK (\d+)", hdr).group(1)) == C and C % 1024 == 0
    assert int(re.search(r"#define BSR_ADAM_MAX_TENSORS (\d+)", hdr).group(1)) == _capi.lib().bsr_adam_max_tensors()


@pytest.mark.parametrize("numel", [1, 3, 4, 5, 255, 1024, C - 1, C, C + 1, 2 * C + 7])
def test_single_tensor(numel):
    rng = np.random.default_rng(numel)
    params = [_param(rng, (numel,))]
    opt, mirror = Adam(params, lr=0.01, eps=EPS), Mirror(params)
    for _ in range(2):
        grads = _grads(rng, params)
        _set_grads(params, grads)
        opt.step()
        mirror.step(grads, [0.01])
    mirror.assert_equals(opt, params)


def test_an_empty_tensor_beside_a_non_empty_neighbour():
    rng = np.random.default_rng(7)
    params = [_param(rng, (0,)), _param(rng, (5,)), _param(rng, (0, 3)), _param(rng, (C + 2,)), _param(rng, (0,))]
    opt, mirror = Adam(params, lr=0.02, eps=EPS), Mirror(params)
    for _ in range(2):
        grads = _grads(rng, params)
        _set_grads(params, grads)
        opt.step()
        mirror.step(grads, [0.02] * len(params))
    mirror.assert_equals(opt, params)


@pytest.mark.parametrize("which", ["p+1", "p+3", "p+3,g+1", "m+1,v+3", "all+1"])
def test_views_at_storage_offsets(which):
    """Some or all of the four pointers 4 or 12 bytes off a 16-byte boundary: the element-by-element path, more than one
    workgroup, the neighbours of the view untouched."""
    n = C + 5
    rng = np.random.default_rng(11)
    off = {k: 0 for k in "pgmv"}
    for item in which.split(","):
        name, o = item.split("+")
        for k in ("pgmv" if name == "all" else name):
            off[k] = int(o)

    def view(values, o):
        base = torch.full((n + 8,), 77.0, device=DEV)
        base[o:o + n] = torch.from_numpy(values).to(DEV)
        return base, base[o:o + n]

    p_base, p_view = view(rng.standard_normal(n).astype(F32), off["p"])
    p = torch.nn.Parameter(p_view)
    assert p.data_ptr() % 16 == 4 * off["p"] and p.is_contiguous()
    opt, mirror = Adam([p], lr=0.01, eps=EPS), Mirror([p])
    m_base, m_view = view(np.zeros(n, F32), off["m"])
    v_base, v_view = view(np.zeros(n, F32), off["v"])
    opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": m_view, "exp_avg_sq": v_view}
    for _ in range(2):
        g = _grads(rng, [p])[0]
        g_base, g_view = view(g, off["g"])
        p.grad = g_view
        assert g_view.data_ptr() % 16 == 4 * off["g"]
        opt.step()
        mirror.step([g], [0.01])
    mirror.assert_equals(opt, [p], which)
    for base, o in ((p_base, off["p"]), (m_base, off["m"]), (v_base, off["v"])):
        assert bool((base[:o] == 77.0).all()) and bool((base[o + n:] == 77.0).all())


def _model(rng, N=129, F=5, K=3):
    """The reference's parameter groups in small: seven per-anchor tensors, three Linear-ReLU-Linear stacks, four tables."""
    groups = []

    def add(name, shapes, lr):
        groups.append({"params": [_param(rng, s) for s in shapes], "lr": lr, "name": name})

    add("anchor", [(N, 3)], 0.0)
    add("offset", [(N, K, 3)], 0.01)
    add("mask", [(N, K, 1)], 0.0075)
    add("anchor_feat", [(N, F)], 0.0075)
    add("opacity", [(N, 1)], 0.02)
    add("scaling", [(N, 6)], 0.007)
    add("rotation", [(N, 4)], 0.002)
    for name, out, lr in (("mlp_opacity", K, 0.002), ("mlp_cov", 7 * K, 0.004), ("mlp_color", 3 * K, 0.008)):
        add(name, [(F, F + 3), (F,), (out, F), (out,)], lr)
    add("encoding_xyz", [(301, 2), (257, 2), (199, 2), (512, 2)], 0.005)
    return groups


def test_model_shaped_set_three_steps_with_a_rate_per_group():
    rng = np.random.default_rng(3)
    groups = _model(rng)
    params = [p for g in groups for p in g["params"]]
    lrs = [g["lr"] for g in groups for _ in g["params"]]
    no_grad = {i for i, p in enumerate(params) if tuple(p.shape) in ((129, 1), (129, 4))}     # opacity, rotation
    assert len(no_grad) == 2 and len(params) == 7 + 12 + 4
    opt, mirror = Adam(groups, lr=0.0, eps=EPS), Mirror(params)
    anchor0 = params[0].detach().clone()
    for k in range(3):
        grads = _grads(rng, params, skip=no_grad)
        _set_grads(params, grads)
        opt.step()
        mirror.step(grads, lrs)
        mirror.assert_equals(opt, params, f"step {k + 1}")
    # lr = 0 (the anchor group): the parameter keeps its bits while its moments move
    assert torch.equal(params[0].detach().view(torch.int32), anchor0.view(torch.int32))
    assert float(opt.state[params[0]]["exp_avg"].abs().max()) > 0 and float(opt.state[params[0]]["exp_avg_sq"].max()) > 0
    assert [g["name"] for g in opt.param_groups][:3] == ["anchor", "offset", "mask"]
    assert all(not opt.state.get(params[i]) for i in no_grad)


def test_more_tensors_than_one_launch_takes():
    """bsr_adam_max_tensors() + 3 tensors of 1 to 9 elements: the second launch, and the prefix search at both ends."""
    n = _capi.lib().bsr_adam_max_tensors() + 3
    rng = np.random.default_rng(5)
    params = [_param(rng, (1 + k % 9,)) for k in range(n)]
    opt, mirror = Adam(params, lr=0.03, eps=EPS), Mirror(params)
    for _ in range(2):
        grads = _grads(rng, params)
        _set_grads(params, grads)
        opt.step()
        mirror.step(grads, [0.03] * n)
    mirror.assert_equals(opt, params)


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("t0", [1, 2000, 30_000])
def test_steps_that_start_late(t0, capturable):
    rng = np.random.default_rng(t0)
    params = [_param(rng, (1000,)), _param(rng, (37,))]
    opt, mirror = Adam(params, lr=0.0075, eps=EPS, capturable=capturable), Mirror(params)
    lr = float(F32(0.0075)) if capturable else 0.0075
    for i, p in enumerate(params):
        mirror.t[i] = t0 - 1
        mirror.m[i] = (rng.standard_normal(tuple(p.shape)) * 0.1).astype(F32)
        mirror.v[i] = (rng.random(tuple(p.shape)) * 0.01).astype(F32)
        if t0 > 1:
            opt.state[p] = {"step": torch.tensor(float(t0 - 1), device=DEV if capturable else "cpu"),
                            "exp_avg": torch.from_numpy(mirror.m[i]).to(DEV), "exp_avg_sq": torch.from_numpy(mirror.v[i]).to(DEV)}
        else:
            mirror.m[i][:], mirror.v[i][:] = 0, 0
    for _ in range(2):
        grads = _grads(rng, params)
        _set_grads(params, grads)
        opt.step()
        mirror.step(grads, [lr, lr])
    mirror.assert_equals(opt, params, f"t0 = {t0}")


def test_special_values():
    g = np.array([0.0, 1e-23, -1e-23, 0.0, -0.0, 1e20, -1e20, np.inf, -np.inf, np.nan, 1.0, 3e-20, -1e-30, 1e-45], F32)
    p0 = np.array([1.5, -2.0, 3.0, 0.0, -0.0, 4.0, -5.0, 6.0, 7.0, 8.0, -0.0, 1e-30, 2.0, -1.0], F32)
    with np.errstate(all="ignore"):
        sq = g * g
    # squares that underflow past the subnormals (1e-46), that are subnormal (9e-40) and that overflow
    assert sq[1] == 0 and 0 < sq[11] < np.finfo(F32).tiny and np.isinf(sq[5])
    params = [torch.nn.Parameter(torch.from_numpy(p0.copy()).to(DEV))]
    opt, mirror = Adam(params, lr=0.01, eps=EPS), Mirror(params)
    rng = np.random.default_rng(9)
    for k, gk in enumerate([g, g, rng.standard_normal(g.shape).astype(F32)]):
        _set_grads(params, [gk])
        opt.step()
        mirror.step([gk], [0.01])
        mirror.assert_equals(opt, params, f"step {k + 1}")
        if k == 0:
            got = params[0].detach().cpu().numpy()
            # g = 0 on zero moments leaves p alone (no 0 / 0: eps > 0); an overflowing square leaves p alone too
            assert AR.bits_equal(got[[0, 3, 4, 5, 6]], p0[[0, 3, 4, 5, 6]])
            assert np.isnan(got[[7, 8, 9]]).all() and not np.isnan(np.delete(got, [7, 8, 9])).any()
            v = opt.state[params[0]]["exp_avg_sq"].cpu().numpy()
            assert np.isinf(v[[5, 6, 7, 8]]).all() and v[0] == 0


def test_surgery_between_steps():
    """What the reference's densification does to an optimizer, in this test's own lines: rows pruned by a mask with
    sliced moments, rows appended with zero moments and the inherited step, a parameter swapped for a new one of another
    size with fresh moments.  The step after each is the restatement's on the same arrays."""
    rng = np.random.default_rng(13)
    groups = [{"params": [_param(rng, (1500, 4))], "lr": 0.01, "name": "scaling"},
              {"params": [_param(rng, (33, 2))], "lr": 0.002, "name": "table"}]
    opt = Adam(groups, lr=0.0, eps=EPS)
    params = [g["params"][0] for g in opt.param_groups]
    mirror, lrs = Mirror(params), [0.01, 0.002]

    def step():
        grads = _grads(rng, params)
        _set_grads(params, grads)
        opt.step()
        mirror.step(grads, lrs)

    def replace(i, new_values, new_m, new_v):
        group, old = opt.param_groups[i], params[i]
        stored = opt.state.pop(old)
        stored["exp_avg"], stored["exp_avg_sq"] = new_m, new_v          # "step" is inherited
        new = torch.nn.Parameter(new_values.contiguous())
        group["params"][0] = new
        opt.state[new] = stored
        params[i] = new
        mirror.p[i], mirror.m[i], mirror.v[i] = (t.detach().cpu().numpy().copy() for t in (new, new_m, new_v))

    step()
    step()
    keep = torch.from_numpy(rng.random(1500) < 0.7).to(DEV)             # prune
    st = opt.state[params[0]]
    replace(0, params[0].detach()[keep], st["exp_avg"][keep].contiguous(), st["exp_avg_sq"][keep].contiguous())
    step()
    mirror.assert_equals(opt, params, "after the prune")
    extra = torch.from_numpy(rng.standard_normal((211, 4)).astype(F32)).to(DEV)   # append
    st = opt.state[params[0]]
    replace(0, torch.cat([params[0].detach(), extra]), torch.cat([st["exp_avg"], torch.zeros_like(extra)]),
            torch.cat([st["exp_avg_sq"], torch.zeros_like(extra)]))
    step()
    mirror.assert_equals(opt, params, "after the append")
    fresh = torch.from_numpy(rng.standard_normal((C + 9, 2)).astype(F32)).to(DEV)  # swap for another size
    replace(1, fresh, torch.zeros_like(fresh), torch.zeros_like(fresh))
    step()
    mirror.assert_equals(opt, params, "after the swap")
    assert mirror.t == [5, 5] and [g["name"] for g in opt.param_groups] == ["scaling", "table"]


FP32_RATES = [0.0078125, 0.001953125, 0.0, 0.5]       # exactly representable: the two forms must agree bit for bit


def test_capturable_form_equals_the_default_form_and_replays_from_a_graph():
    rng = np.random.default_rng(17)
    shapes = [(C + 3,), (50, 7), (9,)]
    init = [rng.standard_normal(s).astype(F32) for s in shapes]
    names = ["a", "b", "c"]

    def make(capturable):
        params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in init]
        groups = [{"params": [p], "lr": FP32_RATES[0], "name": n} for p, n in zip(params, names)]
        return params, Adam(groups, lr=0.0, eps=EPS, capturable=capturable)

    all_grads = [[rng.standard_normal(s).astype(F32) for s in shapes] for _ in range(4)]
    rates = [[FP32_RATES[(k + i) % 4] for i in range(3)] for k in range(4)]          # per step, per group
    # the two forms, eagerly, four steps
    (dp, dopt), (cp, copt) = make(False), make(True)
    mirror = Mirror(dp)
    for k in range(4):
        for params, opt in ((dp, dopt), (cp, copt)):
            _set_grads(params, all_grads[k])
            opt.set_lrs(dict(zip(names, rates[k])))
            opt.step()
        mirror.step(all_grads[k], rates[k])
    mirror.assert_equals(dopt, dp, "default form")
    mirror.assert_equals(copt, cp, "capturable form")
    for g in copt.param_groups:
        assert isinstance(g["lr"], torch.Tensor) and g["lr"].shape == () and g["lr"].device.type == "cuda"
    assert len({g["lr"].untyped_storage().data_ptr() for g in copt.param_groups}) == 1     # views of ONE tensor
    copt.param_groups[1]["lr"] = 0.01
    with pytest.raises(ValueError, match="set_lrs"):
        copt.step()
    # captured on one stream after a warm-up step, replayed three times with set_lrs between the replays
    gp, gopt = make(True)
    mirror = Mirror(gp)
    static_grads = [torch.zeros(s, device=DEV) for s in shapes]
    for p, g in zip(gp, static_grads):
        p.grad = g

    def feed(k):
        for dst, src in zip(static_grads, all_grads[k]):
            dst.copy_(torch.from_numpy(src))
        gopt.set_lrs(dict(zip(names, rates[k])))
        mirror.step(all_grads[k], rates[k])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        feed(0)
        gopt.step()                                       # the warm-up: t = 1, creates the state
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gopt.step()
    for k in (1, 2, 3):
        feed(k)
        graph.replay()
        mirror.assert_equals(gopt, gp, f"replay at t = {k + 1}")
    assert all(float(gopt.state[p]["step"]) == 4.0 and gopt.state[p]["step"].device.type == "cuda" for p in gp)


def test_capturable_optimizer_takes_a_default_state_dict_a_new_group_and_gives_it_back():
    """load_state_dict brings `step` and the rates to each form's places (the device and the one rate tensor, or the CPU and
    python numbers); add_param_group re-seats every rate view on a longer tensor."""
    rng = np.random.default_rng(31)
    shapes, names, rates = [(C + 1,), (21, 3)], ["a", "b"], [2.0 ** -7, 2.0 ** -9]

    def groups(params, ns, lrs):
        return [{"params": [p], "lr": lr, "name": n} for p, n, lr in zip(params, ns, lrs)]

    def clones(params):
        return [torch.nn.Parameter(p.detach().clone()) for p in params]

    d_params = [_param(rng, s) for s in shapes]
    d_opt, mirror = Adam(groups(d_params, names, rates), lr=0.0, eps=EPS), Mirror(d_params)
    grads = _grads(rng, d_params)
    _set_grads(d_params, grads)
    d_opt.step()
    mirror.step(grads, rates)
    c_params = clones(d_params)
    c_opt = Adam(groups(c_params, names, [0.5, 0.5]), lr=0.0, eps=EPS, capturable=True)
    c_opt.load_state_dict(d_opt.state_dict())
    assert all(c_opt.state[p]["step"].device.type == "cuda" and float(c_opt.state[p]["step"]) == 1.0 for p in c_params)
    assert [float(g["lr"]) for g in c_opt.param_groups] == rates
    extra = _param(rng, (11,))
    c_opt.add_param_group({"params": [extra], "lr": 2.0 ** -5, "name": "c"})
    c_params, names, rates = c_params + [extra], names + ["c"], rates + [2.0 ** -5]
    assert [float(g["lr"]) for g in c_opt.param_groups] == rates
    assert len({g["lr"].untyped_storage().data_ptr() for g in c_opt.param_groups}) == 1 and len(c_opt.param_groups) == 3
    grown = Mirror(c_params)
    grown.m[:2], grown.v[:2], grown.t[:2] = mirror.m, mirror.v, mirror.t
    grads = _grads(rng, c_params)
    _set_grads(c_params, grads)
    c_opt.step()
    grown.step(grads, rates)
    grown.assert_equals(c_opt, c_params, "capturable, after load_state_dict and add_param_group")
    b_params = clones(c_params)                                  # ... and back into the default form
    b_opt = Adam(groups(b_params, names, [0.5] * 3), lr=0.0, eps=EPS)
    b_opt.load_state_dict(c_opt.state_dict())
    assert all(type(g["lr"]) is float for g in b_opt.param_groups) and [g["lr"] for g in b_opt.param_groups] == rates
    assert all(b_opt.state[p]["step"].device.type == "cpu" for p in b_params)
    grads = _grads(rng, b_params)
    _set_grads(b_params, grads)
    b_opt.step()
    grown.step(grads, rates)
    grown.assert_equals(b_opt, b_params, "default, after loading the capturable state dict")


def test_state_dict_moves_to_torch_adam_and_back_on_the_device():
    rng = np.random.default_rng(19)
    init = [rng.standard_normal(s).astype(F32) for s in ((300, 3), (17,))]
    grads = [[rng.standard_normal(a.shape).astype(F32) for a in init] for _ in range(3)]

    def make(cls, **kw):
        params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in init]
        return params, cls([{"params": [p], "lr": 0.01, "name": f"g{i}"} for i, p in enumerate(params)], lr=0.0, eps=EPS, **kw)

    p1, ours = make(Adam)
    mirror = Mirror(p1)
    _set_grads(p1, grads[0])
    ours.step()
    mirror.step(grads[0], [0.01, 0.01])
    p2, theirs = make(torch.optim.Adam, foreach=False)           # ours -> torch: it takes the state and steps on
    theirs.load_state_dict(ours.state_dict())
    with torch.no_grad():
        for a, b in zip(p2, p1):
            a.copy_(b)
    _set_grads(p2, grads[1])
    theirs.step()
    assert all(float(theirs.state[p]["step"]) == 2.0 for p in p2)
    p3, back = make(Adam)                                         # torch -> ours: the next step is the restatement's
    back.load_state_dict(theirs.state_dict())
    with torch.no_grad():
        for a, b in zip(p3, p2):
            a.copy_(b)
    for i, p in enumerate(p2):
        mirror.t[i] = 2
        mirror.p[i] = p.detach().cpu().numpy().copy()
        mirror.m[i] = theirs.state[p]["exp_avg"].cpu().numpy().copy()
        mirror.v[i] = theirs.state[p]["exp_avg_sq"].cpu().numpy().copy()
    _set_grads(p3, grads[2])
    back.step()
    mirror.step(grads[2], [0.01, 0.01])
    mirror.assert_equals(back, p3)
    assert [g["name"] for g in back.param_groups] == ["g0", "g1"]


@pytest.mark.parametrize("foreach", [False, None])
def test_no_further_from_a_float64_adam_than_eager_torch(foreach):
    """The siblings' rule: after five steps the kernel's distance from a float64 Adam is at most twice eager
    torch.optim.Adam's on the same device, plus 2^-23 of the tensor's scale -- for p, m and v."""
    rng = np.random.default_rng(23)
    shapes, lr, eps = [(2 * C + 5,), (129, 5)], 0.01, 1e-8
    init = [rng.standard_normal(s).astype(F32) for s in shapes]
    grads = [[(rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 0, s)).astype(F32) for s in shapes] for _ in range(5)]

    def run(cls, **kw):
        params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in init]
        opt = cls(params, lr=lr, eps=eps, **kw)
        for gs in grads:
            _set_grads(params, gs)
            opt.step()
        torch.cuda.synchronize()
        return [(p.detach().cpu().numpy(), opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy())
                for p in params]

    ours, eager = run(Adam), run(torch.optim.Adam, foreach=foreach)
    for i, a in enumerate(init):
        ref = (a.astype(np.float64), np.zeros(a.shape), np.zeros(a.shape))
        for t, gs in enumerate(grads, 1):
            ref = AR.adam_step_f64(*ref[:1], gs[i], *ref[1:], lr, t, 0.9, 0.999, eps)
        for name, r, o, e in zip(("p", "m", "v"), ref, ours[i], eager[i]):
            d_ours, d_eager, scale = np.abs(o - r).max(), np.abs(e - r).max(), np.abs(r).max()
            print(f"tensor {i} {name}: kernel {d_ours:.3e}, eager torch (foreach={foreach}) {d_eager:.3e}, scale {scale:.3e}")
            assert d_ours <= 2 * d_eager + 2.0 ** -23 * scale, (i, name, d_ours, d_eager, scale)


def test_the_library_owns_no_device_memory_and_waits_for_nothing():
    rng = np.random.default_rng(29)
    params = [_param(rng, (3 * C + 1,)), _param(rng, (64, 3)), _param(rng, (5,))]
    opt = Adam(params, lr=0.01, eps=EPS)
    _set_grads(params, _grads(rng, params))
    opt.step()                                             # creates the state: the only allocations there ever are
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    torch.cuda.set_sync_debug_mode("error")                # a torch call that waits on the host raises
    try:
        for _ in range(20):
            opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == before and torch.cuda.max_memory_allocated() == before
    # ... and the library's own calls wait for nothing either: a stream capture refuses any that would
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()                                         # (the default form bakes lr and t into the launch: captured, not replayed)
    torch.cuda.synchronize()
    assert float(opt.state[params[0]]["step"]) == 22.0      # (the graph object keeps a KiB of torch's own: not compared again)
