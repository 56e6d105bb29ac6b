"""Restatements of include/bloomscene_adjust.h for the tests, written from the header.

  (a) ``decide_ref`` / ``resize_ref``   A and B of the header in numpy, per row
  (b) ``adjust_anchor_ref``             the whole of GM:898-952 as a sequence of its own lines over numpy arrays: boolean
                                        indexing, concatenation, np.unique(axis=0), and the header's fp32 threshold rule
  (c) ``eager_adjust``                  the same sequence in eager torch on a duck-typed model, on the device of its
                                        tensors (what the fused call replaces and is timed against)
  (d) ``Model`` / ``make_state``        a seeded duck-typed model with the attributes adjust_anchor uses

Two functions of the device's libm enter the values that are MOVED here, exp in get_scaling and log in the new anchors'
scaling and opacity.  They are not this feature's to restate: (b) takes them as callables and the tests hand it the ones of
the torch build the comparison runs against.
"""
import numpy as np
import torch

from anchor_state_reference import quantize_anchor_np
from densify_reference import scatter_max_ref
from voxel_reference import grow_level_eager, quantise_ref

F32 = np.float32
PARAMS = ("anchor", "offset", "mask", "anchor_feat", "opacity", "scaling", "rotation")
SKIPPED = ("mlp", "conv", "feat_base", "encoding")


def fl32(x):
    """A python double rounded to fp32 once: what torch compares a float32 tensor with."""
    return F32(float(x))


# ---- (a) ----

def decide_ref(opacity_accum, anchor_demon, offset_gradient_accum, offset_denom, K, thresholds, check_interval=100,
               success_threshold=0.8, min_opacity=0.005):
    """-> (offset_flags uint8 [N K], anchor_flags uint8 [N], src_of int32 [n_keep], status [4])."""
    s, d = (np.asarray(a, F32).reshape(-1) for a in (opacity_accum, anchor_demon))
    acc, den = (np.asarray(a, F32).reshape(-1) for a in (offset_gradient_accum, offset_denom))
    assert acc.shape[0] == s.shape[0] * K
    with np.errstate(all="ignore"):
        q = (acc / den).astype(F32)
        q = np.where(np.isnan(q), F32(0), q)
        g = np.abs(q)
        om = den > fl32(check_interval * success_threshold * 0.5)
        offset_flags = np.where(om, 0x80, 0).astype(np.uint8)
        for i, t in enumerate(thresholds):
            offset_flags |= np.where((g >= fl32(t)) & om, 1 << i, 0).astype(np.uint8)
        am = d > fl32(check_interval * success_threshold)
        prune = (s < (fl32(min_opacity) * d).astype(F32)) & am
    anchor_flags = (prune.astype(np.uint8) | (am.astype(np.uint8) << 1)).astype(np.uint8)
    src_of = np.nonzero(~prune)[0].astype(np.int32)
    status = [int(src_of.shape[0]), int(am.sum()), int(om.sum()), 0]
    return offset_flags, anchor_flags, src_of, status


def resize_ref(src, src_of, n_keep, A, append=None, fill=0, op=None):
    """One tensor of bsr_rows_resize on bit patterns.  src [N, ...] float32 or int32; fill a uint32 bit pattern;
    op None, ("zero_flagged", flags, mask, per_element) or ("clamp_from", column, bound).  -> uint32 [n_keep + A, width]."""
    src = np.ascontiguousarray(src)
    N = src.shape[0]
    w = int(np.prod(src.shape[1:], dtype=np.int64))
    bits = src.reshape(N, w).view(np.uint32)
    out = np.zeros((n_keep + A, w), np.uint32)
    rows = np.asarray(src_of[:n_keep], np.int64)
    inside = (rows >= 0) & (rows < N)
    rows = rows[inside]                                             # an entry outside [0, N) leaves its row zero
    kept = bits[rows]
    if op is not None and op[0] == "zero_flagged":
        flags = np.asarray(op[1], np.uint8).reshape(-1)
        hit = flags.reshape(N, w)[rows] if op[3] else flags[rows][:, None]
        kept = np.where((hit & op[2]) != 0, np.uint32(0), kept)
    out[:n_keep][inside] = kept
    if A:
        out[n_keep:] = np.ascontiguousarray(append).reshape(A, w).view(np.uint32) if append is not None else np.uint32(fill)
    if op is not None and op[0] == "clamp_from":
        v = out.view(F32)
        with np.errstate(all="ignore"):
            over = v > fl32(op[2])
        over[:, :op[1]] = False
        out[over] = np.array([op[2]], F32).view(np.uint32)[0]
    return out


def boundary_stats(K, thresholds, check_interval=100, success_threshold=0.8, min_opacity=0.005):
    """Statistics that sit ON every threshold and one ulp on either side of it -> (opacity_accum [N], anchor_demon [N],
    offset_gradient_accum [N K], offset_denom [N K]).  g = fl32(t_i) and its neighbours (the count 64 makes accum / 64
    exact), counts of 40 and 80 and their neighbours, s = fl(mo d) and its neighbours, 0 / 0 and NaN statistics."""
    up = lambda x: np.nextafter(F32(x), F32(np.inf))
    down = lambda x: np.nextafter(F32(x), F32(-np.inf))
    three = lambda x: [down(x), F32(x), up(x)]
    offsets = []                                                    # (accum, denom)
    for t in thresholds:
        for g in three(fl32(t)):
            offsets += [(g * F32(64), F32(64)), (g * F32(32), F32(32)), (-g * F32(64), F32(64))]
    for d in three(fl32(check_interval * success_threshold * 0.5)):
        offsets += [(F32(1), d), (F32(1e-9), d)]
    offsets += [(F32(0), F32(0)), (F32(1), F32(0)), (F32(np.nan), F32(64)), (F32(1), F32(np.nan)), (F32(3.3e-23) * F32(64), F32(64))]
    anchors = []                                                    # (s, d)
    for d in three(fl32(check_interval * success_threshold)):
        anchors += [(F32(0), d), (F32(10), d)]
    for d in (F32(100), F32(81), F32(333)):
        for s in three((fl32(min_opacity) * d).astype(F32)):
            anchors.append((s, d))
    anchors += [(F32(0), F32(0)), (F32(np.nan), F32(100)), (F32(0), F32(np.nan)), (F32(-1), F32(100))]
    N = max(len(anchors), -(-len(offsets) // K))
    offsets += [(F32(0), F32(0))] * (N * K - len(offsets))
    anchors += [(F32(1), F32(10))] * (N - len(anchors))
    a, o = np.array(anchors, F32), np.array(offsets, F32)
    return a[:, 0].copy(), a[:, 1].copy(), o[:, 0].copy(), o[:, 1].copy()


# ---- (b) ----

def _torch_exp(x):
    return torch.exp(torch.from_numpy(np.ascontiguousarray(x, F32))).numpy()


def _torch_log(x):
    return torch.log(torch.from_numpy(np.ascontiguousarray(x, F32))).numpy()


def adjust_anchor_ref(state, cfg, rand, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, min_opacity=0.005,
                      rule="divide", exp_fn=_torch_exp, log_fn=_torch_log):
    """``state``: {"params": {name: array}, "moments": {name: (exp_avg, exp_avg_sq)} for the groups that have state,
    "opacity_accum" [N, 1], "anchor_demon" [N, 1], "offset_gradient_accum" [N K, 1], "offset_denom" [N K, 1],
    "bound_min" [1, 3], "bound_max" [1, 3]}; ``cfg``: an object with n_offsets, voxel_size, update_depth, update_init_factor,
    update_hierachy_factor; ``rand``: update_depth arrays [N K].  ``rule``: how the comparison's torch divides a tensor by
    a python scalar (voxel_reference.quantise_ref).  -> (the new state, levels): levels[i] = anchors level i added."""
    K = cfg.n_offsets
    P = {k: np.array(v, F32) for k, v in state["params"].items()}
    M = {k: (np.array(m, F32), np.array(v, F32)) for k, (m, v) in state["moments"].items()}
    opacity_accum, anchor_demon = np.array(state["opacity_accum"], F32), np.array(state["anchor_demon"], F32)
    accum, denom = np.array(state["offset_gradient_accum"], F32), np.array(state["offset_denom"], F32)
    bmin, bmax = np.asarray(state["bound_min"], F32).reshape(1, 3), np.asarray(state["bound_max"], F32).reshape(1, 3)
    N = P["anchor"].shape[0]
    with np.errstate(all="ignore"):
        grads = (accum / denom).astype(F32)
    grads[np.isnan(grads)] = 0
    g = np.abs(grads).reshape(-1)
    offset_mask = (denom > fl32(check_interval * success_threshold * 0.5)).reshape(-1)
    levels = []
    for i in range(cfg.update_depth):
        levels.append(0)
        candidate = (g >= fl32(grad_threshold * ((cfg.update_hierachy_factor // 2) ** i))) & offset_mask
        candidate &= np.asarray(rand[i], F32).reshape(-1) > fl32(0.5 ** (i + 1))
        if P["anchor"].shape[0] == N and i > 0:
            continue                                                # the level-skip quirk
        get_anchor = quantize_anchor_np(P["anchor"], bmin, bmax)
        get_scaling = exp_fn(P["scaling"])
        # the candidates are old offsets only: the new anchors' part of the mask is zero padding
        xyz = (get_anchor[:N, None, :] + (P["offset"][:N] * get_scaling[:N, None, :3]).astype(F32)).astype(F32)
        cur_size = cfg.voxel_size * (cfg.update_init_factor // (cfg.update_hierachy_factor ** i))
        grid, _ = quantise_ref(get_anchor, cur_size, rule)
        picked = np.nonzero(candidate)[0]
        if picked.shape[0] == 0:
            continue
        selected, _ = quantise_ref(xyz.reshape(-1, 3)[picked], cur_size, rule)
        unique, inverse = np.unique(selected, axis=0, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
        occupied = {tuple(row) for row in grid.tolist()}
        fresh = np.array([tuple(row) not in occupied for row in unique.tolist()], bool)
        new_anchor = (unique[fresh].astype(F32) * fl32(cur_size)).astype(F32)
        A = new_anchor.shape[0]
        if A == 0:
            continue
        levels[-1] = A
        new_feat, _ = scatter_max_ref(P["anchor_feat"][picked // K], inverse, unique.shape[0])
        one = np.ones((1,), F32)
        block = {
            "anchor": new_anchor,
            "scaling": log_fn(np.full((A, 6), fl32(cur_size), F32)),
            "rotation": np.tile(np.array([1, 0, 0, 0], F32), (A, 1)),
            "anchor_feat": new_feat[fresh],
            "offset": np.zeros((A, K, 3), F32),
            "mask": np.ones((A, K, 1), F32),
            "opacity": np.broadcast_to(log_fn(((fl32(0.1) * one) / (one - fl32(0.1) * one)).astype(F32)), (A, 1)),
        }
        for name in P:
            P[name] = np.concatenate([P[name], block[name].astype(F32)])
            if name in M:
                M[name] = tuple(np.concatenate([m, np.zeros_like(block[name], F32)]) for m in M[name])
        opacity_accum = np.concatenate([opacity_accum, np.zeros((A, 1), F32)])
        anchor_demon = np.concatenate([anchor_demon, np.zeros((A, 1), F32)])
    grown = P["anchor"].shape[0]
    denom[offset_mask] = 0
    accum[offset_mask] = 0
    denom = np.concatenate([denom, np.zeros(((grown - N) * K, 1), F32)])
    accum = np.concatenate([accum, np.zeros(((grown - N) * K, 1), F32)])
    anchors_mask = (anchor_demon > fl32(check_interval * success_threshold)).reshape(-1)
    prune = (opacity_accum < (fl32(min_opacity) * anchor_demon).astype(F32)).reshape(-1) & anchors_mask
    keep = ~prune
    denom = denom.reshape(-1, K)[keep].reshape(-1, 1)
    accum = accum.reshape(-1, K)[keep].reshape(-1, 1)
    opacity_accum[anchors_mask] = 0
    anchor_demon[anchors_mask] = 0
    for name in P:
        P[name] = P[name][keep]
        if name in M:
            M[name] = tuple(m[keep] for m in M[name])
    tail = P["scaling"][:, 3:]
    with np.errstate(all="ignore"):
        tail[tail > fl32(0.05)] = fl32(0.05)
    out = {"params": P, "moments": M, "opacity_accum": opacity_accum[keep], "anchor_demon": anchor_demon[keep],
           "offset_gradient_accum": accum, "offset_denom": denom, "max_radii2D": np.zeros(int(keep.sum()), F32)}
    return out, levels


# ---- (c) ----

def _per_anchor_groups(optimizer):
    return [g for g in optimizer.param_groups if not any(s in g["name"] for s in SKIPPED)]


def _swap_groups(model, change):
    """Every per-anchor group gets nn.Parameter(change(old tensor)), its moments change(moment); the state moves."""
    opt = model.optimizer
    for group in _per_anchor_groups(opt):
        old = group["params"][0]
        stored = opt.state.get(old, None)
        new = torch.nn.Parameter(change(group["name"], old.detach()).requires_grad_(True))
        if stored is not None:
            stored["exp_avg"] = change(None, stored["exp_avg"])
            stored["exp_avg_sq"] = change(None, stored["exp_avg_sq"])
            del opt.state[old]
            opt.state[new] = stored
        group["params"][0] = new
        setattr(model, "_" + group["name"], new)


@torch.no_grad()
def eager_adjust(model, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, min_opacity=0.005, rand=None):
    """GM:898-952 in eager torch on the device of the model's tensors, with the level's random numbers given over the OLD
    N K offsets (``rand``; None draws them)."""
    K, dev = model.n_offsets, model._anchor.device
    N = model._anchor.shape[0]
    grads = model.offset_gradient_accum / model.offset_denom
    grads[grads.isnan()] = 0.0
    grads_norm = torch.norm(grads, dim=-1)
    offset_mask = (model.offset_denom > check_interval * success_threshold * 0.5).squeeze(dim=1)
    for i in range(model.update_depth):
        candidate = (grads_norm >= grad_threshold * ((model.update_hierachy_factor // 2) ** i)) & offset_mask
        draw = rand[i].reshape(-1) if rand is not None else torch.rand(N * K, device=dev)
        candidate = candidate & (draw > 0.5 ** (i + 1))
        now = model._anchor.shape[0]
        if now == N and i > 0:
            continue
        candidate = torch.cat([candidate, torch.zeros((now - N) * K, dtype=torch.bool, device=dev)])
        cur_size = model.voxel_size * (model.update_init_factor // (model.update_hierachy_factor ** i))
        new_anchor, new_feat = grow_level_eager(model.get_anchor, model._offset.detach(), model.get_scaling, candidate,
                                                model._anchor_feat.detach(), cur_size)
        A = new_anchor.shape[0]
        if A == 0:
            continue
        rotation = torch.zeros(A, 4, device=dev)
        rotation[:, 0] = 1.0
        tenth = 0.1 * torch.ones((A, 1), dtype=torch.float, device=dev)
        block = {"anchor": new_anchor, "scaling": torch.log(torch.ones(A, 6, device=dev) * cur_size), "rotation": rotation,
                 "anchor_feat": new_feat, "offset": torch.zeros(A, K, 3, device=dev), "mask": torch.ones(A, K, 1, device=dev),
                 "opacity": torch.log(tenth / (1 - tenth))}
        model.anchor_demon = torch.cat([model.anchor_demon, torch.zeros(A, 1, device=dev)])
        model.opacity_accum = torch.cat([model.opacity_accum, torch.zeros(A, 1, device=dev)])
        _swap_groups(model, lambda name, t: torch.cat([t, block[name] if name else torch.zeros(
            (A,) + tuple(t.shape[1:]), device=dev)]))
    grown = model._anchor.shape[0]
    pad = torch.zeros((grown - N) * K, 1, device=dev)
    model.offset_denom[offset_mask] = 0
    model.offset_denom = torch.cat([model.offset_denom, pad])
    model.offset_gradient_accum[offset_mask] = 0
    model.offset_gradient_accum = torch.cat([model.offset_gradient_accum, pad])
    prune = (model.opacity_accum < min_opacity * model.anchor_demon).squeeze(dim=1)
    anchors_mask = (model.anchor_demon > check_interval * success_threshold).squeeze(dim=1)
    prune = prune & anchors_mask
    keep = ~prune
    model.offset_denom = model.offset_denom.view(-1, K)[keep].view(-1, 1)
    model.offset_gradient_accum = model.offset_gradient_accum.view(-1, K)[keep].view(-1, 1)
    if anchors_mask.sum() > 0:
        model.opacity_accum[anchors_mask] = 0
        model.anchor_demon[anchors_mask] = 0
    model.opacity_accum = model.opacity_accum[keep]
    model.anchor_demon = model.anchor_demon[keep]
    _swap_groups(model, lambda name, t: t[keep])
    tail = model._scaling[:, 3:]
    tail[tail > 0.05] = 0.05
    model.max_radii2D = torch.zeros(model._anchor.shape[0], device=dev)


# ---- (d) ----

class Model:
    """The attributes adjust_anchor uses, over tensors of ``make_state`` moved to ``device``."""
    voxel_size, update_depth, update_init_factor, update_hierachy_factor = 0.01, 3, 16, 4

    def __init__(self, state, device, make_optimizer, mlp=True):
        self.n_offsets = state["params"]["offset"].shape[1]
        self.feat_dim = state["params"]["anchor_feat"].shape[1]
        for name in PARAMS:
            t = torch.from_numpy(state["params"][name].copy()).to(device)
            setattr(self, "_" + name, torch.nn.Parameter(t.requires_grad_(True)))
        for name in ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom"):
            setattr(self, name, torch.from_numpy(state[name].copy()).to(device))
        self.x_bound_min = torch.from_numpy(state["bound_min"].copy()).to(device)
        self.x_bound_max = torch.from_numpy(state["bound_max"].copy()).to(device)
        self.max_radii2D = torch.zeros(self._anchor.shape[0], device=device)
        groups = [{"params": [getattr(self, "_" + n)], "lr": 1e-5 * (k + 1), "name": n} for k, n in enumerate(PARAMS)]
        if mlp:
            self.mlp_w = torch.nn.Parameter(torch.ones(4, 4, device=device))
            groups.insert(3, {"params": [self.mlp_w], "lr": 0.002, "name": "mlp_opacity"})
        self.optimizer = make_optimizer(groups)

    @property
    def get_anchor(self):
        interval = (self.x_bound_max - self.x_bound_min) * (1.0 / 65535.0) + 1e-6
        q = torch.clamp(torch.div(self._anchor - self.x_bound_min, interval, rounding_mode="floor"), 0, 65535)
        return q * interval + self.x_bound_min

    @property
    def get_scaling(self):
        return 1.0 * torch.exp(self._scaling)

    def state(self):
        """The model's tensors as the numpy ``state`` of adjust_anchor_ref, and the optimizer's (names, steps)."""
        opt = self.optimizer
        moments, steps = {}, {}
        for g in opt.param_groups:
            st = opt.state.get(g["params"][0], None)
            if st and g["name"] in PARAMS:
                moments[g["name"]] = (st["exp_avg"].detach().cpu().numpy(), st["exp_avg_sq"].detach().cpu().numpy())
                steps[g["name"]] = float(st["step"])
        return {"params": {n: getattr(self, "_" + n).detach().cpu().numpy() for n in PARAMS}, "moments": moments,
                "steps": steps, "names": [g["name"] for g in opt.param_groups],
                "opacity_accum": self.opacity_accum.cpu().numpy(), "anchor_demon": self.anchor_demon.cpu().numpy(),
                "offset_gradient_accum": self.offset_gradient_accum.cpu().numpy(),
                "offset_denom": self.offset_denom.cpu().numpy(), "bound_min": self.x_bound_min.cpu().numpy(),
                "bound_max": self.x_bound_max.cpu().numpy(), "max_radii2D": self.max_radii2D.cpu().numpy()}

    def two_steps(self, seed=0, stateless=("opacity", "rotation")):
        """Two real optimizer steps with seeded gradients; the ``stateless`` groups never receive one."""
        gen = torch.Generator().manual_seed(seed)
        for _ in range(2):
            for g in self.optimizer.param_groups:
                p = g["params"][0]
                p.grad = None if g["name"] in stateless else torch.randn(p.shape, generator=gen).to(p.device) * 0.01
            self.optimizer.step()
        for g in self.optimizer.param_groups:
            g["params"][0].grad = None


def make_state(N, F, K, seed=0, grow=0.05, prune=0.05, box=4.0):
    """A seeded model state in numpy whose statistics take every branch: rows pruned, rows reset but kept, rows
    untouched, candidates of all three levels.  No g, d or s lies within 4 ulp of a threshold of the default arguments
    (the counts are integers away from 40 and 80, g is drawn from bands between the thresholds, s is a multiple of d far
    from 0.005 d)."""
    rng = np.random.default_rng(seed)
    anchor = (rng.random((N, 3)) * box).astype(F32)
    bound_min = (anchor.min(axis=0, keepdims=True) - F32(0.05) * box).astype(F32)
    bound_max = (anchor.max(axis=0, keepdims=True) + F32(0.25) * box).astype(F32)
    params = {
        "anchor": anchor,
        "offset": (rng.standard_normal((N, K, 3)) * 0.5).astype(F32),
        "mask": rng.standard_normal((N, K, 1)).astype(F32),
        "anchor_feat": rng.standard_normal((N, F)).astype(F32),
        "opacity": rng.standard_normal((N, 1)).astype(F32),
        "scaling": np.log(rng.uniform(0.05, 0.5, (N, 6))).astype(F32),    # offsets reach the neighbouring voxels
        "rotation": rng.standard_normal((N, 4)).astype(F32),
    }
    params["scaling"][:, 3:] = rng.uniform(-0.2, 0.2, (N, 3)).astype(F32)  # raw values on both sides of 0.05
    params["scaling"][::7, 4] = F32(0.05)                                  # ... and on it
    # per anchor: a third not looked at (d <= 80), the rest looked at; `prune` of all have too little opacity
    d = rng.choice(np.array([0, 13, 79, 80, 81, 100, 100, 100], F32), N).astype(F32)
    s = (d * rng.uniform(0.02, 0.9, N)).astype(F32)
    pruned = rng.random(N) < prune
    s[pruned] = (d[pruned] * F32(0.001)).astype(F32)                       # far below 0.005 d
    # per offset: counts on both sides of 40; g in bands: below t0, [t0, t1), [t1, t2), above t2
    od = rng.choice(np.array([0, 7, 39, 40, 41, 60, 100], F32), N * K).astype(F32)
    band = rng.choice(4, N * K, p=[1 - grow, grow / 2, grow / 4, grow / 4])
    lo = np.array([0.00001, 0.00025, 0.0005, 0.001], F32)[band]
    hi = np.array([0.00015, 0.00035, 0.0007, 0.01], F32)[band]
    g = (lo + (hi - lo) * rng.random(N * K)).astype(F32)
    accum = (g * od).astype(F32)
    return {"params": params, "moments": {}, "opacity_accum": s.reshape(N, 1), "anchor_demon": d.reshape(N, 1),
            "offset_gradient_accum": accum.reshape(-1, 1), "offset_denom": od.reshape(-1, 1),
            "bound_min": bound_min, "bound_max": bound_max}
