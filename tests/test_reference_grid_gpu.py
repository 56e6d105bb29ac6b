"""The hash-grid encoder (include/bloomscene_grid.h) against the reference's OWN kernels: submodules/gridencoder compiled
for gfx950 by oracle/reference_build.py and loaded by tests/reference_builds.py.  tests/test_grid_encoder_gpu.py compares
the product with tests/grid_reference.py, a restatement written from one reading of the reference; this file pins that
reading: the border exclusion, the wn_re renormalisation and its 1e-9 substitute, the dense / hashed switch, the clamp
min(pos_grid + 1, res - 1), the out-of-range rule, the corner pairing of dy_dx, and the reference's DOUBLE 0.5 in
pos = x * float(res - 2) + 0.5.

Both backends are called through the extension's argument lists (_gridencoder.grid_encode_forward / _backward here,
reference_builds.ref_grid_forward / _backward there).  The reference gets well-formed tables and zeroed grad_embeddings
only.  Skips only when build() found no reference tree (the manifest says reference_missing).
"""
import numpy as np
import pytest
import torch

import grid_reference as GR
import reference_builds as RB
import reference_cases as RC

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = "cuda:0"
U = 2.0 ** -24


def _bits_differ(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def _both(x, emb, offs, res, grad, lo=0, n=None, build="strict", with_backward=True):
    """Forward (+ backward) of levels lo .. lo + n - 1 on both backends, offsets / resolutions handed over as sliced views of
    the whole lists (BloomScene's int min_level_id) -> {"ours": {...}, "ref": {...}} of numpy arrays
    outputs [L, N, F], dy_dx [N, L, D, F], grad_embeddings [rows, F], grad_inputs [N, D]."""
    import _gridencoder as ours
    N, D = x.shape
    rows, F = emb.shape
    n = len(res) - lo if n is None else n
    xt = torch.from_numpy(x).to(DEV)
    et = torch.from_numpy(emb).to(DEV)
    ot = torch.tensor(np.asarray(offs), dtype=torch.int32, device=DEV)[lo:lo + n + 1]
    rt = torch.tensor(np.asarray(res), dtype=torch.int32, device=DEV)[lo:lo + n]
    assert int(ot[-1]) <= rows and (lo > 0 or n < len(res) or int(ot[-1]) == rows)
    gt = torch.from_numpy(np.ascontiguousarray(grad)).to(DEV) if with_backward else None
    res_out = {}
    for who in ("ours", "ref"):
        outputs = torch.full((n, N, F), 7.0, device=DEV)
        dy_dx = torch.full((N, n * D * F), 7.0, device=DEV)
        fwd = (xt, et, ot, rt, outputs, N, D, F, n, 0, 128, 0.0, dy_dx, None, None)
        if who == "ours":
            ours.grid_encode_forward(*fwd)
        else:
            RB.ref_grid_forward(*fwd, build=build)
        r = {"outputs": outputs, "dy_dx": dy_dx.view(N, n, D, F)}
        if with_backward:
            ge = torch.zeros(rows, F, device=DEV)       # the reference accumulates into it
            gi = torch.full((N, D), 7.0, device=DEV)
            bwd = (gt, xt, et, ot, rt, ge, N, D, F, n, 0, 128, dy_dx, gi, None, None)
            if who == "ours":
                ours.grid_encode_backward(*bwd)
            else:
                RB.ref_grid_backward(*bwd, build=build)
            r.update(grad_embeddings=ge, grad_inputs=gi)
        torch.cuda.synchronize()
        res_out[who] = {k: v.cpu().numpy() for k, v in r.items()}
    return res_out


def _element_stats(x, offs, res, rows, grad):
    """Per element (row, ch) of grad_embeddings: the exact (float64) sum of the fp32 contributions v_i, sum |v_i|, their
    count n, the product's documented error bound, the quantisation exponent s_l of the element's level, and whether a
    non-finite contribution reaches it."""
    L, N, F = grad.shape
    s64, ours_bound, cnt = GR.fixed_point_bound(x, offs, res, rows, grad)
    sabs = np.zeros(rows * F, np.float64)
    bad = np.zeros(rows * F, bool)
    for e, v in GR.contributions(x, offs, res, rows, grad):
        np.add.at(sabs, e, np.abs(v.astype(np.float64)))
        bad[e[~np.isfinite(v)]] = True
    s_exp = np.zeros(rows, np.int64)
    for l in range(L):
        s_exp[int(offs[l]):int(offs[l + 1])] = GR.scale_exp(GR.level_gmax_bits(grad[l]), N, x.shape[1])
    return s64, sabs.reshape(rows, F), cnt, ours_bound, s_exp, bad.reshape(rows, F)


def _check_grad_embeddings(tag, ours, ref, x, offs, res, grad):
    """grad_embeddings cannot be bit-compared: the reference adds its contributions with fp32 atomics in an order the
    hardware picks.  Per element with contributions v_1 .. v_n (fp32, GR.contributions) and exact sum s64:

      * reference: |ref - s64| <= gamma_(n-1) sum |v_i|, gamma_k = k u / (1 - k u), u = 2^-24.  The standard bound of a
        recursive fp32 sum in ANY order (Higham, Accuracy and Stability, 4.2): starting from the zeroed element, 0 + v is
        exact, each of the other n - 1 additions rounds once, and a term passes at most n - 1 of them.
      * ours: within the bound include/bloomscene_grid.h documents (0.5 ulp of the result + n 2^(-s_l - 1)).
      * n = 0: exactly 0 on both sides.
      * n = 1: the reference holds v exactly (0 + v).  Ours holds rint(v 2^s_l) 2^-s_l, the header's quantisation: they differ
        by at most HALF a quantisation step, 2^(-s_l - 1), and are bit-equal wherever v is a multiple of 2^-s_l (which is
        every v within 2^-24 .. 1 of the level's largest gradient at these N) -- both asserted.
    """
    rows, F = ours.shape
    s64, sabs, cnt, ours_bound, s_exp, bad = _element_stats(x, offs, res, rows, grad)
    assert not bad.any()
    o64, r64 = ours.astype(np.float64), ref.astype(np.float64)
    zero = cnt == 0
    assert (ours[zero] == 0).all() and (ref[zero] == 0).all()
    k = np.maximum(cnt - 1, 0)
    gamma = k * U / (1 - k * U)
    ref_err = np.abs(r64 - s64)
    assert (ref_err <= gamma * sabs).all(), (tag, float((ref_err - gamma * sabs).max()))
    assert (np.abs(o64 - s64) <= ours_bound).all(), tag
    one = cnt == 1
    step_half = np.ldexp(1.0, (-s_exp - 1).astype(np.int64))[:, None] * np.ones((1, F))
    assert (ref_err[one] == 0).all(), tag                       # (s64 of one contribution is that contribution)
    assert (np.abs(o64 - r64)[one] <= step_half[one]).all(), tag
    scaled = np.ldexp(r64, s_exp[:, None] * np.ones((1, F), np.int64))
    on_lattice = one & (scaled == np.rint(scaled))
    assert _bits_differ(ours[on_lattice], ref[on_lattice]) == 0, tag
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(k > 0, ref_err / (gamma * sabs), 0.0))) if (k > 0).any() else 0.0
    print(f"{tag}: grad_embeddings n=0: {int(zero.sum())}, n=1: {int(one.sum())} ({int(on_lattice.sum())} bit-equal, "
          f"the rest within half a step), n>1: {int((cnt > 1).sum())}; reference error / its bound max {worst:.3g}; "
          f"ours vs reference max |diff| {float(np.abs(o64 - r64).max()):.3g}")


def _check_strict(tag, both, x, offs, res, grad, lo=0, n=None):
    n = len(res) - lo if n is None else n
    o, r = both["ours"], both["ref"]
    d = {k: _bits_differ(o[k], r[k]) for k in ("outputs", "dy_dx", "grad_inputs")}
    print(f"{tag}: elements that differ from the strict reference: {d}")
    assert d == {"outputs": 0, "dy_dx": 0, "grad_inputs": 0}, (tag, d)
    _check_grad_embeddings(tag, o["grad_embeddings"], r["grad_embeddings"], x, offs[lo:lo + n + 1], res[lo:lo + n], grad)


@pytest.mark.parametrize("F", RC.GRID_FEATURES)
@pytest.mark.parametrize("D", RC.GRID_DIMS)
def test_strict_small_collision_heavy_tables(D, F):
    """Every (D, F) -- F = 4 included -- on small hashmaps, with the edge points, the k / (res - 2) lattice and its fp32
    neighbours, and tiny positive inputs down to the smallest subnormal."""
    RB.skip_if_missing()
    res, log2 = RC.SMALL_TABLES[D]
    offs, r, emb = RC.grid_table(D, F, res, log2, seed=D * 10 + F)
    N = 20_000
    x = RC.grid_points(N, D, res, seed=F)
    g = RC.grid_grad(len(res), N, F, seed=7)
    both = _both(x, emb, offs, r, g)
    _check_strict(f"grid strict D={D} F={F}", both, x, offs, r, g)
    # and the restatement itself, without the product in between
    out_ref, dy_ref = GR.forward(x, emb, offs, r)
    assert _bits_differ(both["ref"]["outputs"], out_ref) == 0 and _bits_differ(both["ref"]["dy_dx"], dy_ref) == 0


@pytest.mark.parametrize("cfg", ["3d", "2d"])
def test_strict_bloomscene_configurations_at_100k(cfg):
    RB.skip_if_missing()
    D, res, log2 = (3, RC.RES_3D, 19) if cfg == "3d" else (2, RC.RES_2D, 17)
    offs, r, emb = RC.grid_table(D, 2, res, log2, seed=5)
    N = 100_000
    x = RC.grid_points(N, D, res, seed=11)
    g = RC.grid_grad(len(res), N, 2, seed=8, sigma=1e-3)
    _check_strict(f"grid strict bloomscene {cfg}", _both(x, emb, offs, r, g), x, offs, r, g)


def test_strict_sliced_offsets_and_resolutions():
    """BloomScene's int min_level_id: both backends get views into the middle of the lists."""
    RB.skip_if_missing()
    offs, r, emb = RC.grid_table(3, 2, RC.RES_3D, 19, seed=2)
    N = 5000
    x = RC.grid_points(N, 3, RC.RES_3D, seed=3)
    for lo, n in ((0, 4), (6, 3), (10, 2), (3, 9)):
        g = RC.grid_grad(n, N, 2, seed=lo)
        both = _both(x, emb, offs, r, g, lo=lo, n=n)
        _check_strict(f"grid strict levels {lo}..{lo + n - 1}", both, x, offs, r, g, lo=lo, n=n)
        for who in ("ours", "ref"):   # rows of the levels not computed stay 0
            ge = both[who]["grad_embeddings"]
            assert (ge[:offs[lo]] == 0).all() and (ge[offs[lo + n]:] == 0).all()


def test_strict_one_inf_gradient_same_non_finite_elements():
    """One inf upstream gradient: the elements that come out non-finite are the same on both sides (NaN here, inf or NaN
    in the reference: the deviation include/bloomscene_grid.h states), every other element keeps its bounds."""
    RB.skip_if_missing()
    res, log2 = (10, 40), 10
    offs, r, emb = RC.grid_table(2, 2, res, log2, seed=1)
    N = 2000
    x = RC.grid_points(N, 2, res, seed=4)
    x[17] = (0.37, 0.61)
    g = RC.grid_grad(2, N, 2, seed=3)
    g[1, 17, 0] = np.inf
    both = _both(x, emb, offs, r, g)
    ge_o, ge_r = both["ours"]["grad_embeddings"], both["ref"]["grad_embeddings"]
    *_, bad = _element_stats(x, offs, r, emb.shape[0], g)
    assert bad.sum() >= 1
    assert np.array_equal(~np.isfinite(ge_o), bad) and np.array_equal(~np.isfinite(ge_r), bad)
    assert np.isnan(ge_o[bad]).all()
    for k in ("outputs", "dy_dx"):
        assert _bits_differ(both["ours"][k], both["ref"][k]) == 0
    gi_o, gi_r = both["ours"]["grad_inputs"], both["ref"]["grad_inputs"]
    clean = np.ones(N, bool)
    clean[17] = False
    assert _bits_differ(gi_o[clean], gi_r[clean]) == 0
    assert not np.isfinite(gi_o[17]).all() and np.array_equal(np.isfinite(gi_o[17]), np.isfinite(gi_r[17]))
    g_fin = g.copy()
    g_fin[1, 17, 0] = 0.0    # the other elements: the same bounds as without the inf (an inf contributes to `bad` only)
    s64, sabs, cnt, *_ = _element_stats(x, offs, r, emb.shape[0], g_fin)
    k = np.maximum(cnt - 1, 0)
    ok = ~bad
    assert (np.abs(ge_r.astype(np.float64) - s64)[ok] <= (k * U / (1 - k * U) * sabs)[ok]).all()


def _f64_dy_dx(x, emb, offs, res, fused_pos=False):
    """float64 evaluation of the dy_dx formula from the fp32 cell quantities of GR._cell (positions, inclusion, rows: pinned
    bit for bit by the strict tests) -> dy_dx [N, L, D, F], and the same sum with |val_right| + |val_left| (the unit of
    its rounding bound).  fused_pos: the position rounded once (GR.pos_fused), as a contracting build computes it."""
    N, D = x.shape
    rows, F = emb.shape
    L = len(res)
    dy = np.zeros((N, L, D, F))
    unit = np.zeros((N, L, D, F))
    inside = np.all((x >= 0) & (x <= 1), axis=1)
    xi = x[inside]
    e64 = emb.astype(np.float64)
    for l in range(L):
        off, hs, r = int(offs[l]), int(offs[l + 1]) - int(offs[l]), int(res[l])
        pos, ws, oks, rws, _ = GR._cell(xi, hs, r, rows - off, pos=GR.pos_fused(xi, r) if fused_pos else None)
        p64 = pos.astype(np.float64)
        val = [np.where(ok[:, None], e64[off + rw.astype(np.int64)], 0.0) for ok, rw in zip(oks, rws)]
        for gd in range(D):
            for idx in range(1 << (D - 1)):
                w = np.full(xi.shape[0], float(r - 2))
                corner = 0
                for nd in range(D - 1):
                    d = nd + 1 if nd >= gd else nd
                    if (idx >> nd) & 1:
                        w = w * p64[:, d]
                        corner |= 1 << d
                    else:
                        w = w * (1.0 - p64[:, d])
                right, left = val[corner | (1 << gd)], val[corner]
                dy[inside, l, gd] += w[:, None] * (right - left)
                unit[inside, l, gd] += w[:, None] * (np.abs(right) + np.abs(left))
    return dy, unit


@pytest.mark.parametrize("D", RC.GRID_DIMS)
def test_contract_within_rounding_of_float64(D):
    """Outputs and dy_dx of the contract build AND of the product, each against float64, with one bound for both: what
    separates the product from an nvcc-style build of the reference is rounding and nothing else.

    Unit.  outputs: T = sum_k |w_k wn_re val_k| (float64: GR.forward_f64 on |embeddings|; the weights are non-negative).
    dy_dx: T' = sum over the 2^(D-1) edges of w_edge (|val_right| + |val_left|).

    The position.  pos = x float(res - 2) + 0.5 is an fp32 quantity of the evaluation, and the two builds do not compute the
    same one.  The specification (and the product, and the strict build) rounds twice: the product, then the sum.  A
    contracting compiler narrows the reference's double 0.5 to fp32 (legal: it moves no bit, see
    tests/test_reference_goldens_cpu.py) and then fuses: `v_fma_f32 v, v, v, 0.5` in the gfx950 code of the contract build,
    `v_mul_f32` + `v_add_f32 0.5` in the strict one.  The fused pos is rounded once (GR.pos_fused, exact).  Where the two differ
    the inputs sit at the same place to within an ulp of pos, but floor() may put them in neighbouring cells (the lattice
    inputs (k + 0.5) / (res - 2), whose strict pos is an integer): dy_dx, constant per cell in its own dimension, then
    differs by whole differences of table rows, and the output by about ulp(pos) times its slope.  That is a property of
    the reference under contraction, not a rounding of the interpolation, and no bound in units of T can cover it.  So
    each side is held against the float64 twin evaluated AT ITS OWN fp32 pos (fused_pos for the contract build), with one
    and the same bound; from pos on, everything that separates the two builds is rounding.  The test also counts the
    (point, level, dimension) triples whose two positions differ, and those in different cells, and requires that the inputs
    contain some (no cell flip among the D = 3 inputs: resolutions up to 201).

    Bound for outputs, R u / (1 - R u) T with R = 4 D + 2^(D+1) - 1 (u = 2^-24), counting the roundings a term can pass in
    source order (a fused multiply-add only removes one; float64's own roundings, 2^-53 each, are covered by taking
    gamma_R = R u / (1 - R u) instead of (1 + u)^R - 1 -- see Higham 3.1: a product of R factors (1 + e_i), |e_i| <= u, is
    1 + t with |t| <= gamma_R, and the slack between the two exceeds 2^-40 relative):
      pos and its floor are taken from fp32 by the float64 twin itself, and pos - floor(pos) is exact in fp32;
      w_k: D factors (1 - pos[d]) with one rounding each and D - 1 products that round (1 * a is exact): 2 D - 1;
      wn: a sum of non-negative w: 2 D - 1 of its terms plus 2^D - 1 additions (0 + w is exact);  wn_re: 1;
      (w_k wn_re) val_k: 2;   the running sum: at most 2^D - 1 additions (0 + t is exact).
    Bound for dy_dx, R' u / (1 - R' u) T' with R' = 2 D - 1 + 2^(D-1): D - 1 factors with one rounding each, D - 1 products
    with float(res - 2), 1 for val_right - val_left (relative to |val_right| + |val_left|), 1 for the product, 2^(D-1) - 1
    additions.

    Measured on an MI355X, against the twin at the SPECIFICATION's pos on both sides (the first form of this test): the
    product 1.97 / 4.25 / 5.94 u T and 1.80 / 3.31 / 4.23 u T' for D = 1 / 2 / 3; the contract build 8190 / 1326 / 1729 u T and
    3.2e7 / 2.8e7 / 964 u T' -- the cell flips described above.
    """
    RB.skip_if_missing()
    F = 4
    res, log2 = RC.SMALL_TABLES[D]
    offs, r, emb = RC.grid_table(D, F, res, log2, seed=40 + D)
    N = 20_000
    x = RC.grid_points(N, D, res, seed=9)
    both = _both(x, emb, offs, r, None, build="contract", with_backward=False)
    xt = torch.from_numpy(x)
    R = 4 * D + 2 ** (D + 1) - 1
    R2 = 2 * D - 1 + 2 ** (D - 1)
    moved = flips = 0
    inside = np.all((x >= 0) & (x <= 1), axis=1)
    for res_l in r:
        strict = x[inside] * F32(int(res_l) - 2) + F32(0.5)
        fused = GR.pos_fused(x[inside], res_l)
        moved += int((strict != fused).sum())
        flips += int((np.floor(strict) != np.floor(fused)).sum())
    print(f"grid contract D={D}: (point, level, dimension) triples whose fused pos differs from the strict one: {moved}; "
          f"in a different cell: {flips}")
    assert moved >= 1 and (D == 3 or flips >= 1)      # (D = 3: resolutions 18 .. 201, no flip among these inputs)
    for who, fused in (("ours", False), ("ref", True)):
        f64 = GR.forward_f64(xt.double(), torch.from_numpy(emb).double(), offs, r, fused_pos=fused).numpy()
        T = GR.forward_f64(xt.double(), torch.from_numpy(np.abs(emb)).double(), offs, r, fused_pos=fused).numpy()
        dy64, T2 = _f64_dy_dx(x, emb, offs, r, fused_pos=fused)
        err = np.abs(both[who]["outputs"].astype(np.float64) - f64)
        bound = R * U / (1 - R * U) * T
        err2 = np.abs(both[who]["dy_dx"].astype(np.float64) - dy64)
        bound2 = R2 * U / (1 - R2 * U) * T2
        with np.errstate(divide="ignore", invalid="ignore"):
            w1 = float(np.nanmax(np.where(T > 0, err / (U * T), 0.0)))
            w2 = float(np.nanmax(np.where(T2 > 0, err2 / (U * T2), 0.0)))
        print(f"grid contract D={D} {who}: outputs max err {w1:.3f} u T (bound {R}), dy_dx max err {w2:.3f} u T' "
              f"(bound {R2})")
        assert (err <= bound).all(), (who, w1)
        assert (err2 <= bound2).all(), (who, w2)
    d = {k: _bits_differ(both["ours"][k], both["ref"][k]) for k in ("outputs", "dy_dx")}
    print(f"grid contract D={D}: elements where the contract build and the product differ: {d}")
