"""BSR_FLAG_EXACT_GRAD (strict_gradients=True, k_render_bwd_strict) pinned pair by pair.

The strict walk claims "the reference's per-pair operations on the reference's operands; only the ORDER of the nine
sums differs from the oracle's".  A one-hot upstream (onehot.onehot_upstream: dL/dcolour kept at ONE pixel) takes
the order out: every one of the 9 P sums then has at most one nonzero term (tests/test_onehot_oracle_cpu.py holds that
on the CPU oracle), so the claim becomes VALUE equality with the oracle, element by element, with no tolerance
(a, b).  With every pixel live the same terms pass through a summation tree whose height is read off the code (d).
The depth-gradient instantiation k_render_bwd_strict<true> runs in (b) and (c); the default walk k_render_bwd_t is
measured, not changed, under the same one-hot upstreams (e).

Every test runs inside numerics(exact_exp=True) (tests/conftest.py): the forward is the oracle's bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers as Hh
import onehot as OH
from oracle import oracle as O
from test_parity_gpu import CASES, EPS32, _dev, _native_forward, _raw_backward

pytestmark = pytest.mark.gpu

ONEHOT_CASES = {"lists_gt_1024": CASES["lists_gt_1024"],    # 48 x 48: nine dense tiles, several 128-entry batches each
                "huge_splats": CASES["huge_splats"],        # 70 x 50: ragged in x and y
                "single_pixel": CASES["single_pixel"],      # 1 x 1
                "dense_ragged": OH.DENSE_RAGGED}     # 40 x 24: dense, ragged, SH colour, bg = (1, 0.5, 0)
CULLED_ZERO = ("mean2D", "conic", "opacity", "color", "mean3D", "cov3D")


def _flags(strict):
    from bloomscene_amd.numerics import FLAG_EXACT_EXP, FLAG_EXACT_GRAD
    return FLAG_EXACT_EXP | (FLAG_EXACT_GRAD if strict else 0)


@functools.lru_cache(maxsize=None)
def _onehot_reference(name):
    """(case, oracle forward state, hot pixels, one oracle backward per hot pixel) -- computed once per case, shared by
    (a), (b) and (e) and left unchanged.  The coverage conditions are asserted here, from the oracle alone, so that no
    test built on it can pass vacuously."""
    c = Hh.make_case(**ONEHOT_CASES[name])
    st, _ = Hh.run_oracle(c, backward=False)
    pix = OH.hot_pixels(st.n_contrib, c.W, c.H)
    assert len(pix) <= 17 and (c.W - 1, c.H - 1) in pix
    refs, pairs = [], 0
    for x, y in pix:
        g = O.backward(st, OH.onehot_upstream(c.gC, x, y), c.gD, want_abs_sums=True)
        rows = int((g.dL_dcolors != 0).any(axis=1).sum())
        assert rows >= 15, (name, (x, y), rows)
        pairs += rows
        refs.append(g)
    assert pairs >= 200 or name == "single_pixel", (name, pairs)
    return c, st, pix, refs, pairs


def _assert_value_equal(got, ref, where):
    """`==` element by element (+0 and -0 are equal, a NaN equals nothing)."""
    bad = got != ref
    if bad.any():
        rows = np.nonzero(bad.any(axis=1))[0]
        i = int(rows[0])
        raise AssertionError(f"{where}: {int(bad.sum())} of {int((ref != 0).sum())} nonzero elements differ, in "
                             f"{rows.size} Gaussians, per component {bad.sum(axis=0).tolist()}; first: Gaussian {i} "
                             f"hip {got[i].tolist()} oracle {ref[i].tolist()}")


@pytest.mark.parametrize("name", list(ONEHOT_CASES))
def test_a_onehot_upstream_strict_walk_equals_the_oracle_value_for_value(name):
    """(a) One forward per case, one strict backward per hot pixel on that forward's buffers.  The nine accumulators of
    bsr_backward_ex must equal the oracle's AS VALUES for every Gaussian and every component: the hot pixel's whole
    back-to-front chain (T / (1 - alpha), accum_rec, the background term, the skip decisions, up to ~2800 list positions
    deep), the batch indexing, n_walk, the DPP sum network with 63 zero lanes, take_quadrant_sum, instance_index, the
    slab row and k_preprocess_bwd's row sum all lie between the two.  Gaussians not blended at the hot pixel get exact
    zeros.

    What this found when it was written: the background term of dL_dalpha was formed as (-T_final * bg_dot) * (1 / om),
    the reference (backward.cu:557) and the oracle form (-T_final / om) * bg_dot; in fp32 the two differ on ~40 % of
    random operands.  On the hot pixels of these four cases the library with the old form differed from the oracle on
    1315 of 19989 elements (249 of 2221 Gaussian-pixel pairs) on the MI355X, 1260 in an fp32 emulation of the pixel's
    chain; k_render_bwd_strict now forms the reference's and nothing else differed (docs/EXPERIMENTS.md)."""
    c, st, pix, refs, pairs = _onehot_reference(name)
    rs, t, R, color, depth, radii, gb, bb, ib = _native_forward(c)
    assert R == st.num_rendered
    vis = st.radii > 0
    print(f"[onehot] {name}: {len(pix)} hot pixels, {pairs} (Gaussian, pixel) pairs")
    for (x, y), g in zip(pix, refs):
        out, _ = _raw_backward(c, rs, t, R, radii, gb, bb, ib, OH.onehot_upstream(c.gC, x, y), c.gD, flags=_flags(True))
        _assert_value_equal(OH.nine_sums_hip(out), OH.nine_sums(g), f"{name} hot pixel {(x, y)}")
        assert not out["mean2D"][:, 2].any() and not out["conic"][:, 2].any()
        for k in CULLED_ZERO:
            assert not out[k][~vis].any(), (k, (x, y))


def _raw_backward_depth(c, rs, t, R, radii, gb, bb, ib, gC, gD, flags, out_depth):
    """bsr_backward_ex with out_depth given (the depth-gradient extension: k_render_bwd_strict<true> under
    BSR_FLAG_EXACT_GRAD), written out here because test_parity_gpu._raw_backward passes NULL there.  Same outputs,
    NaN-filled before the call: it must overwrite every element."""
    from bloomscene_amd import _capi
    dev = _dev()
    P = c.P
    M = 0 if c.shs is None else c.shs.shape[1]
    shapes = dict(mean2D=(P, 3), conic=(P, 4), opacity=(P, 1), color=(P, 3), mean3D=(P, 3), cov3D=(P, 6),
                  sh=(P, max(M, 1), 3), scale=(P, 3), rot=(P, 4))
    out = {k: torch.full(s, float("nan"), device=dev, dtype=torch.float32) for k, s in shapes.items()}

    def p(x):
        return None if x is None or x.numel() == 0 else x.data_ptr()
    gC, gD, out_depth = gC.to(dev).contiguous(), gD.to(dev).contiguous(), out_depth.to(dev).contiguous()
    rc = _capi.lib().bsr_backward_ex(
        P, c.deg, M, R, rs.bg.data_ptr(), c.W, c.H, t["means3D"].data_ptr(), p(t["shs"]), p(t["colors"]),
        p(t["scales"]), float(rs.scale_modifier), p(t["rot"]), p(t["cov"]), rs.viewmatrix.data_ptr(),
        rs.projmatrix.data_ptr(), rs.campos.data_ptr(), float(rs.tanfovx), float(rs.tanfovy), radii.data_ptr(),
        gb.data_ptr(), p(bb), ib.data_ptr(), out_depth.data_ptr(), gC.data_ptr(), gD.data_ptr(),
        out["mean2D"].data_ptr(), out["conic"].data_ptr(), out["opacity"].data_ptr(), out["color"].data_ptr(),
        out["mean3D"].data_ptr(), out["cov3D"].data_ptr(), out["sh"].data_ptr() if M else None, out["scale"].data_ptr(),
        out["rot"].data_ptr(), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream), int(flags))
    _capi.check(rc, "bsr_backward_ex")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, M


@pytest.mark.parametrize("name", ["lists_gt_1024", "dense_ragged"])
def test_b_onehot_upstream_depth_instantiation_with_zero_depth_upstream(name):
    """(b) k_render_bwd_strict<true> (out_depth given: ten-float slab rows, a fourth recurrence channel) with dL/ddepth
    all zeros: gz = 0, g1 = -+0, d_i = 0 and every depth term is +-0, so the nine accumulators must be value-equal to
    (a)'s oracle.  The tenth sum (dL/dz) is not an output of the ABI: it enters dL_dmean3D as vm[2,6,10] * dL_dz, which
    must therefore add exactly 0 -- every output of the call equals the DEPTH = false call's as values."""
    c, st, pix, refs, _ = _onehot_reference(name)
    rs, t, R, color, depth, radii, gb, bb, ib = _native_forward(c)
    np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), st.depth.view(np.uint32))
    gD0 = torch.zeros_like(c.gD)
    for (x, y), g in zip(pix, refs):
        gC = OH.onehot_upstream(c.gC, x, y)
        out, _ = _raw_backward_depth(c, rs, t, R, radii, gb, bb, ib, gC, gD0, _flags(True), depth)
        _assert_value_equal(OH.nine_sums_hip(out), OH.nine_sums(g), f"{name} hot pixel {(x, y)} (depth instantiation)")
        assert not out["mean2D"][:, 2].any() and not out["conic"][:, 2].any()
        plain, _ = _raw_backward(c, rs, t, R, radii, gb, bb, ib, gC, gD0, flags=_flags(True))
        for k in out:   # (both cases have SH colour and scale + rotation inputs: every output is written)
            assert (out[k] == plain[k]).all(), (k, (x, y))


@pytest.mark.parametrize("name", ["sh3", "precomp_color", "precomp_cov", "shell_view", "free_camera_sh3", "lists_gt_1024"])
def test_c_strict_walk_with_a_live_depth_upstream(name):
    """(c) GaussianRasterizer(depth_gradient=True, strict_gradients=True) against the oracle's extension, at
    test_depth_gradient_extension's own bar: every gradient finite and within 1e-5 of its tensor's scale.

    Bit-equality is NOT asked here: the oracle's depth pass advances Rd += alpha * (d - Rd), the kernel advances
    last_alpha * last + (1 - last_alpha) * acc (the colour channels' recurrence), and the extension is pinned by float64
    autograd (tests/test_oracle_crosscheck.py), not by the reference."""
    c = Hh.make_case(**CASES[name])
    st, g = Hh.run_oracle(c, depth_gradient=True)
    out = Hh.run_hip(c, depth_gradient=True, strict_gradients=True)
    np.testing.assert_array_equal(out.color.view(np.uint32), st.color.view(np.uint32))
    np.testing.assert_array_equal(out.depth.view(np.uint32), st.depth.view(np.uint32))
    og = Hh.oracle_grads(c, g)
    for k in Hh.GRAD_KEYS:
        ref, got = getattr(og, k), getattr(out.grads, k)
        if ref is None:
            assert got is None, k
            continue
        assert np.isfinite(got).all(), k
        e = Hh.max_err_over_scale(got, ref)
        print(f"[strict+depth] {name:18s} dL_d{k:14s} norm-wise {e:.2e}")
        assert e < 1e-5, (k, e)


STRICT_SMALL = ["sh3", "sh1_near_ragged", "precomp_color", "precomp_cov", "extraM_scalemod_bg", "shell_view",
                "lists_gt_1024", "lists_gt_8192", "free_camera_sh3", "free_camera_precomp_cov", "huge_splats",
                "single_pixel", "one_gaussian", "M16_D1", "M4_D0"]


@pytest.mark.parametrize("name", STRICT_SMALL)
def test_d_strict_walk_all_terms_live_within_the_summation_tree_bound(name):
    """(d) The strict walk at the shapes where the default walk is pinned, every pixel live.

    Stage A, per element, against the oracle's binary64 sums.  By (a) the per-pair terms are the oracle's fp32 terms, so
    only additions lie between the two.  A term of Gaussian i passes through at most h_i fp32 additions:
      * 6 in the wave's halving reduction (csrc/bwd_sums.h, wave_sums_masked: one add per lane bit -- row_ror:4,
        row_ror:8, permlane16 swap + add, permlane32 swap + add, quad_perm [1,0,3,2], quad_perm [2,3,0,1]);
      * 3 in take_quadrant_sum (csrc/render_bwd_common.h: ((p0 + p1) + p2) + p3);
      * K_i - 1 in k_preprocess_bwd's in-order row sum (csrc/preprocess_bwd.hip: g[k] += row[k] over the Gaussian's
        rows, starting from 0; the first add is exact), K_i = the entries of i in the oracle's point_list -- the HIP
        lists are sub-sequences of it, so the Gaussian has at most K_i slab rows.
    With u = 2^-24, S_i = the oracle's sum |term| (abs_sums, itself rounded to fp32: the factor 1 + u) and h_i = K_i + 8:
        |hip - oracle| <= ((1 + u)^h_i - 1) S_i (1 + u)  +  u |oracle|  +  256 K_i 2^-53 S_i
    = an fp32 sum over an addition tree of height h_i (zero addends add no error), the oracle's single rounding to
    fp32, and the oracle's binary64 accumulation of at most 256 K_i terms.  No relative and no norm-wise term.

    Stage B exactly as test_backward_stagewise_vs_oracle: the oracle's per-Gaussian chain fed with the HIP accumulators
    reproduces the HIP outputs to 1e-6 of each tensor's scale and 1e-4 elementwise."""
    c = Hh.make_case(**CASES[name])
    st, g = Hh.run_oracle(c, want_abs_sums=True)
    rs, t, R, color, depth, radii, gb, bb, ib = _native_forward(c)
    assert R == st.num_rendered
    np.testing.assert_array_equal(color.cpu().numpy().view(np.uint32), st.color.view(np.uint32))
    out, M = _raw_backward(c, rs, t, R, radii, gb, bb, ib, c.gC, c.gD, flags=_flags(True))

    u = 2.0 ** -24
    K = np.bincount(st.point_list, minlength=c.P).astype(np.float64)[:, None]
    S = g.abs_sums.astype(np.float64)
    ref = OH.nine_sums(g).astype(np.float64)
    got = OH.nine_sums_hip(out).astype(np.float64)
    bound = np.expm1((K + 8.0) * np.log1p(u)) * S * (1.0 + u) + u * np.abs(ref) + 256.0 * K * 2.0 ** -53 * S
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"[strict-tree] {name:24s} max err / bound {worst:.3f}; elements off {int((err > bound).sum())} of {err.size}")
    assert (err <= bound).all(), (name, worst, int((err > bound).sum()), (err > bound).sum(axis=0).tolist())
    assert not out["mean2D"][:, 2].any()
    assert not out["conic"][:, 2].any()

    h = O.empty_grads(st)
    h.dL_dmeans2D[:] = out["mean2D"]
    h.dL_dconic[:] = out["conic"].reshape(-1, 2, 2)
    h.dL_dopacity[:] = out["opacity"]
    h.dL_dcolors[:] = out["color"]
    O.backward_chain(st, h)
    chain = [("mean3D", h.dL_dmeans3D), ("cov3D", h.dL_dcov3D)]
    if M:
        chain.append(("sh", h.dL_dsh))
    if c.scales is not None:
        chain += [("scale", h.dL_dscales), ("rot", h.dL_drotations)]
    for k, r in chain:
        a = out[k].reshape(r.shape)
        assert np.isfinite(a).all(), k
        assert Hh.max_err_over_scale(a, r) < 1e-6, k
        m, _ = Hh.rel_err(a, r)
        assert m < 1e-4, (k, m)
    vis = st.radii > 0
    for k in CULLED_ZERO:
        assert not out[k][~vis].any(), k


@pytest.mark.parametrize("name", list(ONEHOT_CASES))
def test_e_default_walk_under_the_onehot_upstreams(name):
    """(e) k_render_bwd_t (flags = BSR_FLAG_EXACT_EXP only) under (a)'s upstreams: the project's stage-A bound of
    test_backward_stagewise_vs_oracle, in which S = |oracle| now that every sum has one term.  Printed, not asserted:
    the default walk's largest relative per-pair error with no summation order mixed in, and beside it the same figure
    for the reference built with fp contraction (onehot.contracted_oracle_nine_sums) -- docs/EXPERIMENTS.md."""
    c, st, pix, refs, _ = _onehot_reference(name)
    ups = [OH.onehot_upstream(c.gC, x, y) for x, y in pix]
    contracted = OH.contracted_oracle_nine_sums(c, ups)
    assert contracted is not None, "oracle/libbsr_oracle_fma.so missing and not buildable (make -C oracle fma)"
    rs, t, R, color, depth, radii, gb, bb, ib = _native_forward(c)
    worst_hip = worst_fma = 0.0
    for gC, g, con in zip(ups, refs, contracted):
        out, _ = _raw_backward(c, rs, t, R, radii, gb, bb, ib, gC, c.gD, flags=_flags(False))
        ref = OH.nine_sums(g).astype(np.float64)
        got = OH.nine_sums_hip(out).astype(np.float64)
        S = g.abs_sums.astype(np.float64)
        err = np.abs(got - ref)
        nz = ref != 0
        worst_hip = max(worst_hip, float((err[nz] / np.abs(ref[nz])).max()))
        worst_fma = max(worst_fma, float((np.abs(con.astype(np.float64) - ref)[nz] / np.abs(ref[nz])).max()))
        bound = 1e-4 * np.abs(ref) + 256 * EPS32 * S + 1e-6 * np.abs(ref).max(axis=0, keepdims=True) + 1e-30
        assert (err <= bound).all(), (name, float((err / bound).max()))
    print(f"[onehot-default] {name:14s} largest relative per-pair error: default walk {worst_hip:.2e}, "
          f"contracted reference {worst_fma:.2e}")
