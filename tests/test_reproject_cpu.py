"""The reprojection's numpy restatement (tests/reproject_reference.py) against scipy / numpy, on the host.

The goldens ``tests/golden/reproject/reproject_*.npz`` hold what scipy computed where ``BloomScene.generate_pcd`` calls it
(``tools/make_reproject_goldens.py`` wrote them); the GPU tests then pin the kernels to the restatement bit for bit.
"""
import glob
import os

import numpy as np
import pytest

import reproject_reference as RR
from bloomscene_amd import _capi, reproject  # noqa: F401  (the feature: without it this file fails at import)

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reproject", "reproject_*.npz")))
NAMES = [os.path.basename(p)[len("reproject_"):-len(".npz")] for p in GOLDEN]

_cache = {}


def warped(path, tol):
    """The restatement on a golden case, computed once per (case, tolerance) and shared."""
    if (path, tol) not in _cache:
        g = np.load(path)
        w = RR.warp_points(g["points"], g["colors"], g["K"], g["R"], g["T"], int(g["H"]), int(g["W"]), tol)
        _cache[(path, tol)] = (g, w)
    return _cache[(path, tol)]


def interior(mask):
    """mask == 1 without the border ring of 2, which step 6 rewrites."""
    m = mask == 1
    m[:RR.RING] = m[-RR.RING:] = False
    m[:, :RR.RING] = m[:, -RR.RING:] = False
    return m


def test_goldens_are_the_documented_set():
    assert len(GOLDEN) == 6 and sum(n.startswith("smooth") for n in NAMES) == 4
    for p in GOLDEN:
        g = np.load(p)
        assert int(g["H"]) <= 64 and int(g["W"]) <= 64 and os.path.getsize(p) < 300_000
        assert g["colors"].shape[0] % 256 != 0


@pytest.mark.parametrize("path", GOLDEN, ids=NAMES)
@pytest.mark.parametrize("tol", [0.05, None])
def test_discrete_outputs_are_exactly_the_reference_s(path, tol):
    g, w = warped(path, tol)
    W = int(g["W"])
    valid = np.nonzero(w.pixel >= 0)[0]
    assert np.array_equal(valid, g["valid_idx"])
    assert np.array_equal(w.pixel[valid], g["round_coord"][1] * W + g["round_coord"][0])
    assert (w.pixel[w.pixel < 0] == -1).all()
    for name in ("hit", "known", "mask", "mask_hf"):
        assert np.array_equal(getattr(w, name), g[name]), name
    assert w.image.dtype == np.float32 and w.depth.dtype == np.float32 and w.pixel.dtype == np.int32
    assert (w.image[w.mask == 0] == 0).all()


@pytest.mark.parametrize("path", [p for p, n in zip(GOLDEN, NAMES) if n.startswith("smooth")],
                         ids=[n for n in NAMES if n.startswith("smooth")])
def test_smooth_fixture_is_nearer_to_griddata_linear_than_griddata_nearest_is(path):
    """mean |image - linear| over mask == 1 without the ring  <=  the same mean of scipy's own method='nearest'.
    Measured (docs/EXPERIMENTS.md): 0.0033 / 0.0047 on the two 64 x 64 cases, 0.0042 / 0.0060 at 40 x 48,
    0.0093 / 0.0115 at 17 x 33."""
    g, w = warped(path, 0.05)
    m = interior(g["mask"])
    assert m.sum() > 100
    ours = float(np.abs(w.image - g["linear"])[m].mean())
    nearest = float(np.abs(g["nearest"] - g["linear"])[m].mean())
    print(f"{os.path.basename(path)}: ours {ours:.4f}, griddata nearest {nearest:.4f}")
    assert ours <= nearest


def test_a_smooth_scene_has_no_occlusion_to_test():
    """On the single-surface fixture the visibility test changes next to nothing: the two settings agree within the
    difference between griddata's two methods."""
    g, w = warped(GOLDEN[NAMES.index("smooth_64x64_yaw_p5")], 0.05)
    _, w0 = warped(GOLDEN[NAMES.index("smooth_64x64_yaw_p5")], None)
    m = interior(g["mask"])
    assert float(np.abs(w.image - w0.image)[m].mean()) < float(np.abs(g["nearest"] - g["linear"])[m].mean())


def test_window_filters_equal_scipy_s_on_random_masks():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    for H, W, p in ((17, 33, 0.02), (40, 48, 0.01), (5, 4, 0.2), (3, 3, 0.5)):
        hit = (rng.random((H, W)) < p).astype(np.uint8)
        known = RR.window_max(hit, RR.FILL_RADIUS)
        assert np.array_equal(known, ndi.maximum_filter(hit, size=(9, 9)))
        assert np.array_equal(RR.window_min(known, RR.ERODE_RADIUS), ndi.minimum_filter(known, size=(11, 11)))


def test_half_integers_round_to_even_and_the_frame_edge_is_valid():
    K = np.eye(3)
    R, T = np.eye(3), np.zeros(3)
    H, W = 6, 8
    uv = np.array([[0.5, 0.5], [1.5, 2.5], [2.5, 3.5], [0.0, 0.0], [7.0, 5.0], [7.00001, 2.0], [3.0, 5.00001], [-0.00001, 1.0]])
    pts = np.stack([uv[:, 0], uv[:, 1], np.ones(len(uv))]).astype(np.float32)   # z = 1: u = x, v = y
    w = RR.warp_points(pts, np.full((len(uv), 3), 0.5, np.float32), K, R, T, H, W)
    assert w.pixel.tolist() == [0 * W + 0, 2 * W + 2, 4 * W + 2, 0, 5 * W + 7, -1, -1, -1]


def test_invalid_points_leave_no_trace():
    K, R, T = np.eye(3), np.eye(3), np.zeros(3)
    pts = np.array([[2, 2, 1], [2, 2, 0], [2, 2, -1], [np.nan, 2, 1], [3, 3, 1], [4, 4, 1]], np.float32)
    col = np.full((6, 3), 0.25, np.float32)
    col[4, 1] = np.nan
    col[5, 2] = np.inf
    w = RR.warp_points(pts, col, K, R, T, 8, 8)
    assert w.pixel.tolist() == [2 * 8 + 2, -1, -1, -1, -1, -1]
    assert w.hit.sum() == 1 and np.isfinite(w.image).all() and np.isfinite(w.depth).all()


def test_fill_runs_and_never_reads_a_filled_value():
    """A sparse cloud: known pixels that no footprint reaches take the weighted mean of the resolved ones around them."""
    K, R, T = np.eye(3), np.eye(3), np.zeros(3)
    pts = np.array([[4, 4, 2], [8, 4, 2]], np.float32) * np.array([2, 2, 1], np.float32)   # u = x / z
    col = np.array([[1, 0, 0], [0, 0, 1]], np.float32)
    w = RR.warp_points(pts, col, K, R, T, 12, 16)
    assert w.resolved.sum() == 2 and ((w.known == 1) & ~w.resolved).sum() > 50
    # midway between the two points both weigh the same
    assert (w.depth[(w.known == 1)] == 2.0).all() and (w.depth[1:-1, 1:-1][w.known[1:-1, 1:-1] == 0] == 0).all()
    # the erosion's window is clipped at the frame too: the corner in front of the two points stays in the mask
    assert w.mask.sum() == 32 and (w.mask[:4, :8] == 1).all()
    assert w.image[0, 0].tolist() == [1, 0, 0]          # the ring shows (1, 1), whose window holds the first point alone
    assert w.image[3, 6].tolist() == [0.5, 0, 0.5]      # both points at squared distance 5
    assert (w.image[w.mask == 0] == 0).all()


MEASURED_LIFT_ULP = 4.5e-10   # in units of the last place of a point's largest coordinate (the test below has the account)


def test_lift_pixels_against_the_reference_lines_in_numpy():
    """BS:470-471 with numpy's matmul / dot (BLAS) against the restatement's source-order sums.  Measured on this
    fixture: 4.5e-10 units in the last place of a point's largest coordinate.  The summation orders differ in the last
    bits of an fp64 value; no rounding to fp32 of the 12288 values fell on the other side, and all that differs is the
    residue of a cancellation (a coordinate that is 0 in one order and about 1e-16 in the other).  The bound is twice
    the measured value."""
    g = np.load(GOLDEN[NAMES.index("smooth_64x64_yaw_p5")])
    H, W, K, R, T = int(g["H"]), int(g["W"]), g["K"], g["R"], g["T"]
    rng = np.random.default_rng(3)
    depth = (2.0 + 0.3 * rng.random((H, W))).astype(np.float32)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    # the reference's arithmetic: fp32 products with the pixel coordinates, then float64 matrix products (BLAS),
    # R^-1 applied to the points and to T separately
    cols, rows = np.arange(W, dtype=np.float32)[None, :], np.arange(H, dtype=np.float32)[:, None]
    homogeneous = np.stack([cols * depth, rows * depth, depth]).reshape(3, H * W)
    Rinv = np.linalg.inv(R)
    want = (Rinv @ (np.linalg.inv(K) @ homogeneous) - Rinv @ T.reshape(3, 1)).astype(np.float32)
    pts, col = RR.lift_pixels(depth, image, K, R, T)
    assert pts.shape == (H * W, 3) and pts.dtype == np.float32
    # (a point's unit: the last place of its largest coordinate -- a coordinate near 0 is a difference of such values)
    ulp = np.abs(pts - want.T) / np.spacing(np.abs(want.T).max(axis=1, keepdims=True))
    print(f"lift_pixels: largest difference {ulp.max():.3g} ulp")
    assert ulp.max() <= 2 * MEASURED_LIFT_ULP
    assert np.array_equal(col, image.reshape(-1, 3).astype(np.float32) / 255.)
    # a selection comes out in np.where's order
    sel = rng.random((H, W)) < 0.3
    ps, cs = RR.lift_pixels(depth, image, K, R, T, sel)
    idx = np.where(sel.reshape(-1))[0]
    assert np.array_equal(ps, pts[idx]) and np.array_equal(cs, col[idx])



def test_lifted_points_project_back_onto_their_pixels():
    g = np.load(GOLDEN[NAMES.index("smooth_40x48_yaw_m5")])
    H, W, K, R, T = int(g["H"]), int(g["W"]), g["K"], g["R"], g["T"]
    depth = np.full((H, W), 1.75, np.float32)
    pts, _ = RR.lift_pixels(depth, np.zeros((H, W, 3), np.float32), K, R, T)
    u, v, z = RR.project(pts.T, K, R, T)
    assert np.abs(u.reshape(H, W) - np.arange(W)).max() < 1e-4 and np.abs(v.reshape(H, W) - np.arange(H)[:, None]).max() < 1e-4
    assert np.abs(z - 1.75).max() < 1e-5


def test_signatures_and_header_agree_on_the_new_entry_points():
    names = {"bsr_reproject_scratch_bytes", "bsr_warp_points", "bsr_lift_scratch_bytes", "bsr_lift_count", "bsr_lift_pixels"}
    assert names <= set(_capi.SIGNATURES)
    hdr = open(os.path.join(os.path.dirname(_capi.CSRC), "..", "include", "bloomscene_reproject.h")).read()
    assert all(n + "(" in hdr for n in names)
    lib = _capi.lib()
    assert lib.bsr_reproject_scratch_bytes(512, 512) == 512 * 512 * 45
    assert lib.bsr_reproject_scratch_bytes(2, 512) == 0 and lib.bsr_reproject_scratch_bytes(65536, 32768) == 0
    assert lib.bsr_lift_scratch_bytes(512, 512) == 4096 and lib.bsr_lift_scratch_bytes(0, 4) == 0


def test_error_order_needs_no_gpu():
    """dtype TypeError, then NotImplementedError, then shapes ValueError, the device last (bloomscene_amd/_operands.py)."""
    import torch
    K, R, T = np.eye(3), np.eye(3), np.zeros(3)
    pts, col = torch.zeros(5, 3), torch.zeros(5, 3)
    with pytest.raises(TypeError, match="points must be float32"):
        reproject.warp_points(pts.double().requires_grad_(), col[:4], K, R, T, 2, 2)
    with pytest.raises(TypeError, match="K must be a host array"):
        reproject.warp_points(pts.clone().requires_grad_(), col[:4], "camera", R, T, 2, 2)
    with pytest.raises(NotImplementedError, match="no gradient"):
        reproject.warp_points(pts.clone().requires_grad_(), col[:4], K, R, T, 2, 2)
    with pytest.raises(ValueError, match=r"points must be \[4, 3\] or \[3, 4\]"):
        reproject.warp_points(pts, col[:4], K, R, T, 8, 8)
    for bad in ({"K": np.eye(4)}, {"T": np.zeros(4)}, {"H": 2}, {"W": 65536, "H": 32768}, {"z_tolerance": -0.1},
                {"z_tolerance": float("nan")}):
        kw = dict(K=K, R=R, T=T, H=8, W=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            reproject.warp_points(pts, col, **kw)
    with pytest.raises(ValueError, match="must be on the GPU"):
        reproject.warp_points(pts, col, K, R, T, 8, 8)
    depth, image = torch.zeros(4, 6), torch.zeros(4, 6, 3)
    with pytest.raises(TypeError, match="image must be float32 or uint8"):
        reproject.lift_pixels(depth, image.half(), K, R, T)
    with pytest.raises(TypeError, match="select must be bool or uint8"):
        reproject.lift_pixels(depth, image, K, R, T, select=torch.zeros(4, 6))
    with pytest.raises(NotImplementedError):
        reproject.lift_pixels(depth.clone().requires_grad_(), image[:3], K, R, T)
    with pytest.raises(ValueError, match=r"image must be \[4, 6, 3\]"):
        reproject.lift_pixels(depth, image[:3], K, R, T)
    with pytest.raises(ValueError, match="invertible"):
        reproject.lift_pixels(depth, image, np.zeros((3, 3)), R, T)
    with pytest.raises(ValueError, match="must be on the GPU"):
        reproject.lift_pixels(depth, image.to(torch.uint8), K, R, T, select=torch.ones(4, 6, dtype=torch.bool))
