"""``bloomscene_amd.reproject`` on the GPU: every output bit-equal to tests/reproject_reference.py.

Frames of 48 x 40 and 33 x 17 (neither a multiple of the 32 x 16 tile, the first more than one tile each way), point
counts that are no multiple of 256.  Reads no scipy and nothing outside the repository: scipy's part is in the goldens.
"""
import glob
import os

import numpy as np
import pytest
import torch

import reproject_reference as RR
from bloomscene_amd.reproject import lift_pixels, warp_points

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reproject", "reproject_*.npz")))
NAMES = [os.path.basename(p)[len("reproject_"):-len(".npz")] for p in GOLDEN]
OUTPUTS = ("image", "depth", "mask", "mask_hf", "pixel")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run(points, colors, K, R, T, H, W, tol=0.05):
    got = warp_points(torch.from_numpy(np.ascontiguousarray(points)).to(DEV), torch.from_numpy(colors).to(DEV), K, R, T, H, W, tol)
    return {k: getattr(got, k).cpu().numpy() for k in OUTPUTS}


def assert_equals_restatement(points, colors, K, R, T, H, W, tol=0.05, got=None):
    """-> the restatement's result, after every output of the kernels was compared with it bit for bit."""
    want = RR.warp_points(points, colors, K, R, T, H, W, tol)
    got = got or run(points, colors, K, R, T, H, W, tol)
    for k in OUTPUTS:
        w = getattr(want, k)
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
        differ = bits(got[k]) != bits(w)
        assert not differ.any(), f"{k}: {int(differ.sum())} of {differ.size} differ, first at {np.argwhere(differ)[0].tolist()}"
    return want


def camera(H, W):
    return np.array([[1.1 * W, 0, W / 2], [0, 1.1 * W, H / 2], [0, 0, 1]], dtype=np.float64)


def surface(H, W, P, seed, depth=2.0, spread=1.0):
    """P points of a wavy surface that covers the frame of the identity camera `spread` times, with smooth colours."""
    rng = np.random.default_rng(seed)
    K = camera(H, W)
    px = rng.uniform((0.5 - spread / 2) * W, (0.5 + spread / 2) * W, P)
    py = rng.uniform((0.5 - spread / 2) * H, (0.5 + spread / 2) * H, P)
    d = depth + 0.2 * np.sin(3 * px / W) * np.cos(2 * py / H)
    pts = (np.linalg.inv(K) @ np.stack([px * d, py * d, d])).astype(F32)
    col = np.stack([0.5 + 0.4 * np.sin(3 * px / W), 0.5 + 0.4 * np.cos(2 * py / H), px / W * 0.0 + 0.3], axis=1).astype(F32)
    return pts, col, K


def yaw(deg, d=2.0):
    a = np.deg2rad(deg)
    R = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])
    return R, np.array([d * np.sin(a), 0.0, d - d * np.cos(a)])


EYE = (np.eye(3), np.zeros(3))


@pytest.mark.parametrize("path", GOLDEN, ids=NAMES)
@pytest.mark.parametrize("tol", [0.05, None])
def test_golden_cases(path, tol):
    g = np.load(path)
    want = assert_equals_restatement(g["points"], g["colors"], g["K"], g["R"], g["T"], int(g["H"]), int(g["W"]), tol)
    # ... and with that scipy's / numpy's discrete results
    assert np.array_equal(np.nonzero(want.pixel >= 0)[0], g["valid_idx"])
    assert np.array_equal(want.mask, g["mask"]) and np.array_equal(want.mask_hf, g["mask_hf"])


@pytest.mark.parametrize("H,W,P", [(40, 48, 3001), (17, 33, 777)])
@pytest.mark.parametrize("tol", [0.05, None])
def test_two_layers(H, W, P, tol):
    far, cf, K = surface(H, W, P, 1, depth=3.0, spread=1.3)
    near, cn, _ = surface(H, W, P // 3, 2, depth=1.4, spread=0.5)
    pts, col = np.concatenate([far, near], axis=1), np.concatenate([cf, 1 - cn])
    R, T = yaw(5, 2.0)
    want = assert_equals_restatement(pts, col, K, R, T, H, W, tol)
    if tol is not None:   # the near layer hides the far one where it lies: the depth there is the near layer's
        assert float(np.median(want.depth[H // 2 - 2:H // 2 + 2, W // 2 - 2:W // 2 + 2])) < 1.7


@pytest.mark.parametrize("H,W,P", [(40, 48, 1501), (17, 33, 301)])
def test_a_camera_moved_towards_the_surface_makes_the_fill_run(H, W, P):
    pts, col, K = surface(H, W, P, 16, spread=1.0)
    R, T = np.eye(3), np.array([0.0, 0.0, -1.2])   # 2.0 -> 0.8 away: the cloud thins out to a point per 6 pixels
    want = assert_equals_restatement(pts, col, K, R, T, H, W)
    filled = (want.known == 1) & ~want.resolved
    assert filled.sum() > H * W // 10
    assert filled[:3, :3].any() and filled[-3:, -3:].any()      # clipped windows, and the ring's shifted ones
    assert want.mask.any() and (want.depth[filled] > 0).all()


def test_half_integer_coordinates_round_to_even():
    H, W = 17, 33
    K = np.eye(3)
    gx, gy = np.meshgrid(np.arange(W - 1) + 0.5, np.arange(H - 1) + 0.5)
    u, v = np.concatenate([gx.ravel(), gx.ravel()[:40]]), np.concatenate([gy.ravel(), np.arange(40) % H * 1.0])
    z = 1.0 + (np.arange(len(u)) % 7) * 0.5                       # (u z and v z are exact in fp32: quarters)
    pts = np.stack([u * z, v * z, z]).astype(F32)
    col = np.random.default_rng(4).random((len(u), 3)).astype(F32)
    want = assert_equals_restatement(pts, col, K, *EYE, H, W)
    assert np.array_equal(want.pixel[:3], [0, 2, 2]) and want.pixel[W - 1] == 2 * W   # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2; v = 1.5 -> 2
    assert len(u) % 256 != 0


def test_frame_edges_and_invalid_points():
    H, W = 40, 48
    K = np.eye(3)
    uvz = [(0, 5, 1), (W - 1, 7, 2), (9, H - 1, 1), (0, 0, 1), (W - 1, H - 1, 4), (W - 1, 0, 1),   # on the edges: valid
           (np.nextafter(F32(W - 1), F32(W)), 3, 1), (4, np.nextafter(F32(H - 1), F32(H)), 1), (-1e-3, 4, 1),  # just outside
           (5, 5, 0), (5, 5, -1), (6, 6, -0.0),                                                   # z <= 0
           (np.nan, 5, 1), (5, np.nan, 1), (5, 5, np.nan), (np.inf, 5, 1), (5, 5, np.inf)]        # non-finite
    pts = np.array([(u * z, v * z, z) for u, v, z in uvz], dtype=F32).T
    pts = np.concatenate([pts, np.array([[20.25, 21.5, 22.75, 23], [10.5, 10.25, 10, 10], [1, 1, 1, 1]], F32)], axis=1)
    col = np.full((pts.shape[1], 3), 0.5, F32)
    col[-3, 0], col[-2, 1], col[-1, 2] = np.nan, np.inf, -np.inf    # NaN / infinite colours: invalid, no trace
    with np.errstate(invalid="ignore"):
        want = assert_equals_restatement(pts, col, K, *EYE, H, W)
    assert (want.pixel[:6] >= 0).all() and (want.pixel[6:17] == -1).all()
    assert want.pixel[17] >= 0 and (want.pixel[18:] == -1).all()
    assert want.pixel[4] == H * W - 1 and np.isfinite(want.image).all() and np.isfinite(want.depth).all()


def test_three_thousand_points_on_one_pixel_twice():
    H, W, P = 17, 33, 3000
    rng = np.random.default_rng(5)
    u, v = 20 + rng.uniform(-0.45, 0.45, P), 9 + rng.uniform(-0.45, 0.45, P)
    z = 2.0 + rng.uniform(0, 0.09, P)
    K = camera(H, W)
    pts = (np.linalg.inv(K) @ np.stack([u * z, v * z, z])).astype(F32)
    col = rng.random((P, 3)).astype(F32)
    a, b = run(pts, col, K, *EYE, H, W), run(pts, col, K, *EYE, H, W)
    for k in OUTPUTS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    want = assert_equals_restatement(pts, col, K, *EYE, H, W, got=a)
    assert (want.pixel == 9 * W + 20).all() and want.resolved.sum() == 9


def test_a_region_no_point_reaches():
    H, W = 40, 48
    pts, col, K = surface(H, W, 1201, 6, spread=1.0)
    keep = pts[0] / pts[2] < 0.0                                   # the left half of the frame only
    want = assert_equals_restatement(pts[:, keep], col[keep], K, *EYE, H, W)
    assert (want.mask[:, W // 2 + 6:] == 0).all() and (want.image[:, W // 2 + 6:] == 0).all() and (want.depth[:, W // 2 + 6:] == 0).all()
    assert want.mask[:, :W // 2 - 6].all() and want.mask_hf.any()


@pytest.mark.parametrize("tol", [0.05, None])
def test_no_points(tol):
    H, W = 17, 33
    got = warp_points(torch.zeros(3, 0, device=DEV), torch.zeros(0, 3, device=DEV), camera(H, W), *EYE, H, W, tol)
    assert got.pixel.shape == (0,) and got.pixel.dtype == torch.int32
    for k in OUTPUTS[:4]:
        assert getattr(got, k).shape[:2] == (H, W) and not getattr(got, k).any(), k
    assert_equals_restatement(np.zeros((3, 0), F32), np.zeros((0, 3), F32), camera(H, W), *EYE, H, W, tol)


def test_both_layouts_of_the_points_are_read_in_place():
    H, W = 17, 33
    pts, col, K = surface(H, W, 515, 7, spread=1.2)
    R, T = yaw(-5)
    want = assert_equals_restatement(pts, col, K, R, T, H, W)                       # [3, P]
    assert_equals_restatement(np.ascontiguousarray(pts.T), col, K, R, T, H, W)      # [P, 3]
    dev = torch.from_numpy(pts).to(DEV)
    wide = torch.zeros(515, 5, device=DEV)
    wide[:, 1:4] = dev.T
    for view in (dev.T, wide[:, 1:4], wide[:, 1:4].T):                                # strided views, no copy made
        assert not view.is_contiguous()
        got = warp_points(view, torch.from_numpy(col).to(DEV), K, R, T, H, W)
        assert all(np.array_equal(bits(getattr(got, k).cpu().numpy()), bits(getattr(want, k))) for k in OUTPUTS)
    # three points: [3, 3] reads as [P, 3]
    assert_equals_restatement(np.ascontiguousarray(pts[:, :3].T), col[:3], K, R, T, H, W)


def lift_case(H, W, seed):
    rng = np.random.default_rng(seed)
    depth = (1.5 + rng.random((H, W))).astype(F32)
    R, T = yaw(15)
    return depth, rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.random((H, W, 3)).astype(F32), camera(H, W), R, T + 0.1


def assert_lift(depth, image, K, R, T, select=None):
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)   # noqa: E731
    pts, col = lift_pixels(dev(depth), dev(image), K, R, T, dev(select))
    wp, wc = RR.lift_pixels(depth, image, K, R, T, select)
    assert pts.shape == wp.shape and col.shape == wc.shape and pts.dtype == col.dtype == torch.float32
    assert np.array_equal(bits(pts.cpu().numpy()), bits(wp)) and np.array_equal(bits(col.cpu().numpy()), bits(wc))
    return wp.shape[0]


def test_lift_every_pixel():
    depth, u8, f32, K, R, T = lift_case(40, 48, 8)
    assert assert_lift(depth, u8, K, R, T) == 40 * 48
    assert assert_lift(depth, f32, K, R, T) == 40 * 48
    depth, u8, f32, K, R, T = lift_case(17, 33, 9)
    assert assert_lift(depth, u8, K, R, T) == 17 * 33


def test_lift_a_selection_across_scan_blocks():
    """40 x 48 pixels are 7.5 blocks of 256: the ranks carry over block ends, with full, empty and partial blocks."""
    depth, u8, f32, K, R, T = lift_case(40, 48, 10)
    sel = np.random.default_rng(11).random((40, 48)) < 0.6
    sel.reshape(-1)[256:512] = True      # a block with every pixel selected
    sel.reshape(-1)[512:768] = False     # one with none
    sel.reshape(-1)[-1] = True           # the last pixel of the partial block
    n = assert_lift(depth, u8, K, R, T, sel)
    assert n == int(sel.sum()) > 256 * 3
    assert assert_lift(depth, f32, K, R, T, sel.astype(np.uint8) * 7) == n          # uint8: non-zero selects
    one = np.zeros((40, 48), bool)
    one[39, 47] = True
    assert assert_lift(depth, f32, K, R, T, one) == 1


def test_lift_an_empty_selection():
    depth, u8, f32, K, R, T = lift_case(17, 33, 12)
    assert assert_lift(depth, u8, K, R, T, np.zeros((17, 33), bool)) == 0


def test_lift_then_warp_returns_the_frame():
    """The two calls are inverses on a frame: lifting every pixel and warping into the same camera resolves each pixel to
    its own colour and depth (to fp32 rounding; the footprint of a point a hair off its pixel has a second, tiny weight)."""
    depth, u8, f32, K, R, T = lift_case(40, 48, 13)
    pts, col = lift_pixels(torch.from_numpy(depth).to(DEV), torch.from_numpy(f32).to(DEV), K, R, T)
    got = warp_points(pts, col, K, R, T, 40, 48, None)
    pixel, own = got.pixel.cpu().view(40, 48), torch.arange(40 * 48).view(40, 48)
    inner = (slice(1, -1), slice(1, -1))
    # (a point of the outermost row or column may land a rounding error outside the frame, where it is invalid)
    assert got.mask.all() and (pixel[inner] == own[inner]).all() and ((pixel == own) | (pixel == -1)).all()
    assert float((got.image.cpu()[inner] - torch.from_numpy(f32)[inner]).abs().max()) < 1e-4
    assert float((got.depth.cpu()[inner] - torch.from_numpy(depth)[inner]).abs().max()) < 1e-4


def test_error_order():
    K, R, T = camera(17, 33), *EYE
    pts, col = torch.zeros(3, 5, device=DEV), torch.zeros(5, 3, device=DEV)
    with pytest.raises(TypeError):                        # the dtype before the gradient, the shape and the device
        warp_points(pts.cpu().half(), col[:4].requires_grad_(), K, R, T, 2, 2)
    with pytest.raises(NotImplementedError):              # the gradient before the shape and the device
        warp_points(pts.cpu(), col[:4].clone().requires_grad_(), K, R, T, 2, 2)
    with pytest.raises(ValueError, match="points must be"):   # the shape before the device
        warp_points(pts.cpu(), col[:4], K, R, T, 17, 33)
    with pytest.raises(ValueError, match="H, W >= 3"):
        warp_points(pts.cpu(), col, K, R, T, 2, 33)
    with pytest.raises(ValueError, match="2\\^31"):
        warp_points(pts.cpu(), col, K, R, T, 65536, 32768)
    with pytest.raises(ValueError, match="must be on the GPU"):
        warp_points(pts.cpu(), col, K, R, T, 17, 33)
    with pytest.raises(ValueError, match="must be on the GPU"):
        warp_points(pts, col.cpu(), K, R, T, 17, 33)
    depth, image = torch.zeros(17, 33, device=DEV), torch.zeros(17, 33, 3, device=DEV)
    with pytest.raises(TypeError):
        lift_pixels(depth.cpu(), image.double(), K, R, T, select=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="select must be"):
        lift_pixels(depth.cpu(), image, K, R, T, select=torch.zeros(3, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="must be on the GPU"):
        lift_pixels(depth.cpu(), image, K, R, T)
    assert warp_points(pts, col, K, R, T, 17, 33).image.shape == (17, 33, 3)   # and the same operands, right, run


def test_capture_and_replay_in_a_graph():
    H, W = 40, 48
    a, ca, K = surface(H, W, 1801, 14, spread=1.2)
    b, cb, _ = surface(H, W, 1801, 15, depth=2.5, spread=1.1)
    R, T = yaw(5)
    pts, col = torch.from_numpy(a).to(DEV), torch.from_numpy(ca).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warp_points(pts, col, K, R, T, H, W)                # warm-up: the library is loaded, the allocator is warm
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # (a capture refuses any call that waits for the device)
        out = warp_points(pts, col, K, R, T, H, W)
    for p, c in ((b, cb), (a, ca)):
        pts.copy_(torch.from_numpy(p))
        col.copy_(torch.from_numpy(c))
        graph.replay()
        torch.cuda.synchronize()
        assert_equals_restatement(p, c, K, R, T, H, W, got={k: getattr(out, k).cpu().numpy() for k in OUTPUTS})
