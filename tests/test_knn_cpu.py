"""simple_knn / mean_dist3, CPU side: the restatement (tests/knn_reference.py) against its float64 twin and hand-computed
cases, the torch brute force equal to the numpy one bit for bit, the pruning bound of csrc/knn.hip below every distance
it stands for, the shim's import and rejections without a GPU, and the scratch size function."""
import ctypes
import os

import numpy as np
import pytest
import torch

import knn_reference as KR

F32 = np.float32
FLT_MAX = KR.FLT_MAX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("kind", ["uniform", "planar", "collinear", "clusters", "surface", "duplicates"])
def test_restatement_matches_float64_twin(kind):
    x = KR.make_cloud(kind, 700, seed=3)
    got = KR.mean_dist3_numpy(x).astype(np.float64)
    twin = KR.mean_dist3_f64(x)
    scale = np.maximum(np.abs(twin), 1e-30)
    # rounding of the coordinates' differences only: a few ulp relative, except where cancellation leaves ~0
    ok = (np.abs(got - twin) <= 4e-6 * scale) | (np.abs(got - twin) <= 1e-12)
    assert ok.all(), (kind, np.abs(got - twin).max())


def test_small_p_hand_cases():
    # P = 1, 2: no three neighbours -> (FLT_MAX + FLT_MAX + ...) / 3 = inf
    assert np.isposinf(KR.mean_dist3_numpy(np.zeros((1, 3), F32))).all()
    assert np.isposinf(KR.mean_dist3_numpy(np.array([[0, 0, 0], [1, 0, 0]], F32))).all()
    # P = 3: two real neighbours + FLT_MAX -> FLT_MAX / 3
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], F32)
    out = KR.mean_dist3_numpy(x)
    assert np.array_equal(_bits(out), _bits(np.full(3, FLT_MAX / F32(3))))
    assert abs(float(out[0]) - 1.1342744e38) < 1e32
    # P = 4: the corners of a unit right tetrahedron
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    out = KR.mean_dist3_numpy(x)
    assert out[0] == F32(1.0)                                    # (1 + 1 + 1) / 3
    assert out[1] == F32(5.0) / F32(3.0)                         # (1 + 2 + 2) / 3
    for P in (1, 2, 3, 4):
        xx = KR.make_cloud("uniform", P, seed=P)
        assert np.array_equal(_bits(KR.mean_dist3_numpy(xx)), _bits(KR.mean_dist3_torch(torch.from_numpy(xx)).numpy()))


def test_duplicates_and_ties():
    # duplicates count, as 0
    x = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [5, 5, 5]], F32)
    out = KR.mean_dist3_numpy(x)
    assert (out[:4] == 0).all()
    assert out[4] == F32(75.0)
    # two copies: the third best is the next real neighbour
    x = np.array([[0, 0, 0], [0, 0, 0], [3, 0, 0], [0, 4, 0]], F32)
    out = KR.mean_dist3_numpy(x)
    assert out[0] == (F32(9) + F32(16)) / F32(3)
    # ties: four neighbours at the same distance, three of them count
    x = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], F32)
    assert KR.mean_dist3_numpy(x)[0] == F32(1.0)
    # the sum in order, then a correctly rounded division
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, np.sqrt(F32(5))]], F32)
    d = KR.pair_dist(x[0], x[3])
    assert KR.mean_dist3_numpy(x)[0] == ((F32(1) + F32(1)) + d) / F32(3)


def test_nonfinite_points():
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], F32)
    out = KR.mean_dist3_numpy(x)
    assert np.isposinf(out[4:]).all()
    # nobody's neighbour: the finite points see the same as without them
    assert np.array_equal(_bits(out[:4]), _bits(KR.mean_dist3_numpy(x[:4])))
    t = KR.mean_dist3_torch(torch.from_numpy(x)).numpy()
    assert np.array_equal(_bits(out), _bits(t))


def test_overflowing_distances_never_count():
    # d around 1e19^2: below FLT_MAX it counts, at or above it (inf) it does not
    x = np.array([[0, 0, 0], [1.5e19, 0, 0], [0, 1.2e19, 0], [0, 0, 1.0e19], [3e19, 0, 0]], F32)
    out = KR.mean_dist3_numpy(x)
    d01, d02, d03 = (KR.pair_dist(x[0], x[k]) for k in (1, 2, 3))
    assert d01 < FLT_MAX and np.isfinite(d01)
    with np.errstate(over="ignore"):
        assert out[0] == ((d03 + d02) + d01) / F32(3)   # (the sum itself overflows: inf)
    # point 4 is 3e19 from the origin: d = 9e38 -> inf, and 1.5e19 from point 1: d = 2.25e38 counts
    assert np.isinf(KR.pair_dist(x[4], x[0]))
    d41 = KR.pair_dist(x[4], x[1])
    assert d41 < FLT_MAX
    with np.errstate(over="ignore"):
        assert out[4] == ((d41 + FLT_MAX) + FLT_MAX) / F32(3)
    t = KR.mean_dist3_torch(torch.from_numpy(x)).numpy()
    assert np.array_equal(_bits(out), _bits(t))


@pytest.mark.parametrize("kind", ["uniform", "planar", "collinear", "identical", "duplicates", "clusters", "offset",
                                  "nonfinite", "surface"])
def test_torch_brute_force_equals_numpy_bit_for_bit(kind):
    x = KR.make_cloud(kind, 1500, seed=11)
    a = KR.mean_dist3_numpy(x)
    b = KR.mean_dist3_torch(torch.from_numpy(x), chunk=97).numpy()
    assert np.array_equal(_bits(a), _bits(b)), kind


def test_box_bounds_never_exceed_a_distance_inside_the_box():
    rng = np.random.default_rng(5)
    n_box, m = 4000, 16
    for scale in (1e-3, 1.0, 1e6, 1e18):
        centre = rng.normal(0, scale, (n_box, 1, 3))
        pts = (centre + rng.normal(0, scale * rng.uniform(1e-4, 1, (n_box, 1, 1)), (n_box, m, 3))).astype(F32)
        lo, hi = pts.min(1), pts.max(1)
        # queries: random, on the box's faces, one ulp outside, inside
        q = (centre[:, 0] + rng.normal(0, 2 * scale, (n_box, 3))).astype(F32)
        q[: n_box // 4] = np.nextafter(lo[: n_box // 4], -np.inf)
        q[n_box // 4: n_box // 2] = np.nextafter(hi[n_box // 4: n_box // 2], np.inf)
        bp = KR.box_bound_point(q, lo, hi)
        d = KR.pair_dist(q[:, None, :], pts)
        assert (bp[:, None] <= d).all(), scale
        # the wave-level form: a box of queries around q
        qs = (q[:, None, :] + rng.normal(0, scale * 0.05, (n_box, 4, 3))).astype(F32)
        qlo, qhi = qs.min(1), qs.max(1)
        br = KR.box_bound_range(qlo, qhi, lo, hi)
        for k in range(4):
            assert (br <= KR.box_bound_point(qs[:, k], lo, hi)).all()
            assert (br[:, None] <= KR.pair_dist(qs[:, k][:, None, :], pts)).all()


def test_simple_knn_shim_imports_without_a_gpu_and_rejects_bad_input():
    from simple_knn._C import distCUDA2
    from bloomscene_amd.knn import mean_dist3
    assert callable(distCUDA2)
    with pytest.raises(ValueError, match="no CPU path"):
        distCUDA2(torch.zeros(10, 3))
    with pytest.raises(TypeError):
        distCUDA2(torch.zeros(10, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        distCUDA2(torch.zeros(10, 4))
    with pytest.raises(ValueError):
        mean_dist3(torch.zeros(10))


def test_scratch_bytes_monotone_and_aligned():
    lib = ctypes.CDLL(os.path.join(ROOT, "bloomscene_amd", "libbloomscene_rast.so"))
    lib.bsr_knn_scratch_bytes.restype = ctypes.c_size_t
    lib.bsr_knn_scratch_bytes.argtypes = [ctypes.c_int]
    sizes = [0, 1, 2, 3, 63, 64, 65, 255, 256, 4095, 4096, 4097, 65536, 262143, 262144, 262145, 10 ** 6, 4 * 10 ** 6,
             1 << 28]
    prev = 0
    for P in sizes:
        b = lib.bsr_knn_scratch_bytes(P)
        assert b % 256 == 0 and b >= prev and b >= 16 * P, (P, b)
        prev = b
    rng = np.random.default_rng(0)
    ps = np.sort(rng.integers(0, 1 << 22, 2000))
    bs = [lib.bsr_knn_scratch_bytes(int(p)) for p in ps]
    assert all(a <= b for a, b in zip(bs, bs[1:]))
    assert lib.bsr_knn_scratch_bytes(-5) == 0
