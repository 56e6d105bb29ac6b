"""Inputs shared by the tests against the reference's own kernels (tests/test_reference_*_gpu.py), the recorder of
their results (tests/golden/make_reference_goldens.py) and the CPU tests that replay the records
(tests/test_reference_goldens_cpu.py).  Everything is regenerated from seeds; nothing here touches a GPU.
"""
import numpy as np

import knn_reference as KR

F32 = np.float32

# ---- knn ----
KNN_KINDS = ["uniform", "planar", "collinear", "identical", "duplicates", "clusters", "offset", "nonfinite", "surface"]
KNN_SIZES = [1, 2, 3, 4, 7, 64, 1000, 20000]
KNN_GOLDEN_SIZES = [P for P in KNN_SIZES if P <= 1000]


def knn_cloud(kind, P):
    return KR.make_cloud(kind, P, seed=P + len(kind))


# ---- grid ----
GRID_DIMS = (1, 2, 3)
GRID_FEATURES = (1, 2, 4, 8)
# the collision-heavy small tables of tests/test_grid_encoder_gpu.py: (resolutions, log2_hashmap_size) per D
SMALL_TABLES = {1: ((7, 50, 300, 3000), 8), 2: ((10, 40, 130, 514), 10), 3: ((18, 33, 80, 201), 10)}
RES_3D = (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514)
RES_2D = (130, 258, 514, 1026)
GOLDEN_N = 400


def level_rows(D, res, log2):
    """min(2^log2, res^D) rounded up to a multiple of 8 (bloomscene_amd.grid_encoder.level_rows, restated so that the CPU
    replay needs no torch)."""
    cap = 2 ** log2
    return [int(np.ceil(min(cap, int(r) ** D) / 8) * 8) for r in res]


def grid_table(D, F, res, log2, seed=0):
    """-> offsets [L + 1] int64, resolutions [L] int64, embeddings [rows, F] fp32"""
    offs = np.array([0] + np.cumsum(level_rows(D, res, log2)).tolist(), np.int64)
    emb = np.random.default_rng(seed).uniform(-1, 1, (int(offs[-1]), F)).astype(F32)
    return offs, np.array(res, np.int64), emb


def special_coordinates(res):
    """fp32 coordinates where the encoder's arithmetic is at an edge, each with its two fp32 neighbours:
    k / (res - 2) (pos = k + 0.5: the weights are exactly one half) and (k + 0.5) / (res - 2) (pos lands on an integer or,
    after rounding, next to it: floor() decides the cell), for the first, middle and last cells of every level; and tiny
    positive values down to the smallest subnormal (x * float(res - 2) + 0.5 is added in DOUBLE by the reference, in fp32
    by include/bloomscene_grid.h)."""
    vals = []
    for r in res:
        s = F32(int(r) - 2)
        for k in (0, 1, int(r) // 2, int(r) - 3, int(r) - 2):
            for num in (F32(k), F32(k) + F32(0.5)):
                v = F32(num / s)
                vals += [np.nextafter(v, F32(-1)), v, np.nextafter(v, F32(2))]
    tiny = [2.0 ** -149, 2.0 ** -148, 3 * 2.0 ** -149, 2.0 ** -140, 2.0 ** -127, 2.0 ** -126, 2.0 ** -100, 2.0 ** -60,
            2.0 ** -37, 2.0 ** -30, 2.0 ** -26, 2.0 ** -25, 2.0 ** -24, 2.0 ** -23]
    return np.array(vals + tiny, F32)


def grid_points(N, D, res, seed):
    """[N, D] fp32: uniform points, then (N >= 64) the edge points of tests/test_grid_encoder_gpu.py in rows 0 .. 29 --
    exactly 0, exactly 1, out of range, border cells -- and from row 30 on special_coordinates(res): once in one
    coordinate of an otherwise random point, once in every coordinate."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (N, D)).astype(F32)
    if N >= 64:
        x[0:4] = 0.0
        x[4:8] = 1.0
        x[8, 0] = -0.25
        x[9, -1] = 1.5
        x[10:20] = rng.uniform(0, 0.004, (10, D)).astype(F32)
        x[20:30] = 1 - rng.uniform(0, 0.004, (10, D)).astype(F32)
        sp = special_coordinates(res)
        n = min(len(sp), (N - 30) // 2)
        for i in range(n):
            x[30 + i, i % D] = sp[i]
            x[30 + n + i, :] = sp[i]
    return x


def grid_grad(L, N, F, seed, sigma=1.0):
    return np.random.default_rng(seed).normal(0, sigma, (L, N, F)).astype(F32)


def golden_grid_case(D, F):
    """The recorded small case of (D, F): table, points, upstream gradient."""
    res, log2 = SMALL_TABLES[D]
    offs, r, emb = grid_table(D, F, res, log2, seed=D * 10 + F)
    x = grid_points(GOLDEN_N, D, res, seed=100 + F)
    g = grid_grad(len(res), GOLDEN_N, F, seed=7)
    return offs, r, emb, x, g
