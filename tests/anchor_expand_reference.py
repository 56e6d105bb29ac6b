"""A numpy restatement of the anchor expansion's backward (k_anchor_expand_bwd, bloomscene_amd/csrc/anchors.hip) and a
model of its three-kernel selection (counts per workgroup, exclusive scan in rounds of 8192 counts, ordered write),
plus the seeded inputs that tests/test_anchor_expand_reference_cpu.py and tests/test_anchor_expand_edges_gpu.py share.
Test infrastructure only: the product never imports it.

What the kernel computes with ONE rounding per operation and no library function is restated in fp32 and compared bit
for bit: d_neural_opacity, d_color, d_offsets = fl(g_xyz * gs[c]), and the per-anchor sums d_anchor / d_gs[:, 0:3],
which include/bloomscene_anchors.h promises in slot order k = 0 .. K-1 from +0.0 (the unit is built without
contraction, so fl(g * of) and the additions round separately).  What goes through the sigmoid or the quaternion norm
(d_gs[:, 3:6], d_sr) is restated in float64 and compared by distance.
"""
import functools

import numpy as np
import torch

from oracle import anchors as OA

BLOCK = 256          # lanes of a workgroup (BSR_ANCHOR_BLOCK)
SCAN_ROUND = 8192    # workgroup counts per round of k_anchor_scan (1024 lanes x 8)
EPS = 1e-12          # F.normalize's eps

UPSTREAMS = ("xyz", "color", "opacity", "scaling", "rot")
WIDTHS = {"xyz": 3, "color": 3, "opacity": 1, "scaling": 3, "rot": 4}
IN_NAMES = ("anchor", "grid_scaling", "grid_offsets", "neural_opacity", "color", "scale_rot")


# ---------------------------------------------------------------------------------------------- the backward
def _scatter(g, sel, width, dtype):
    """Upstream [S, width] (selected candidates, candidate order) -> [n_cand, width]; +0.0 on unselected rows."""
    out = np.zeros((sel.size, width), dtype)
    if g is not None:
        out[sel] = np.asarray(g, dtype).reshape(-1, width)
    return out


def slot_order_sum(terms):
    """[N, K, C] -> [N, C]: acc = +0.0; acc += terms[:, k] for k = 0 .. K-1, each addition rounded in terms.dtype."""
    acc = np.zeros((terms.shape[0], terms.shape[2]), terms.dtype)
    for k in range(terms.shape[1]):
        acc = acc + terms[:, k]
    return acc


def tree_sum(terms):
    """[N, K, C] -> [N, C] by the strided halving of an LDS reduction (x[i] += x[i + s], s = P/2 .. 1; K padded with
    +0.0 to a power of two P): the order a rewrite of the kernel's sum would most likely use instead."""
    n, k, c = terms.shape
    p = 1
    while p < k:
        p *= 2
    x = np.zeros((n, p, c), terms.dtype)
    x[:, :k] = terms
    s = p // 2
    while s >= 1:
        x = x[:, :s] + x[:, s:2 * s]
        s //= 2
    return x[:, 0]


def expand_backward(anchor, grid_scaling, grid_offsets, neural_opacity, color, scale_rot,
                    g_xyz, g_color, g_opacity, g_scaling, g_rot, K, dtype=np.float32):
    """-> dict.  In ``dtype`` (fp32: the kernel's bits): d_anchor [N,3], d_gs_xyz [N,3] (= d_grid_scaling[:, 0:3]),
    d_offsets [N*K,3], d_color [N*K,3], d_neural_opacity [N*K].  In float64 from the same inputs: d_gs_scale [N,3]
    (= d_grid_scaling[:, 3:6]) and d_sr [N*K,7].  A missing upstream (None) is zeros, as in the C ABI."""
    del anchor, color   # (their values do not enter any gradient)
    gs = np.asarray(grid_scaling, dtype)
    N = gs.shape[0]
    of = np.asarray(grid_offsets, dtype).reshape(N * K, 3)
    sr = np.asarray(scale_rot, np.float64).reshape(N * K, 7)
    sel = np.asarray(neural_opacity).reshape(-1) > 0
    gs_rep = np.repeat(gs, K, axis=0)
    gx = _scatter(g_xyz, sel, 3, dtype)
    with np.errstate(all="ignore"):
        out = {
            "d_neural_opacity": _scatter(g_opacity, sel, 1, dtype).reshape(-1),
            "d_color": _scatter(g_color, sel, 3, dtype),
            "d_offsets": gx * gs_rep[:, :3],
            "d_anchor": slot_order_sum(gx.reshape(N, K, 3)),
            "d_gs_xyz": slot_order_sum((gx * of).reshape(N, K, 3)),
        }
        # ---- float64: through the sigmoid and the normalisation
        gsc = _scatter(g_scaling, sel, 3, np.float64)
        s = 1.0 / (1.0 + np.exp(-sr[:, :3]))
        out["d_gs_scale"] = (gsc * s).reshape(N, K, 3).sum(axis=1)
        d_sr = np.zeros((N * K, 7), np.float64)
        d_sr[:, :3] = gsc * gs_rep[:, 3:6].astype(np.float64) * (s * (1.0 - s))
        g = _scatter(g_rot, sel, 4, np.float64)
        v = sr[:, 3:7]
        length = np.sqrt((v * v).sum(axis=1, keepdims=True))
        normal = length > EPS
        safe = np.where(normal, length, 1.0)
        r = v / safe
        d_sr[:, 3:7] = np.where(normal, (g - r * (r * g).sum(axis=1, keepdims=True)) / safe, g / EPS)
        out["d_sr"] = d_sr
    for k in ("d_neural_opacity", "d_color", "d_offsets", "d_anchor", "d_gs_xyz"):
        assert out[k].dtype == dtype, k
    return out


def normal_branch_rot_gradient(scale_rot, g_rot_rows):
    """(g - r (r.g)) / |v| for every row, whatever |v| is: what the backward would give WITHOUT its clamped branch
    (float64; rows with |v| = 0 come out non-finite)."""
    v = np.asarray(scale_rot, np.float64).reshape(-1, 7)[:, 3:7]
    g = np.asarray(g_rot_rows, np.float64)
    with np.errstate(all="ignore"):
        length = np.sqrt((v * v).sum(axis=1, keepdims=True))
        r = v / length
        return (g - r * (r * g).sum(axis=1, keepdims=True)) / length


# ---------------------------------------------------------------------------------------------- the selection
def selection_model(mask, K, carry="kept"):
    """The three kernels' bookkeeping: a workgroup owns per_wg = (256 // K) * K consecutive candidates; counts per
    workgroup; exclusive scan in rounds of 8192 counts with a running carry; destination = workgroup base + rank among
    the workgroup's lanes.  -> (counts, bases, destination row of every selected candidate in candidate order, total).
    ``carry``: "kept" (the kernel), or the two mutations "dropped" / "doubled" a test must be able to see.
    K = 1 is the partition of bsr_visible_filter_indices (256 points per workgroup)."""
    mask = np.asarray(mask, bool).reshape(-1)
    per_wg = (BLOCK // K) * K
    n_wg = -(-mask.size // per_wg)
    lanes = np.zeros(n_wg * per_wg, bool)
    lanes[:mask.size] = mask
    lanes = lanes.reshape(n_wg, per_wg)
    counts = lanes.sum(axis=1).astype(np.int64)
    bases, run = np.zeros(n_wg, np.int64), 0
    for r0 in range(0, n_wg, SCAN_ROUND):
        c = counts[r0:r0 + SCAN_ROUND]
        bases[r0:r0 + c.size] = {"kept": run, "dropped": 0, "doubled": 2 * run}[carry] + np.cumsum(c) - c
        run += int(c.sum())
    rank = np.cumsum(lanes, axis=1) - lanes
    dest = (bases[:, None] + rank).reshape(-1)[:mask.size]
    return counts, bases, dest[mask], run


def workgroups(N, K):
    return -(-N // (BLOCK // K))


# ---------------------------------------------------------------------------------------------- shared inputs
def upstreams(S, seed, names=UPSTREAMS):
    """name -> randn [S, width] (fp32) for the names given, None for the others."""
    g = torch.Generator().manual_seed(seed)
    full = {n: torch.randn(S, WIDTHS[n], generator=g) for n in UPSTREAMS}
    return {n: (full[n] if n in names else None) for n in UPSTREAMS}


def regional_opacity(N, K, seed):
    """neural_opacity [N*K, 1] whose selection density varies by region -- 0.1, 0.9 and 0.5 in thirds -- with 300
    workgroups selecting nothing across the scan's first round boundary (workgroups 8042 .. 8341) and the last anchor
    fully selected, so that the last count of the last round is not zero: a wrong carry then moves rows."""
    g = torch.Generator().manual_seed(seed)
    n = N * K
    keep = torch.tensor([0.1, 0.9, 0.5]).repeat_interleave(-(-n // 3))[:n]
    mag = torch.rand(n, generator=g) + 1e-3
    nop = torch.where(torch.rand(n, generator=g) < keep, mag, -mag)
    per_wg = (BLOCK // K) * K
    nop[(SCAN_ROUND - 150) * per_wg:(SCAN_ROUND + 150) * per_wg] = -1.0
    nop[(N - 1) * K:] = 0.5
    return nop.view(n, 1)


SCAN_SHAPES = ((8192, 129), (8193, 129), (25 * 16384 + 1, 10))   # 8192, 8193 and 16385 workgroup counts
VISIBLE_P = 8192 * 256 + 257                                     # 8194 workgroup counts


@functools.lru_cache(maxsize=1)
def scan_inputs(N, K):
    """(one case is kept: the largest holds 230 MB)"""
    inp = list(OA.synthetic_anchor_inputs(N, K, seed=N % 1000))
    inp[3] = regional_opacity(N, K, seed=K)
    return tuple(inp)


@functools.lru_cache(maxsize=None)
def visible_pattern():
    """bool [VISIBLE_P]: in front of the camera or behind it, alternating in blocks of irregular length (1 .. 700); the
    last 300 points in front, so that the second round's last count is not zero."""
    rng = np.random.default_rng(5)
    lengths = rng.integers(1, 701, size=VISIBLE_P // 300)
    front = np.repeat(np.arange(lengths.size) % 2 == 0, lengths)[:VISIBLE_P]
    assert front.size == VISIBLE_P
    front[-300:] = True
    return front


AWKWARD_K = (2, 85, 86, 128, 129, 255)


@functools.lru_cache(maxsize=None)
def awkward_inputs(K):
    """N = 3 * (256 // K) + 1: three full workgroups and a last one that holds a single anchor."""
    return OA.synthetic_anchor_inputs(3 * (BLOCK // K) + 1, K, seed=K)


CLAMP_KINDS = ("zero", "3e-13 e0", "4 x 1e-13", "2e-12 e0", "4 x 1e-7", "ordinary")
CLAMPED = (True, True, True, False, False, False)
CLAMP_MARGIN = 0.01   # of the clamped rows' scale: how far the normal-branch formula is from them, at least


@functools.lru_cache(maxsize=None)
def clamped_inputs():
    """(inputs, kind int64 [400]): N = 40, K = 10, every candidate selected; candidate i has a quaternion of kind
    i % 6 (CLAMP_KINDS).  |v| = 0, 3e-13 and 2e-13 take the clamped branch, 2e-12, 2e-7 and the ordinary rows the
    normal one; every row is at least a factor 1.5 away from |v| = 1e-12 on its side."""
    inp = list(OA.synthetic_anchor_inputs(40, 10, seed=40))
    inp[3] = inp[3].abs() + 0.1
    kind = torch.arange(400) % 6
    q = inp[5][:, 3:7]
    sign = torch.where(torch.rand(400, 4, generator=torch.Generator().manual_seed(41)) < 0.5, -1.0, 1.0)
    e0 = torch.tensor([1.0, 0.0, 0.0, 0.0])
    q[kind == 0] = 0.0
    q[kind == 1] = 3e-13 * e0
    q[kind == 2] = 1e-13 * sign[kind == 2]
    q[kind == 3] = 2e-12 * e0
    q[kind == 4] = 1e-7 * sign[kind == 4]
    return tuple(inp), kind


SUBSETS = (("xyz",), ("color",), ("opacity",), ("scaling",), ("rot",), ("xyz", "rot"), ("color", "opacity"), ())


@functools.lru_cache(maxsize=None)
def subset_inputs():
    """(50, 10), about half the candidates selected; ordinary quaternions only, so that no clamped row sets the scale
    of d_sr[:, 3:7] (clamped_inputs has those)."""
    return OA.synthetic_anchor_inputs(50, 10, seed=50, keep_fraction=0.55)


def numpy_inputs(inp, dtype=np.float32):
    return [t.detach().cpu().numpy().astype(dtype) for t in inp]


def restate(inp, up, K, dtype=np.float32):
    """expand_backward on torch inputs and an upstreams() dict."""
    g = [None if up[n] is None else up[n].detach().cpu().numpy().astype(dtype) for n in UPSTREAMS]
    return expand_backward(*numpy_inputs(inp, dtype), *g, K, dtype=dtype)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
