"""The ORDER of csrc/grid_sum.h's grid-wide fp64 sum, restated in numpy float64 from the header's comment, with switches
for the orders it must NOT be:

  1. per wave a xor butterfly, offsets 32 .. 1          lanes="ascending": offsets 1 .. 32; "sequential": lane 0 + 1 + ..
  2. the wave results from the left                      waves="right": ((s3 + s2) + s1) + s0
  3. thread 0 stores the workgroup's partial
  4. the last workgroup: thread t adds the partials      partials="contiguous": thread t adds the partials c t .. c t + c - 1,
     t, t + 256, ... in that order onto 0.0, then           c = ceil(G / 256); "pairwise": all G partials as one balanced
     steps 1 and 2 again                                    tree, neighbours first, without the threads

A butterfly step adds the same two values on both sides and fp addition commutes, so after the step with offset o the
lanes l and l ^ o hold the same bits: the value every lane ends with is that of a tree, and one half of the lanes is
enough to carry on with.  "contiguous" is the header's own order while G <= 256 (c = 1), and "pairwise" while G <= 2 (one
addition): no input can tell them apart there (same_sequence).

`cancelling_grid` is the input family that makes an order show in the bits (the idea of cancelling_rows in
test_mlp_wgrad_order.py): values of order 1 everywhere, and a few twins +B / -B of about 2^60.  While an accumulator
stands at 2^60 it keeps nothing below 2^8 of what is added to it, so the result is the sum of the values that met no B --
which ones, the order decides.  The twins sit
  * on lanes 1 and 2 of a wave (they meet in the LAST butterfly step 32 .. 1, in the second of 1 .. 32, at once in a
    lane-by-lane sum),
  * on waves 1 and 2 of a workgroup (from the left s0 is lost, from the right s3),
  * for G > 33 on workgroups 1 and 33, whose partials meet in the first butterfly step of the last workgroup and in the
    last of an ascending one, and which a contiguous split gives to two threads far apart,
  * for G > 256 on workgroups 0 and 256 floor((G - 1) / 256): the first and the last partial of thread 0,
each in a workgroup and wave of its own where the grid has that many, and for G <= 2 so that the wave with the lane twin
is added last (what a B has passed is lost to every order alike)."""
import numpy as np

BLOCK = 256
ORDERS = {                         # name -> the switches of the wrong order
    "butterfly_ascending": dict(lanes="ascending"),
    "lanes_left_to_right": dict(lanes="sequential"),
    "waves_from_the_right": dict(waves="right"),
    "partials_contiguous": dict(partials="contiguous"),
    "partials_pairwise": dict(partials="pairwise"),
}


def same_sequence(order, G):
    """whether the wrong order performs the header's own additions at this grid (see the module's docstring)"""
    return (order == "partials_contiguous" and G <= BLOCK) or (order == "partials_pairwise" and G <= 2)


def _pairwise(v):
    """v [m, ...] -> the balanced tree over axis 0, neighbours first (an odd one out joins the next level)"""
    while len(v) > 1:
        even = v[0:len(v) - (len(v) & 1):2] + v[1::2]
        v = np.concatenate([even, v[-1:]]) if len(v) & 1 else even
    return v[0]


def _workgroup(v, lanes, waves):
    """v [..., 256, N] -> [..., N]: steps 1 and 2"""
    v = v.reshape(v.shape[:-2] + (BLOCK // 64, 64, v.shape[-1]))
    if lanes == "descending":
        h = 32
        while h:
            v = v[..., :h, :] + v[..., h:2 * h, :]
            h >>= 1
        s = v[..., 0, :]
    elif lanes == "ascending":
        while v.shape[-2] > 1:
            v = v[..., 0::2, :] + v[..., 1::2, :]
        s = v[..., 0, :]
    else:
        assert lanes == "sequential"
        s = v[..., 0, :]
        for lane in range(1, 64):
            s = s + v[..., lane, :]
    order = range(BLOCK // 64) if waves == "left" else range(BLOCK // 64 - 1, -1, -1)
    assert waves in ("left", "right")
    order = list(order)
    out = s[..., order[0], :]
    for w in order[1:]:
        out = out + s[..., w, :]
    return out


def workgroup_partials(x, lanes="descending", waves="left"):
    """x [G, 256, N] float64 -> the partials [G, N] (steps 1 to 3)"""
    x = np.asarray(x)
    assert x.dtype == np.float64 and x.ndim == 3 and x.shape[1] == BLOCK
    return _workgroup(x, lanes, waves)


def last_workgroup(p, lanes="descending", waves="left", partials="strided"):
    """p [G, N] -> the totals [N] (step 4)"""
    G, N = p.shape
    if partials == "pairwise":
        return _pairwise(p)
    c = (G + BLOCK - 1) // BLOCK
    padded = np.zeros((c * BLOCK, N))        # (a thread that runs out of partials adds nothing: x + 0.0 == x, and no
    padded[:G] = p                           # accumulator is ever -0.0: they start from +0.0)
    own = padded.reshape(c, BLOCK, N) if partials == "strided" else padded.reshape(BLOCK, c, N).transpose(1, 0, 2)
    assert partials in ("strided", "contiguous")
    v = np.zeros((BLOCK, N))
    for j in range(c):
        v = v + own[j]
    return _workgroup(v, lanes, waves)


def grid_sum(x, lanes="descending", waves="left", partials="strided"):
    """x [G, 256, N] float64 -> what grid_sum<N, 256> leaves in thread 0 of the last workgroup, [N]"""
    return last_workgroup(workgroup_partials(x, lanes, waves), lanes, waves, partials)


def _twin(x, rng, a, b):
    """+B at x[a], -B at x[b], another B of [2^59, 2^60) for every one of the N sums (a multiple of 2^52: sums of them are exact)"""
    B = rng.integers(128, 256, size=x.shape[-1]).astype(np.float64) * 2.0 ** 52
    x[a], x[b] = B, -B


def cancelling_grid(G, N, seed=0):
    """-> x [G, 256, N] float64 (see the module's docstring)"""
    rng = np.random.default_rng([seed, G, N])
    x = rng.standard_normal((G, BLOCK, N))
    if G <= 2:
        lane_wg, wave_wg, lane_wave = G - 1, 0, 3
    else:
        lane_wg, wave_wg, lane_wave = (70, 140, 1) if G > 140 else (G - 1, G - 2, 1)
    _twin(x, rng, (lane_wg, 64 * lane_wave + 1), (lane_wg, 64 * lane_wave + 2))
    _twin(x, rng, (wave_wg, 64 * 1 + 7), (wave_wg, 64 * 2 + 50))
    if G > 33:
        _twin(x, rng, (1, 100), (33, 3))
    if G > BLOCK:
        _twin(x, rng, (0, 200), (BLOCK * ((G - 1) // BLOCK), 31))
    return x
