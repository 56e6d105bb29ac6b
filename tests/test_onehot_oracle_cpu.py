"""The premises of tests/test_strict_backward_gpu.py, held on the CPU oracle where there is no GPU.

With dL/dcolour kept at ONE pixel (onehot.onehot_upstream) every per-pair term of every other pixel is exactly +-0, a
Gaussian occurs at most once in a tile's list and a pixel belongs to one tile: each of the oracle's 9 P pair sums then
has at most one nonzero term.  A sum of one value and zeros is that value in any order and any precision, so the
oracle's result is the fp32 per-pair term itself -- which is what lets the GPU test ask k_render_bwd_strict for VALUE
equality.  Checked here, per hot pixel:
  * abs_sums == |sums| bit for bit (one term per sum: sum |term| = |sum of terms|),
  * the binary32 summation order (f32_sums=True) gives the binary64 order's result bit for bit,
  * the coverage the GPU test relies on: >= 15 Gaussians with a nonzero dL_dcolors row per hot pixel, >= 200
    (Gaussian, pixel) pairs per case, hot pixels in all four 8 x 8 quadrants of the hottest tile."""
import numpy as np
import pytest

import helpers as Hh
import onehot as OH
from oracle import oracle as O

from test_parity_gpu import CASES as GPU_CASES   # (shapes only: importing the module touches no GPU)

CASES = {"lists_gt_1024": GPU_CASES["lists_gt_1024"], "huge_splats": GPU_CASES["huge_splats"],
         "dense_ragged": OH.DENSE_RAGGED}


def test_hot_offsets_cover_every_column_row_and_quadrant():
    assert sorted(x for x, _ in OH.HOT_OFFSETS) == list(range(16))
    assert sorted(y for _, y in OH.HOT_OFFSETS) == list(range(16))
    assert {(x >= 8, y >= 8) for x, y in OH.HOT_OFFSETS} == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize("name", list(CASES))
def test_onehot_upstream_leaves_one_term_per_sum(name):
    c = Hh.make_case(**CASES[name])
    st, _ = Hh.run_oracle(c, backward=False)
    pix = OH.hot_pixels(st.n_contrib, c.W, c.H)
    assert (c.W - 1, c.H - 1) in pix and len(pix) <= 17
    tx, ty = OH.hottest_tile(st.n_contrib, c.W, c.H)
    in_tile = [(x, y) for x, y in pix if x // 16 == tx and y // 16 == ty]
    assert {((x % 16) >= 8, (y % 16) >= 8) for x, y in in_tile} == {(False, False), (False, True), (True, False),
                                                                    (True, True)}
    pairs = 0
    for x, y in pix:
        gC = OH.onehot_upstream(c.gC, x, y)
        assert int((gC != 0).any(dim=0).sum()) == 1
        g = O.backward(st, gC, c.gD, want_abs_sums=True)
        nine = OH.nine_sums(g)
        np.testing.assert_array_equal(g.abs_sums.view(np.uint32), np.abs(nine).view(np.uint32))
        g32 = O.backward(st, gC, c.gD, f32_sums=True)
        np.testing.assert_array_equal(OH.nine_sums(g32).view(np.uint32), nine.view(np.uint32))
        rows = int((g.dL_dcolors != 0).any(axis=1).sum())
        assert rows >= 15, (name, (x, y), rows)
        # every Gaussian with a nonzero row is one the pixel's own tile lists below the pixel's last contributor
        t = (y // 16) * st.grid[0] + x // 16
        blended = st.point_list[int(st.ranges[t, 0]):int(st.ranges[t, 0]) + int(st.n_contrib[c.W * y + x])]
        assert np.isin(np.nonzero((nine != 0).any(axis=1))[0], blended).all()
        pairs += rows
    assert pairs >= 200, (name, pairs)
