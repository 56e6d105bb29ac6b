"""csrc/wg_scan.h on its own: every instantiation the product makes, run by tests/native/libbsr_shared_pieces.so on given
words and compared with numpy.cumsum in uint64 reduced mod 2^32 (wg_scan_reference.py), `==` on every word.

The instantiations in csrc (a search for the five function names), all of them callable here:

  function              arguments                  called from                                        entry point
  wg_exclusive_scan     <16, 4> AllValid           binning.hip k_scans (twice on one s_wave),         pt_wg_scan 0
                                                   reproject.hip (BSR_LIFT_SCAN_WAVES = 16)
  wg_exclusive_scan     <16, 4> Hist1ColumnValid   binning.hip k_scans, the rows of hist1             pt_wg_scan 1
  wg_exclusive_scan     <16, 8>                    anchors.hip                                        pt_wg_scan 2
  wg_exclusive_scan     <16, 1>                    voxelize.hip, the block heads                      pt_wg_scan 3
  wg_exclusive_scan     <4, 1>                     binning.hip k_radix_rowscan, voxelize.hip,         pt_wg_scan 4
                                                   knn.hip, anchor_codec.hip (all 256 threads)
  wg_exclusive_sum      <4>, with and without      binning.hip, voxelize.hip, knn.hip,                pt_wg_rounds 0
                        `total`                    anchor_codec.hip
  wg_exclusive_count    <4>, with and without      voxelize.hip k_voxel_emit (alternating sets),      pt_wg_rounds 1
                        `total`                    reproject.hip, anchors.hip
  wg_total              <4>                        adjust.hip, anchor_state.hip, anchor_codec.hip,    pt_wg_totals
                                                   voxelize.hip
  wg_total_of           <4>                        adjust.hip k_decide_plan, anchor_state.hip         pt_wg_totals

Sizes of the array scan, with STEP = 64 * WAVES * VPT: 0, 1, 63, 64, 65, STEP - 1, STEP, STEP + 1, 2 STEP, 2 STEP + 1,
3 STEP + 1 (the third step: the first reuse of an LDS set) and 4 STEP + VPT + 1 (a fifth step, whose last working thread
has a partly filled vector); values below 2^16, and up to 2^32 - 1 so that the sums wrap."""
import numpy as np
import pytest
import torch

import shared_pieces as SP
import wg_scan_reference as WR

pytestmark = pytest.mark.gpu

SCANS = {                          # name -> (number of the entry point, WAVES, VPT)
    "16x4": (0, 16, 4),
    "16x4_column_valid": (1, 16, 4),
    "16x8": (2, 16, 8),
    "16x1": (3, 16, 1),
    "4x1": (4, 4, 1),
}
TAIL, TAIL_WORD = 64, 0xA5A5A5A5
POISON = 0xDEADBEEF
VALUES = {"below_2_16": 1 << 16, "wrapping": 1 << 32}


def _sizes(waves, vpt):
    step = 64 * waves * vpt
    return [0, 1, 63, 64, 65, step - 1, step, step + 1, 2 * step, 2 * step + 1, 3 * step + 1, 4 * step + vpt + 1]


def _scan(name, rows, write_mask, per=None, n_wg=None):
    """rows [calls, n] uint32 -> (the rows afterwards with their tails [calls, n + TAIL], what every thread was
    returned [calls, 64 * WAVES])"""
    inst, waves, _ = SCANS[name]
    rows = np.asarray(rows, dtype=np.uint32)
    calls, n = rows.shape
    if per is None:                # every column valid: wg_of_column < 8 * per for every column below 8 * per
        per = max(1, (n + 7) // 8)
        n_wg = 8 * per
    host = np.full((calls, n + TAIL), TAIL_WORD, dtype=np.uint32)
    host[:, :n] = rows
    data = SP.u32(host)
    totals = SP.u32(np.full((calls, 64 * waves), 0xFFFFFFFF, dtype=np.uint32))
    rc = SP.lib().pt_wg_scan(inst, n, SP.ptr(data), SP.C.c_size_t(n + TAIL), write_mask, calls, per, n_wg, SP.ptr(totals), SP.stream())
    torch.cuda.synchronize()
    assert rc == 0
    return SP.host_u32(data), SP.host_u32(totals)


def _random(n, limit, seed, rows=1):
    return np.random.default_rng(seed).integers(0, limit, size=(rows, n), dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("name", SCANS)
def test_scan_every_size_written_and_total_alone(name, values):
    _, waves, vpt = SCANS[name]
    for n in _sizes(waves, vpt):
        rows = _random(n, VALUES[values], seed=n + 1)
        want, total = WR.exclusive_scan(rows)
        for write in (True, False):
            got, totals = _scan(name, rows, 1 if write else 0)
            assert (got[:, :n] == (want if write else rows)).all(), (name, n, write)
            assert (got[:, n:] == TAIL_WORD).all(), (name, n, write, "words at i >= n were touched")
            assert (totals == total[:, None]).all(), (name, n, write, "not every thread got the total")


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("name", SCANS)
def test_written_scan_then_total_alone_on_the_same_lds(name, values):
    """k_scans: a `write` scan of one array, then the total alone of another, the same s_wave handed in both times"""
    _, waves, vpt = SCANS[name]
    step = 64 * waves * vpt
    for n in (1, step, step + 1, 2 * step + 1, 3 * step + 1):
        rows = _random(n, VALUES[values], seed=7 * n, rows=2)
        want, total = WR.exclusive_scan(rows)
        got, totals = _scan(name, rows, 0b01)
        assert (got[0, :n] == want[0]).all() and (got[1, :n] == rows[1]).all(), (name, n)
        assert (got[:, n:] == TAIL_WORD).all(), (name, n)
        assert (totals == total[:, None]).all(), (name, n)


def _wg_of_column(n, per):
    """hist1_wg_of_column (common.h) as the device evaluates it"""
    out = torch.full((n,), -1, dtype=torch.int32, device=SP.DEV)
    rc = SP.lib().pt_hist1_wg_of_column(n, per, SP.ptr(out), SP.stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu().numpy()


# (per, n_wg, columns that must be holes).  The first two are k_scans' own form, n_wg = 8 per - 3: the last column of
# the last three groups has no workgroup -- 4095 is the last element of a one-step row; 8191 the last element of the
# second step.  The third leaves the last few columns of EVERY group without a workgroup; a group of 1366 columns puts
# 4095 (the last element of the first step) and 4096 (the first of the second) among them, and 8191 / 8192 not.
HOLES = [(512, 4093, (4095,)), (1024, 8189, (6143, 7167, 8191)), (1366, 10900, (4095, 4096))]


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("per,n_wg,must", HOLES)
def test_poisoned_holes_under_the_valid_predicate(per, n_wg, must, values):
    n = 8 * per
    valid = _wg_of_column(n, per) < n_wg
    assert not valid[list(must)].any() and valid.sum() == min(n_wg, n), "the holes are not where the case wants them"
    assert valid[0] and 0 < (~valid).sum() < n // 8
    rows = _random(n, VALUES[values], seed=per)
    rows[0, ~valid] = POISON
    want, total = WR.exclusive_scan_valid(rows, valid[None, :])
    for write in (True, False):
        got, totals = _scan("16x4_column_valid", rows, 1 if write else 0, per, n_wg)
        if write:
            assert (got[0, :n][valid] == want[0][valid]).all(), (per, n_wg)
        else:
            assert (got[:, :n] == rows).all(), (per, n_wg)
        assert (got[:, n:] == TAIL_WORD).all()
        assert (totals == total[:, None]).all(), (per, n_wg, write)


def _patterns(seed):
    """[7, 256] bool: all false, all true, lane 63 of each wave, thread 0, thread 255, random, whole waves empty"""
    t = np.arange(256)
    rng = np.random.default_rng(seed)
    waves_empty = rng.random(256) < 0.5
    waves_empty[(t >> 6 == 0) | (t >> 6 == 2)] = False
    return np.stack([np.zeros(256, bool), np.ones(256, bool), (t & 63) == 63, t == 0, t == 255, rng.random(256) < 0.5, waves_empty])


def _rounds(count, rows, with_total=True):
    rows = np.asarray(rows, dtype=np.uint32)
    tin = SP.u32(rows)
    out, total = SP.u32(np.full(rows.shape, 0xFFFFFFFF, np.uint32)), SP.u32(np.full(rows.shape, 0xFFFFFFFF, np.uint32))
    rc = SP.lib().pt_wg_rounds(int(count), rows.shape[0], int(with_total), SP.ptr(tin), SP.ptr(out), SP.ptr(total), SP.stream())
    torch.cuda.synchronize()
    assert rc == 0
    return SP.host_u32(out), SP.host_u32(total)


@pytest.mark.parametrize("with_total", (True, False))
@pytest.mark.parametrize("order", ("as_listed", "reversed"))
def test_exclusive_count_in_rounds_on_alternating_lds(order, with_total):
    p = _patterns(1)
    p = p if order == "as_listed" else p[::-1]
    # a predicate is any non-zero word
    rows = np.where(p, np.random.default_rng(2).integers(1, 1 << 32, size=p.shape, dtype=np.uint64), 0).astype(np.uint32)
    want, total = WR.exclusive_scan(p.astype(np.uint32))
    got, totals = _rounds(True, rows, with_total)
    assert (got == want).all()
    assert (totals == (total[:, None] if with_total else 0xFFFFFFFF)).all()


@pytest.mark.parametrize("with_total", (True, False))
@pytest.mark.parametrize("values", VALUES)
def test_exclusive_sum_in_rounds_on_alternating_lds(values, with_total):
    p = _patterns(3)
    rows = np.where(p, _random(256, VALUES[values], seed=4, rows=len(p)), 0).astype(np.uint32)
    rows = np.concatenate([rows, _random(256, VALUES[values], seed=5, rows=2)])    # and every thread with a value
    want, total = WR.exclusive_scan(rows)
    got, totals = _rounds(False, rows, with_total)
    assert (got == want).all()
    assert (totals == (total[:, None] if with_total else 0xFFFFFFFF)).all()


@pytest.mark.parametrize("values", ("below_2_16", "near_2_31"))
def test_total_of_the_counts_before_each_workgroup_and_total(values):
    """Workgroup b asks for counts[0 .. b): one launch of 1001 workgroups has every n of 0 .. 1000, with 0, 1, 255, 256,
    257 and 1000 among them; beside it wg_total of the workgroup's own row of values on the second LDS set."""
    grid = 1001
    rng = np.random.default_rng(6)
    if values == "below_2_16":
        counts = rng.integers(0, 1 << 16, size=grid, dtype=np.uint64).astype(np.uint32)
    else:                          # two of them already wrap
        counts = rng.integers((1 << 31) - 1000, (1 << 31) + 1000, size=grid, dtype=np.uint64).astype(np.uint32)
    rows = _random(256, 1 << 32 if values == "near_2_31" else 1 << 16, seed=8, rows=grid)
    of, tot = SP.u32(np.full((grid, 256), 0xFFFFFFFF, np.uint32)), SP.u32(np.full((grid, 256), 0xFFFFFFFF, np.uint32))
    d_counts, d_rows = SP.u32(counts), SP.u32(rows)
    rc = SP.lib().pt_wg_totals(grid, SP.ptr(d_counts), SP.ptr(d_rows), SP.ptr(of), SP.ptr(tot), SP.stream())
    torch.cuda.synchronize()
    assert rc == 0
    before, _ = WR.exclusive_scan(counts)
    of, tot = SP.host_u32(of), SP.host_u32(tot)
    for n in (0, 1, 255, 256, 257, 1000):
        assert (of[n] == before[n]).all(), n
    assert (of == before[:, None]).all()
    assert (tot == WR.exclusive_scan(rows)[1][:, None]).all()
