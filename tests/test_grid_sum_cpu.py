"""The condition that keeps tests/test_grid_sum_gpu.py from passing vacuously, in numpy alone: on the inputs that test
uses (grid_sum_reference.cancelling_grid), at every grid it uses and for the three N the losses instantiate, each wrong
order of grid_sum_reference.ORDERS changes bits in EVERY one of the N sums, and the header's order gives finite sums.

Two orders are the header's own sequence of additions at small grids -- a contiguous split of G <= 256 partials over 256
threads gives thread t partial t, as the strided one does, and a tree over G <= 2 partials is the one addition p0 + p1 --
so no input family can tell them apart there (grid_sum_reference.same_sequence).  For exactly those (order, grid) pairs the
assertion is the opposite one: every bit equal, which also pins that the switch is the same sequence and not a third
order.  Every other pair must differ."""
import numpy as np
import pytest

import grid_sum_reference as GR

GRIDS = (1, 2, 255, 256, 257, 513, 1536, 16384)
NS = (1, 2, 5)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_only_inseparable_pairs_are_the_small_grids():
    same = {(o, G) for o in GR.ORDERS for G in GRIDS if GR.same_sequence(o, G)}
    assert same == {("partials_contiguous", G) for G in (1, 2, 255, 256)} | {("partials_pairwise", G) for G in (1, 2)}


@pytest.mark.parametrize("G", GRIDS)
def test_the_inputs_tell_the_orders_apart(G):
    for N in NS:
        x = GR.cancelling_grid(G, N)
        assert np.isfinite(x).all() and (np.abs(x) > 2.0 ** 58).sum() >= 4 * N
        partials = {}                         # (lanes, waves) -> step 1 to 3, shared by the orders that only differ in step 4

        def total(lanes="descending", waves="left", partials_order="strided"):
            if (lanes, waves) not in partials:
                partials[lanes, waves] = GR.workgroup_partials(x, lanes, waves)
            return GR.last_workgroup(partials[lanes, waves], lanes, waves, partials_order)

        right = total()
        assert right.shape == (N,) and np.isfinite(right).all()
        assert (_bits(right) == _bits(GR.grid_sum(x))).all()
        for name, kw in GR.ORDERS.items():
            wrong = total(kw.get("lanes", "descending"), kw.get("waves", "left"), kw.get("partials", "strided"))
            flipped = _bits(right) ^ _bits(wrong)
            sums_changed = int((flipped != 0).sum())
            bits_changed = sum(bin(int(f)).count("1") for f in flipped)
            print(f"[grid sum order] G={G} N={N} {name}: {sums_changed} of {N} sums, {bits_changed} bits change")
            if GR.same_sequence(name, G):
                assert sums_changed == 0, (G, N, name)
            else:
                assert sums_changed == N, (G, N, name, right, wrong)
