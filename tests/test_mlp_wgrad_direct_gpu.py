"""csrc/mlp_wgrad.{h,hip} on its own: the product's unit, compiled unchanged into tests/native/libbsr_shared_pieces.so,
behind an entry point that builds MlpSegments / MlpProducts through their `add` members and calls mlp_wgrad_layout,
mlp_wgrad_carve and mlp_wgrad_sums (n == 0: mlp_wgrad_zero) the way heads.hip and context.hip do.  dW and db must be
BIT-equal to sums() of test_mlp_wgrad_order.py -- the order the public headers promise -- on the cancelling inputs of that
module, with larger twins (_cancelling), which show the row order, the range order, the fp32 rounding of the partials and
the range length in the bits (test_the_inputs_tell_the_orders_apart_at_these_shapes checks that here, without a GPU).

What test_mlp_wgrad_order.py cannot reach through the ops (it pins [21, 6] and [37, 6], each the last product of its
unit, every segment asked for):
  * one product of (J, Kd) = (1, 1), (3, 2), (4, 4), (5, 7), (17, 9): J or Kd below 4, exact and ragged 4 x 4 edge blocks;
  * four products in one launch, the unit-to-product search at its boundaries (96 | 8 | 24 | 8 units), with the segments
    listed in another order than the products, so that `out` / `bout` are no running sums;
  * the same with a first product of 368 units: 448 in all, blockIdx.y == 1 runs and three boundaries lie inside it;
  * the heads' own table form, 12 segments with W1 of three heads as ONE stacked product over three segments, the second
    weight segment and one bias segment not asked for (NULL); a guard word behind every destination must stay;
  * rows: 0 (every asked gradient exactly +0), 1, 255, 256, 257 and 515;
  * NaN in every padding float of the rows (the pitches are mlp_wgrad_layout's own): the 16-byte loads read them, the
    edge masks must keep them out of what is stored."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import shared_pieces as SP
from test_mlp_wgrad_order import CHUNK, _bits, sums

X, HID, DP1, DP2 = 0, 1, 2, 3      # the row arrays of MlpRowScratch
ROWS = (0, 1, 255, 256, 257, 515)
GUARD = 0x7FC12345


def _single(J, Kd):
    """A = columns 3 .. of dp2, B = columns 1 .. of hid (starts that are no multiples of 4, as heads_offset gives)"""
    return dict(widths=(2, Kd + 1, J + 3), segments=[J * Kd, J], null=(), products=[(DP2, 3, HID, 1, J, Kd, 0, 1)])


def _four(wx, f):
    """layer 1 of three heads stacked over the shared x, layer 2 head by head: (A array, A column, B array, B column,
    J, Kd, weight segment, bias segment); the segments are b3, W2, W0, b1, W3, b0, W1, b2"""
    return dict(widths=(wx, 3 * f, 33), null=(),
                segments=[5, 21 * f, 3 * f * wx, 7, 5 * f, 3 * f, 7 * f, 21],
                products=[(DP1, 0, X, 0, 3 * f, wx, 2, 5), (DP2, 0, HID, 0, 7, f, 6, 3), (DP2, 7, HID, f, 21, f, 1, 7),
                          (DP2, 28, HID, 2 * f, 5, f, 4, 0)])


def _heads_form():
    F, outs = 6, (3, 21, 9)
    segments = [F * (F + 4)] * 3 + [F] * 3 + [o * F for o in outs] + list(outs)
    products = [(DP1, 0, X, 0, 3 * F, F + 4, 0, 3)]
    products += [(DP2, sum(outs[:h]), HID, h * F, outs[h], F, 6 + h, 9 + h) for h in range(3)]
    return dict(widths=(F + 4, 3 * F, sum(outs)), segments=segments, null=(1, 10), products=products)


TABLES = {
    "1x1": _single(1, 1), "3x2": _single(3, 2), "4x4": _single(4, 4), "5x7": _single(5, 7), "17x9": _single(17, 9),
    "four_products": _four(30, 15),
    "four_products_448_units": _four(61, 30),
    "heads_form_12_segments": _heads_form(),
}


def _units(table):
    return [((p[4] + 3) // 4) * ((p[5] + 3) // 4) for p in table["products"]]


def _cancelling(n, width, rng):
    """cancelling_rows of test_mlp_wgrad_order.py with larger twins, so that ONE element shows an order (a product here
    may have no more): rows of order 1; rows r, r + 1 of every four carry +B, -B of about 2^45, so the fp64 accumulator
    keeps the small rows to 2^-7 while it stands there -- far above the fp32 rounding of the result; and in every third
    column rows 2 and CHUNK + 2 carry +H, -H of about 2^50 (fp64 keeps the small rows to 2^-2 beside it, fp32 nothing): two
    partials that cancel exactly once rounded to fp32 and added first.  (The other columns keep the first two ranges in sight at n > CHUNK + 2.)"""
    up = rng.standard_normal((n, width)).astype(np.float32)
    for r in range(0, n - 1, 4):
        big = (rng.standard_normal(width) * 2.0 ** 45).astype(np.float32)
        up[r], up[r + 1] = big, -big
    if n > CHUNK + 2:
        huge = (rng.standard_normal(width) * 2.0 ** 50).astype(np.float32)
        third = np.arange(width) % 3 == 0
        up[2, third], up[CHUNK + 2, third] = huge[third], -huge[third]
    return up


@functools.lru_cache(maxsize=None)
def _rows(name, n):
    """-> the four row arrays [n, width]: dp1 and dp2 cancel, x and hid repeat a row in its twin (rows r and r + 1 of
    every four; CHUNK + 2 and 2), so that the products of a +B and its -B cancel exactly"""
    wx, wh, w2 = TABLES[name]["widths"]
    rng = np.random.default_rng([sorted(TABLES).index(name), n])
    twin = np.arange(n)
    twin[1::2] -= 1
    if n > CHUNK + 2:
        twin[CHUNK + 2] = 2
    x, hid = (rng.standard_normal((n, w)).astype(np.float32)[twin] for w in (wx, wh))
    return x, hid, _cancelling(n, wh, rng), _cancelling(n, w2, rng)


def _partial(name, n, **order):
    """-> the tot elements of the summed partial in the headers' order (or in a wrong one), and first[] of the segments"""
    t = TABLES[name]
    first = np.concatenate([[0], np.cumsum(t["segments"])]).astype(int)
    arrays = _rows(name, n)
    want, written = np.zeros(first[-1], dtype=np.float32), np.zeros(first[-1], dtype=int)
    for (a_arr, a_col, b_arr, b_col, J, Kd, w, b) in t["products"]:
        dW, db = sums(arrays[a_arr][:, a_col:a_col + J], arrays[b_arr][:, b_col:b_col + Kd], **order)
        want[first[w]:first[w] + J * Kd], want[first[b]:first[b] + J] = dW.ravel(), db
        written[first[w]:first[w] + J * Kd] += 1
        written[first[b]:first[b] + J] += 1
    assert (written == 1).all(), "the products of a table write every element of a partial once"
    return want, first


@functools.lru_cache(maxsize=None)
def _want(name, n):
    return _partial(name, n)


def test_the_tables_are_what_the_docstring_says():
    assert _units(TABLES["four_products"]) == [96, 8, 24, 8]
    assert _units(TABLES["four_products_448_units"]) == [368, 16, 48, 16]
    assert len(TABLES["heads_form_12_segments"]["segments"]) == 12
    assert [_units(TABLES[k]) for k in ("1x1", "3x2", "4x4", "5x7", "17x9")] == [[1], [1], [1], [4], [15]]


@pytest.mark.parametrize("name", TABLES)
def test_the_inputs_tell_the_orders_apart_at_these_shapes(name):
    """as test_mlp_wgrad_order.test_the_inputs_tell_the_orders_apart: every wrong order changes bits in dW and in db of
    EVERY product of the table (a 1 x 1 product: in its one element)"""
    t = TABLES[name]
    want, first = _want(name, 515)
    assert np.isfinite(want).all()
    wrong_orders = (dict(rows_descending=True), dict(ranges_descending=True), dict(round_partials=False), dict(chunk=128), dict(chunk=512))
    for kw in wrong_orders:
        wrong, _ = _partial(name, 515, **kw)
        for i, (_, _, _, _, J, Kd, w, b) in enumerate(t["products"]):
            dW = int((_bits(wrong) != _bits(want))[first[w]:first[w] + J * Kd].sum())
            db = int((_bits(wrong) != _bits(want))[first[b]:first[b] + J].sum())
            print(f"[wgrad direct] {name} product {i} {kw}: {dW} of {J * Kd} dW and {db} of {J} db elements change")
            assert dW > 0 and db > 0, (name, i, kw)
    one, _ = _want(name, 256)               # one range: the order of the rows alone
    down, _ = _partial(name, 256, rows_descending=True)
    assert (_bits(one) != _bits(down)).any()


def _ints(values):
    return (C.c_int * len(values))(*values)


def _layout(n, wx, wh, w2, tot):
    out = (C.c_size_t * 10)()
    SP.lib().pt_mlp_wgrad_layout(n, wx, wh, w2, tot, out)
    keys = ("ldx", "ldh", "ld2", "chunks", "tot", "off_hid", "off_dp1", "off_dp2", "off_partials", "floats")
    return dict(zip(keys, (int(v) for v in out)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", TABLES)
def test_sums_bit_equal_to_the_headers_order(name, n):
    t = TABLES[name]
    wx, wh, w2 = t["widths"]
    sizes = t["segments"]
    tot = sum(sizes)
    scratch = None
    if n:
        l = _layout(n, wx, wh, w2, tot)
        assert l["tot"] == tot and l["chunks"] == (n + 255) // 256
        host = np.full(l["floats"], np.nan, dtype=np.float32)      # the padding of every row, the partials, the tail: NaN
        for a, off, ld in zip(_rows(name, n), (0, l["off_hid"], l["off_dp1"], l["off_dp2"]), (l["ldx"], l["ldh"], l["ldh"], l["ld2"])):
            assert ld >= a.shape[1] + 4 and ld % 4 == 0
            host[off:off + n * ld].reshape(n, ld)[:, :a.shape[1]] = a
        scratch = torch.from_numpy(host).to(SP.DEV)
    dst = [None if i in t["null"] else torch.from_numpy(np.full(s + 1, GUARD, dtype=np.uint32).view(np.float32)).to(SP.DEV)
           for i, s in enumerate(sizes)]
    pointers = (C.c_void_p * len(sizes))(*[d.data_ptr() if d is not None else None for d in dst])
    cols = list(zip(*t["products"]))
    rc = SP.lib().pt_mlp_wgrad(n, wx, wh, w2, len(sizes), _ints(sizes), pointers, len(t["products"]), *[_ints(c) for c in cols],
                               SP.ptr(scratch), SP.stream())
    torch.cuda.synchronize()
    assert rc == 0
    want, first = _want(name, n) if n else (np.zeros(tot, dtype=np.float32), np.concatenate([[0], np.cumsum(sizes)]).astype(int))
    for i, d in enumerate(dst):
        if d is None:
            continue
        got = _bits(d)
        assert got[-1] == GUARD, (name, n, i, "the word behind the destination")
        assert (got[:-1] == _bits(want[first[i]:first[i + 1]])).all(), (name, n, "segment", i)
