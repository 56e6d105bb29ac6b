"""The ORDER of the weight-gradient sums that include/bloomscene_heads.h and include/bloomscene_context.h promise, pinned
against numpy: per range of 256 rows the products are added in fp64 with the rows ascending and rounded to fp32 once, the
ranges are added in fp64 in ascending order and rounded to fp32 once.

Two calls are predictable exactly without restating a kernel.  With g_scale_rot as the only upstream of the heads, dpre2
of the cov head is the upstream itself and its hid is relu of the pre1 columns that anchor_heads_maps returns; with
g_context as the only upstream of the context head, dpre2 is g_context in all O columns and hid is relu(pre1) of
context_head_maps (both pre1 are pinned bit for bit in test_heads_gpu.py / test_context_gpu.py).  So dW2 = dpre2^T hid and
db2 = the column sums of dpre2 follow in numpy float64, where the product of two fp32 values is exact: `acc + a * b` is
the kernel's fma.

Benign inputs hide the order behind the fp32 rounding, so the upstream cancels (`cancelling_rows`): rows come in twins
with the same input row, hence the same hid; every other twin carries +B and -B of about 2^30 and the rows between them
are of order 1, so a range's sum is what the fp64 accumulator kept of the small rows while it stood at 2^30.  In column 0 a
twin of 2^40 sits astride the first two ranges: their partials cancel exactly if they are rounded to fp32 and added first.
test_the_inputs_tell_the_orders_apart checks here, in numpy alone, that rows descending, ranges descending, partials kept
in fp64 and a range of 128 or 512 rows each change predicted bits.

Rows: 515 (three ranges, the last of 3 rows, a partial last workgroup of the row pass) and 256 (exactly one range); widths
that are no multiples of 4 (the 4 x 4 edge blocks; the bias sums of the blocks in the first column)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import context_reference as CR
import heads_reference as HR

DEV = "cuda:0"
CHUNK = 256
ROWS = (515, 256)
HEADS_SHAPE = (6, 3)              # F, K: W2 of the cov head is [21, 6]
CONTEXT_SHAPE = (10, 6, 5, 2)     # D, H, F, K: W2 is [37, 6]


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sums(a, b, chunk=CHUNK, rows_descending=False, ranges_descending=False, round_partials=True):
    """a [n, J], b [n, Kd] fp32 -> dW [J, Kd] = a^T b and db [J] = the column sums of a, fp32, in the headers' order"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    partials = []
    for r0 in range(0, len(a), chunk):
        rows = list(range(r0, min(r0 + chunk, len(a))))
        acc, ab = np.zeros((a.shape[1], b.shape[1])), np.zeros(a.shape[1])
        for r in (rows[::-1] if rows_descending else rows):
            acc = acc + a64[r][:, None] * b64[r][None, :]
            ab = ab + a64[r]
        if round_partials:
            acc, ab = acc.astype(np.float32).astype(np.float64), ab.astype(np.float32).astype(np.float64)
        partials.append((acc, ab))
    if ranges_descending:
        partials = partials[::-1]
    dW, db = partials[0]
    for acc, ab in partials[1:]:
        dW, db = dW + acc, db + ab
    return dW.astype(np.float32), db.astype(np.float32)


def cancelling_rows(n, width, seed):
    """-> the upstream [n, width] and `twin`: row r of the inputs is to be row twin[r] (see the module's docstring)"""
    g = torch.Generator().manual_seed(seed)
    up = torch.randn(n, width, generator=g)
    twin = np.arange(n)
    twin[1::2] = twin[1::2] - 1
    for r in range(0, n - 1, 4):
        big = torch.randn(width, generator=g) * 2.0 ** 30
        up[r], up[r + 1] = big, -big
    if n > CHUNK + 2:                 # rows 2 and CHUNK + 2 are small rows of their ranges
        twin[CHUNK + 2] = 2
        huge = float(torch.randn((), generator=g)) * 2.0 ** 40
        up[2, 0], up[CHUNK + 2, 0] = huge, -huge
    return up, twin


def _relu(pre):
    return np.where(pre > 0, pre, np.float32(0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _heads_scene(n):
    F, K = HEADS_SHAPE
    s = HR.scene(n, F, K, seed=n)
    up, twin = cancelling_rows(n, 7 * K, seed=n)
    s.feat, s.anchor, s.up = s.feat[twin].contiguous(), s.anchor[twin].contiguous(), up
    return s


@functools.lru_cache(maxsize=None)
def _context_scene(n):
    D, H, F, K = CONTEXT_SHAPE
    s = CR.scene(n, D, H, F, K, seed=n)
    up, twin = cancelling_rows(n, s.O, seed=n + 1)
    s.enc, s.up = s.enc[twin].contiguous(), up
    return s


def _operands(unit, n):
    """dpre2 and hid of the predictable product, from the numpy chains (the bits of the kernels' maps)"""
    if unit == "heads":
        s = _heads_scene(n)
        pre1 = HR.forward_np(s.feat.numpy(), s.anchor.numpy(), s.cam.numpy(), [w.numpy() for w in s.weights], s.K).pre1
        return s.up.numpy(), _relu(pre1[:, s.F:2 * s.F])
    s = _context_scene(n)
    return s.up.numpy(), _relu(CR.forward_np(s.enc.numpy(), [w.numpy() for w in s.weights], s.F, s.K, s.q).pre1)


@pytest.mark.parametrize("unit", ("heads", "context"))
def test_the_inputs_tell_the_orders_apart(unit):
    a, b = _operands(unit, ROWS[0])
    dW, db = sums(a, b)
    differs = lambda **kw: [int((_bits(x) != _bits(y)).sum()) for x, y in zip(sums(a, b, **kw), (dW, db))]
    assert np.isfinite(dW).all() and np.isfinite(db).all()
    for kw in (dict(rows_descending=True), dict(ranges_descending=True), dict(round_partials=False), dict(chunk=128), dict(chunk=512)):
        changed = differs(**kw)
        print(f"[wgrad order] {unit} {kw}: {changed[0]} of {dW.size} dW2 and {changed[1]} of {db.size} db2 elements change")
        assert changed[0] > 0 and changed[1] > 0, (unit, kw, changed)
    a, b = _operands(unit, ROWS[1])      # one range: the order of the rows alone
    one = sums(a, b)
    assert all((_bits(x) != _bits(y)).any() for x, y in zip(sums(a, b, rows_descending=True), one))


def _leaf(t, grad=False):
    return t.to(DEV).clone().requires_grad_(grad)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_heads_sum_the_rows_in_the_headers_order(n):
    import bloomscene_amd.heads as H
    s = _heads_scene(n)
    F, K = s.F, s.K
    weights = [_leaf(w, True) for w in s.weights]
    feat, anchor, cam, mask = _leaf(s.feat), _leaf(s.anchor), s.cam.to(DEV), _leaf(s.mask)
    pre1 = H.anchor_heads_maps(feat, anchor, cam, [w.detach() for w in weights], K, offset_mask=mask)[3].cpu().numpy()
    scale_rot = H.anchor_heads_tensors(feat, anchor, cam, weights, K, offset_mask=mask)[2]
    (scale_rot * s.up.reshape(n * K, 7).to(DEV)).sum().backward()
    dW, db = sums(s.up.numpy(), _relu(pre1[:, F:2 * F]))
    assert dW.shape == (7 * K, F)
    assert (_bits(weights[6].grad) == _bits(dW)).all(), "cov.W2"
    assert (_bits(weights[7].grad) == _bits(db)).all(), "cov.b2"
    for i in (2, 3, 10, 11):             # the heads without an upstream
        assert not weights[i].grad.any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_context_sums_the_rows_in_the_headers_order(n):
    import bloomscene_amd.context as Cx
    s = _context_scene(n)
    weights = [_leaf(w, True) for w in s.weights]
    enc = _leaf(s.enc)
    pre1 = Cx.context_head_maps(enc, [w.detach() for w in weights], s.F, s.K)[5].cpu().numpy()
    context = Cx.context_head_tensors(enc, weights, s.F, s.K)[0]
    (context * s.up.to(DEV)).sum().backward()
    dW, db = sums(s.up.numpy(), _relu(pre1))
    assert dW.shape == (s.O, s.H)
    assert (_bits(weights[2].grad) == _bits(dW)).all(), "W2"
    assert (_bits(weights[3].grad) == _bits(db)).all(), "b2"
