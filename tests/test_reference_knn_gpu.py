"""mean_dist3 (include/bloomscene_knn.h) against the reference's OWN kernels: submodules/simple-knn compiled for gfx950 by
oracle/reference_build.py and loaded by tests/reference_builds.py.  tests/test_knn_gpu.py compares the product with
tests/knn_reference.py, a restatement written from one reading of the reference; this file pins that reading.

Skips only when build() found no reference tree (the manifest says reference_missing).

Exclusions (cases where the reference's result is provably not a function of its input): none.  Its Morton order depends
on what the hardware makes of casting NaN to an integer, but the order only decides which boxes are pruned, and a pruned
box cannot hold one of the three nearest points (`reject` is a third-smallest distance over real candidates; distBoxPoint
is below every distance into its box because rounding is monotonic) -- so every case below is compared.
"""
import time

import numpy as np
import pytest
import torch

import knn_reference as KR
import reference_builds as RB
import reference_cases as RC

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = "cuda:0"
KINDS = RC.KNN_KINDS      # every kind of KR.make_cloud; shared with the recorder and the CPU replay of its records
SIZES = RC.KNN_SIZES
U = 2.0 ** -24


def _ours(xt):
    from bloomscene_amd.knn import mean_dist3
    out = mean_dist3(xt)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _differing(a, b):
    return np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_strict_reference_bit_equal(kind, P):
    RB.skip_if_missing()
    x = RC.knn_cloud(kind, P)
    assert x.shape == (P, 3)
    xt = torch.from_numpy(x).to(DEV)
    ref = RB.ref_mean_dist3(xt, "strict").cpu().numpy()
    got = _ours(xt)
    bad = _differing(ref, got)
    print(f"knn strict {kind} P={P}: {bad.size} of {P} differ")
    assert bad.size == 0, (kind, P, bad.size, bad[:5], ref[bad[:5]], got[bad[:5]])
    if P <= 1000:   # and the restatement itself, without the product in between
        assert _differing(ref, KR.mean_dist3_numpy(x)).size == 0, (kind, P)


def test_strict_reference_bit_equal_at_1m():
    """uniform at 10^6: the largest cloud tests/test_knn_gpu.py uses.  The size stands as long as the reference does it in
    less time than that whole file takes on the same machine.  Measured on one MI355X: the reference 0.026 s, the whole of
    tests/test_knn_gpu.py 45 s.  The reference's time is printed."""
    RB.skip_if_missing()
    P = 1_000_000
    x = KR.make_cloud("uniform", P, seed=1)
    xt = torch.from_numpy(x).to(DEV)
    RB.ref_mean_dist3(xt[:2000].contiguous(), "strict")   # code object loaded
    t0 = time.perf_counter()
    ref = RB.ref_mean_dist3(xt, "strict").cpu().numpy()
    dt = time.perf_counter() - t0
    got = _ours(xt)
    bad = _differing(ref, got)
    print(f"knn strict uniform P={P}: {bad.size} differ; the reference took {dt:.3f} s")
    assert bad.size == 0, (bad.size, bad[:5], ref[bad[:5]], got[bad[:5]])


@pytest.mark.parametrize("P", [4, 7, 64, 1000, 20000])
@pytest.mark.parametrize("kind", [k for k in KINDS if k != "nonfinite"])
def test_contract_reference_within_rounding(kind, P):
    """The contract build (the compiler may fuse a multiply into the add that follows) against the product:

        |ref - ours| <= ((1 + 2u)^6 - 1) ours  =  12 u ours + O(u^2),   u = 2^-24       (k = 12)

    Derivation.  Both sides start from the same dx, dy, dz (one correctly rounded subtraction each, identical on both
    sides, never fused: a difference feeds a product, not a sum).  From there every quantity is a sum of non-negative
    terms, so a rounding (1 + e), |e| <= u / (1 + u), of an intermediate moves the result by at most that factor.
      * d = dx dx + dy dy + dz dz: in source order the first term passes 1 product and 2 sums, 3 roundings; fused, it passes
        1 product and 2 fma, 3 roundings again; no term passes more.  So d is within (1 + e)^3 of its exact value on either
        side, provided no product underflows or overflows: the test asserts that the smallest non-zero coordinate
        difference of the cloud is above 1e-18 (its square is a normal number) and the largest coordinate below 2.1e6.
      * the three smallest: the k-th smallest of a set whose elements each moved by a factor within [1/c, c] moved by a
        factor within [1/c, c].  The d(i, i) the reference skips and the d < FLT_MAX of the header reject the same pairs.
      * (s0 + s1) + s2: 2 roundings.  / 3: 1 rounding.
    Six roundings a side: ref / exact and ours / exact are within [(1 - u/(1+u))^6, (1 + u/(1+u))^6], so
    ref / ours <= ((1 + u/(1+u)) / (1 - u/(1+u)))^6 = (1 + 2u)^6, and the same for ours / ref.  The comparison is
    evaluated in float64.  P < 4 has FLT_MAX paddings in the sum (inf on both sides): left to the strict test.
    """
    RB.skip_if_missing()
    x = RC.knn_cloud(kind, P)
    assert np.isfinite(x).all() and float(np.abs(x).max()) < 2.1e6
    for a in range(3):
        gaps = np.diff(np.unique(x[:, a]))
        assert gaps.size == 0 or float(gaps.min()) > 1e-18
    xt = torch.from_numpy(x).to(DEV)
    ref = RB.ref_mean_dist3(xt, "contract").cpu().numpy().astype(np.float64)
    got = _ours(xt).astype(np.float64)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    bound = ((1.0 + 2.0 * U) ** 6 - 1.0) * got
    err = np.abs(ref - got)
    worst = float((err / np.maximum(got, 1e-300)).max() / U) if (got > 0).any() else 0.0
    print(f"knn contract {kind} P={P}: max |ref - ours| / (u ours) = {worst:.3f} (bound 12), "
          f"{int((ref != got).sum())} of {P} differ")
    assert (err <= bound).all(), (kind, P, worst)
