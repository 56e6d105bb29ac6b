"""The restatements against RECORDED behaviour of the reference's own kernels (tests/golden/reference/*.npz, written on
an MI355X by tests/golden/make_reference_goldens.py from the strict builds of oracle/_ref): KR.mean_dist3_numpy,
GR.forward and GR.backward (grad_inputs) reproduce the records bit for bit.  Needs neither a GPU nor the reference tree;
the inputs are regenerated from the seeds of tests/reference_cases.py."""
import os

import numpy as np
import pytest

import grid_reference as GR
import knn_reference as KR
import reference_cases as RC

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _load(name):
    path = os.path.join(GOLDEN, name)
    assert os.path.getsize(path) <= 1 << 20
    return np.load(path)


@pytest.mark.parametrize("kind", RC.KNN_KINDS)
def test_knn_restatement_reproduces_the_recorded_reference(kind):
    rec = _load("reference_knn.npz")
    for P in RC.KNN_GOLDEN_SIZES:
        want = rec[f"out_{kind}_{P}"]
        assert want.shape == (P,) and want.dtype == F32
        assert _bits_equal(KR.mean_dist3_numpy(RC.knn_cloud(kind, P)), want), (kind, P)


def test_knn_records_are_complete():
    rec = _load("reference_knn.npz")
    assert sorted(rec.files) == sorted(f"out_{k}_{P}" for k in RC.KNN_KINDS for P in RC.KNN_GOLDEN_SIZES)


@pytest.mark.parametrize("F", RC.GRID_FEATURES)
@pytest.mark.parametrize("D", RC.GRID_DIMS)
def test_grid_restatement_reproduces_the_recorded_reference(D, F):
    rec = _load(f"reference_grid_d{D}.npz")
    offs, r, emb, x, g = RC.golden_grid_case(D, F)
    N, L = x.shape[0], len(r)
    # the case holds what it is meant to hold: out-of-range points, exact 0 and 1, subnormal inputs
    assert (x < 0).any() and (x > 1).any() and (x == 0).any() and (x == 1).any() and (x == F32(2.0 ** -149)).any()
    out, dy = GR.forward(x, emb, offs, r)
    assert rec[f"outputs_f{F}"].shape == (L, N, F) and rec[f"dy_dx_f{F}"].shape == (N, L, D, F)
    assert _bits_equal(out, rec[f"outputs_f{F}"]), (D, F)
    assert _bits_equal(dy, rec[f"dy_dx_f{F}"]), (D, F)
    _, gin, _ = GR.backward(x, offs, r, emb.shape[0], g, rec[f"dy_dx_f{F}"])
    assert _bits_equal(gin, rec[f"grad_inputs_f{F}"]), (D, F)
    assert np.abs(rec[f"outputs_f{F}"]).max() > 0 and np.abs(rec[f"grad_inputs_f{F}"]).max() > 0


def test_double_half_of_the_reference_rounds_like_the_fp32_half():
    """The reference computes pos = x * float(res - 2) + 0.5 with a double 0.5: the fp32 product is widened, the sum taken
    in double and narrowed.  The header and GR._cell add F32(0.5).  The two agree for every non-negative fp32 product:
    below 2^-25 both give 0.5 (the double sum may land on the fp32 tie 0.5 + 2^-25, which goes to even: 0.5); from 2^-25 up
    the product's last bit is at 2^-48 or above, so the double sum is exact and is rounded once.  Checked on every fp32
    product of the binades 2^-27 .. 2^-22 (around the first tie), on the subnormals' ends, and on a random sample."""
    half32, half64 = F32(0.5), np.float64(0.5)
    def same(p):
        a = p + half32
        b = (p.astype(np.float64) + half64).astype(F32)
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for e in range(-27, -21):
        bits = (np.uint32(e + 127) << np.uint32(23)) + np.arange(1 << 23, dtype=np.uint32)
        assert same(bits.view(F32)), e
    assert same(np.arange(0, 1 << 16, dtype=np.uint32).view(F32))                      # +0 and the smallest subnormals
    rng = np.random.default_rng(0)
    assert same(rng.integers(0, 0x47000000, 1 << 22, dtype=np.uint32).view(F32))       # 0 .. 32768: any product of [0, 1] x res
    assert same((rng.uniform(0, 1, 1 << 22).astype(F32) * F32(3000 - 2)))
