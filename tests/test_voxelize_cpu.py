"""Voxel unique, CPU side (include/bloomscene_voxelize.h): the restatement of tests/voxel_reference.py against
np.unique / torch.unique and hand-written cases, the key packing at every width class, voxelize_sample against GM:437
written out, the header / ctypes table / library agreement, the scratch size function, and the Python layer's import
and error order without a GPU.  Every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import voxel_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = VR.I32_MIN, VR.I32_MAX


def _np_unique(coords):
    return np.unique(coords, axis=0, return_index=True, return_inverse=True, return_counts=True)


def _check_against_numpy_and_torch(coords):
    coords = np.asarray(coords, np.int32).reshape(-1, 3)
    got = VR.voxel_unique_ref(coords)
    u, first, inverse, counts = _np_unique(coords)
    assert np.array_equal(got[0], u) and got[0].dtype == np.int32
    assert np.array_equal(got[1], np.asarray(inverse).reshape(-1))
    assert np.array_equal(got[2], first) and np.array_equal(got[3], counts)
    tu, tinv, tcnt = torch.unique(torch.from_numpy(coords), dim=0, return_inverse=True, return_counts=True)
    assert np.array_equal(got[0], tu.numpy()) and np.array_equal(got[1], tinv.numpy())
    assert np.array_equal(got[3], tcnt.numpy())
    return got


@pytest.mark.parametrize("E,span", [(1, 5), (2, 1), (300, 3), (1000, 40), (4097, 7), (2000, 1 << 20)])
def test_restatement_equals_np_unique_and_torch_unique_on_random_int32(E, span):
    rng = np.random.default_rng(E + span)
    coords = rng.integers(-span, span + 1, (E, 3)).astype(np.int32)
    coords[:, 1] += 1000
    got = _check_against_numpy_and_torch(coords)
    assert np.array_equal(got[0][got[1]], coords) and got[3].sum() == E


def test_hand_written_cases():
    # duplicates only
    c, inv, first, cnt = _check_against_numpy_and_torch([[3, -1, 2]] * 5)
    assert c.tolist() == [[3, -1, 2]] and inv.tolist() == [0] * 5 and first.tolist() == [0] and cnt.tolist() == [5]
    # signed lexicographic order, x first; `first` is the smallest position
    c, inv, first, cnt = _check_against_numpy_and_torch([[1, 0, 0], [-1, 5, 5], [1, 0, 0], [-1, 5, -5], [0, -7, 9], [-1, 5, 5]])
    assert c.tolist() == [[-1, 5, -5], [-1, 5, 5], [0, -7, 9], [1, 0, 0]]
    assert inv.tolist() == [3, 1, 3, 0, 2, 1] and first.tolist() == [3, 1, 4, 0] and cnt.tolist() == [1, 2, 1, 2]
    # INT_MIN / INT_MAX in every axis
    corners = [[a, b, c] for a in (LO, HI, 0) for b in (HI, -1, LO) for c in (0, LO, HI)]
    with pytest.raises(VR.TooWide):
        VR.voxel_unique_ref(corners)                       # 32 + 32 + 32 bits
    c, _, _, _ = _check_against_numpy_and_torch([[LO, 7, 7], [HI, 7, 7], [0, 7, 7], [-1, 7, 7], [HI, 7, 7]])
    assert c[:, 0].tolist() == [LO, -1, 0, HI]
    _check_against_numpy_and_torch([[LO, HI, 0], [HI, LO, 0], [LO, LO, 0], [HI, HI, 0], [LO, HI, 0]])   # 64 bits
    # empty
    c, inv, first, cnt = VR.voxel_unique_ref(np.zeros((0, 3), np.int32))
    assert c.shape == (0, 3) and inv.shape == first.shape == cnt.shape == (0,)


def test_quantisation_ties_go_to_even_and_minus_zero_is_zero():
    x = np.array([[0.5, -0.5, 1.5], [2.5, -1.5, -2.5], [-0.0, 0.0, -0.25], [3.5, 0.49999997, -0.50000006]], np.float32)
    for dtype in (np.float32, np.float64):
        for rule in ("divide", "reciprocal") if dtype == np.float32 else ("divide",):
            q, valid = VR.quantise_ref(x.astype(dtype), 1.0, rule)
            assert valid.all()
            assert q.tolist() == [[0, 0, 2], [2, -2, -2], [0, 0, 0], [4, 0, -1]], (dtype, rule)
    # a voxel size that is a power of two is exact under both rules
    q, _ = VR.quantise_ref(x * np.float32(0.25), 0.25, "reciprocal")
    assert q.tolist() == [[0, 0, 2], [2, -2, -2], [0, 0, 0], [4, 0, -1]]
    # -0 and +0 are one voxel
    n_bad, res = VR.unique_rows_ref(np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.2, 0.2, 0.1]], np.float32), 1.0)
    assert n_bad == 0 and res[0].tolist() == [[0, 0, 0]] and res[3].tolist() == [3]


def test_validity_rule():
    s = 1.0
    x = np.zeros((7, 3), np.float32)
    x[1, 0] = np.nan
    x[2, 1] = np.inf
    x[3, 2] = -np.inf
    x[4, 0] = 2.0 ** 31                   # one past INT_MAX: invalid
    x[5, 0] = -2.0 ** 31                  # INT_MIN itself: valid
    x[6, 1] = np.float32(2.0 ** 31 - 128)  # the largest float32 below 2^31: valid
    q, valid = VR.quantise_ref(x, s)
    assert valid.tolist() == [True, False, False, False, False, True, True]
    assert q[5, 0] == LO and q[6, 1] == 2 ** 31 - 128 and (q[1:5] == 0).all()
    xd = x.astype(np.float64)
    xd[6, 1] = 2.0 ** 31 - 0.75           # rounds to 2^31 - 1 in float64
    xd[0, 2] = 2.0 ** 31 - 0.5            # a tie that rounds to 2^31: invalid
    q, valid = VR.quantise_ref(xd, s)
    assert valid.tolist() == [False, False, False, False, False, True, True] and q[6, 1] == HI
    assert VR.unique_rows_ref(x, s)[0] == 4 and VR.unique_rows_ref(x, s)[1] is None
    # rows entries outside the source are invalid and never dereferenced
    pts = np.arange(12, dtype=np.float32).reshape(4, 3)
    assert VR.unique_rows_ref(pts, s, rows=[0, -1, 3, 4, 2 ** 40])[0] == 3
    n_bad, res = VR.unique_rows_ref(pts, 3.0, rows=[3, 0, 3, 1])
    assert n_bad == 0 and res[1].tolist() == [2, 0, 2, 1] and res[2].tolist() == [1, 3, 0]


def test_the_two_rules_differ_on_a_seeded_sample():
    """x / s and x * (1 / s) are different functions: a test that confuses them cannot pass."""
    rng = np.random.default_rng(20)
    x = (rng.random((1_000_000, 3)) * 2.0).astype(np.float32)
    for s in (0.001, 0.004, 0.016):
        a, va = VR.quantise_ref(x, s, "divide")
        b, vb = VR.quantise_ref(x, s, "reciprocal")
        assert va.all() and vb.all()
        differ = int((a != b).any(axis=1).sum())
        assert differ < 1000, (s, differ)                # some tens of every million points at the finest level,
        assert differ > 0 or s > 0.001, (s, differ)      # fewer at the coarser ones (the quotients are smaller)
        assert np.abs(a.astype(np.int64) - b).max() <= 1
    # and on points placed at the boundaries they differ often
    xb = VR.boundary_points(20000, (0.001, 0.004, 0.016), seed=3)
    a, _ = VR.quantise_ref(xb, 0.004, "divide")
    b, _ = VR.quantise_ref(xb, 0.004, "reciprocal")
    assert (a != b).any(axis=1).sum() > 100


@pytest.mark.parametrize("bits", [(0, 0, 0), (3, 5, 0), (0, 8, 0), (2, 3, 4), (9, 0, 0), (1, 0, 32), (11, 11, 11),
                                  (20, 21, 22), (31, 32, 0), (0, 32, 32), (32, 0, 32), (32, 32, 0), (22, 21, 21)])
def test_packed_key_order_is_lexicographic_order(bits):
    assert sum(bits) in (0, 8, 9, 33, 63, 64)
    rng = np.random.default_rng(sum(bits) * 7 + bits[0])
    c = VR.case_with_bits(bits, rng)
    keys, mins, got_bits = VR.pack_keys(c)
    assert tuple(got_bits) == tuple(bits)
    assert np.array_equal(VR.unpack_keys(keys, mins, got_bits), c)
    lex = np.lexsort((c[:, 2], c[:, 1], c[:, 0]))        # ascending signed (x, y, z)
    by_key = np.argsort(keys, kind="stable")
    assert np.array_equal(c[lex], c[by_key])
    # ... strictly: equal keys <=> equal rows
    a, b = c[by_key][1:], c[by_key][:-1]
    assert np.array_equal((keys[by_key][1:] != keys[by_key][:-1]), (a != b).any(axis=1))
    _check_against_numpy_and_torch(c)


@pytest.mark.parametrize("bits", [(32, 32, 1), (1, 32, 32), (22, 22, 21), (32, 32, 32)])
def test_sixty_five_bits_and_more_are_too_wide(bits):
    c = VR.case_with_bits(bits, np.random.default_rng(1))
    with pytest.raises(VR.TooWide, match=f"= {sum(bits)} key bits"):
        VR.pack_keys(c)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_voxelize_sample_restatement_equals_gm437_in_numpy(dtype):
    rng = np.random.default_rng(5)
    data = (rng.standard_normal((60000, 3)) * 0.05).astype(dtype)
    data[:4] = [[0.0, -0.0, 0.0004], [-0.0004, 0.0005, -0.0005], [0.0015, 0.0025, -0.0015], [0.0, 0.0, 0.0]]
    s = 0.001
    want = VR.voxelize_sample_numpy(data, s)
    got = VR.voxelize_sample_ref(data, s)
    assert got.dtype == want.dtype == dtype and got.shape == want.shape and 1000 < got.shape[0] < 60000
    assert (got == want).all()
    assert not np.signbit(got[got == 0]).any()           # a zero is always +0 (numpy keeps round()'s -0)


def test_header_ctypes_table_and_library_agree():
    from bloomscene_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "bloomscene_voxelize.h")).read()
    declared = set(re.findall(r"\b(bsr_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == {"bsr_voxel_quantise", "bsr_voxel_unique", "bsr_voxel_unique_scratch_bytes"}
    lib = ctypes.CDLL(os.path.join(ROOT, "bloomscene_amd", "libbloomscene_rast.so"))
    for name in declared:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
    # one ctypes argument per declared parameter
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for name in declared:
        params = re.search(name + r"\s*\(([^)]*)\)", flat).group(1)
        assert len(params.split(",")) == len(_capi.SIGNATURES[name][1]), name
    # the constants the Python layer repeats
    from bloomscene_amd import voxelize as V
    consts = dict(re.findall(r"#define (BSR_VOXEL_[A-Z_]+)\s+(0x[0-9a-f]+|\d+)u?", hdr))
    assert [int(consts["BSR_VOXEL_" + n], 0) for n in ("COORDS", "POINTS_F", "POINTS_D", "COMPOSITE")] == \
        [V.FORM_COORDS, V.FORM_POINTS_F, V.FORM_POINTS_D, V.FORM_COMPOSITE]
    assert int(consts["BSR_VOXEL_DIVIDE"], 0) == V.RULES["divide"] and int(consts["BSR_VOXEL_RECIPROCAL"], 0) == V.RULES["reciprocal"]
    assert int(consts["BSR_VOXEL_REFUSED_INVALID"], 0) == V.REFUSED_INVALID and int(consts["BSR_VOXEL_REFUSED_WIDE"], 0) == V.REFUSED_WIDE
    assert int(consts["BSR_VOXEL_FLAG_TEST_SMALL_CHUNK"], 0) == V.FLAG_TEST_SMALL_CHUNK
    assert lib.bsr_version() == 4                        # purely additive


def test_scratch_bytes_monotone_and_aligned():
    lib = ctypes.CDLL(os.path.join(ROOT, "bloomscene_amd", "libbloomscene_rast.so"))
    fn = lib.bsr_voxel_unique_scratch_bytes
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int]
    prev = 0
    for E in [1, 2, 63, 64, 65, 1023, 1024, 1025, 4096, 100_000, 131_072, 131_073, 2_600_000, 10 ** 8, 2 ** 31 - 1]:
        b = fn(E)
        assert b % 256 == 0 and b >= prev and b >= 36 * E, (E, b)    # two (key, payload) buffers and the quantised rows
        assert b <= 36 * E + E // 128 + (4 << 20), (E, b)            # ... the histogram and a word per 1024 rows
        prev = b
    assert fn(0) == 0 and fn(-1) == 0 and fn(-2 ** 31) == 0


def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    from bloomscene_amd import _capi
    lib = _capi.lib()
    none = [None, 3, None, None, 3, 1, None, 0.01]
    assert lib.bsr_voxel_quantise(0, 0, 4, 4, *none, None, None, None) == 1 and "no quantisation" in _capi.last_error()
    assert lib.bsr_voxel_quantise(2, 1, 4, 4, *none, None, None, None) == 1 and "fp32 only" in _capi.last_error()
    assert lib.bsr_voxel_quantise(1, 0, 4, 5, *none, None, None, None) == 1 and "E must equal P" in _capi.last_error()
    assert lib.bsr_voxel_quantise(1, 0, 4, 4, *none, None, None, None) == 1 and "NULL source" in _capi.last_error()
    assert lib.bsr_voxel_unique(7, 0, 4, 4, *none, *[None] * 7, 0, None) == 1 and "unknown form" in _capi.last_error()
    assert lib.bsr_voxel_unique(1, 0, -1, -1, *none, *[None] * 7, 0, None) == 1
    assert lib.bsr_voxel_unique(1, 0, 0, 0, *none, *[None] * 7, 0x1, None) == 1 and "unknown flags" in _capi.last_error()
    assert lib.bsr_voxel_unique(1, 0, 0, 0, *none, *[None] * 7, 0, None) == 0          # E == 0: nothing to do
    assert lib.bsr_voxel_quantise(1, 0, 0, 0, *none, None, None, None) == 0


def test_module_imports_without_a_gpu_and_raises_in_the_siblings_order():
    import bloomscene_amd.voxelize as V
    pts = torch.zeros(6, 3)
    rows = torch.zeros(2, dtype=torch.int64)
    # a wrong dtype first ...
    with pytest.raises(TypeError, match="float32, float64 or int32"):
        V.voxel_unique(torch.zeros(6, 2, dtype=torch.float16), 0.1, rule="reciprocal")
    with pytest.raises(TypeError, match="float32, float64 \\(got torch.int32\\)"):
        V.quantise(torch.zeros(6, 3, dtype=torch.int32), 0.1)
    with pytest.raises(TypeError, match="rows must be int64"):
        V.voxel_unique(pts.double()[:, :2], 0.1, rows=rows.int(), rule="reciprocal")
    with pytest.raises(TypeError, match="torch.Tensor"):
        V.voxel_unique(np.zeros((6, 3), np.float32), 0.1)
    # ... then what is not implemented (on a wrong shape too) ...
    with pytest.raises(NotImplementedError, match="float32 only"):
        V.voxel_unique(pts.double()[:, :2], 0.1, rule="reciprocal")
    with pytest.raises(NotImplementedError, match="float32 only"):
        V.quantise(pts.double(), 0.1, rule="reciprocal")
    # ... then shapes ...
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        V.voxel_unique(pts[:, :2], 0.1)
    with pytest.raises(ValueError, match=r"rows must be \[E\]"):
        V.voxel_unique(pts, 0.1, rows=rows.view(1, 2))
    # ... the device last
    for call in (lambda: V.voxel_unique(pts, 0.1), lambda: V.voxel_unique(pts.int()), lambda: V.quantise(pts.double(), 0.1),
                 lambda: V.voxelize(pts, 0.1), lambda: V.voxel_unique(pts, 0.1, rows=rows)):
        with pytest.raises(ValueError, match="no CPU path"):
            call()
    with pytest.raises(ValueError, match="rule must be"):
        V.quantise(pts, 0.1, rule="floor")
    with pytest.raises(ValueError, match="voxel_size is required"):
        V.voxel_unique(pts)
    with pytest.raises(ValueError, match="finite and not 0"):
        V.voxel_unique(pts, 0.0)
    # voxelize_sample: numpy or tensor
    with pytest.raises(TypeError, match="float32 or float64"):
        V.voxelize_sample(np.zeros((4, 3), np.int32), 0.1)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        V.voxelize_sample(np.zeros((4, 2)), 0.1)
    with pytest.raises(TypeError, match="numpy array or a torch.Tensor"):
        V.voxelize_sample([[0.0, 0.0, 0.0]], 0.1)
    # grow_level
    a, off, sc, feat = torch.zeros(4, 3), torch.zeros(4, 5, 3), torch.ones(4, 6), torch.zeros(4, 8)
    mask = torch.zeros(20, dtype=torch.bool)
    with pytest.raises(TypeError, match="scaling must be float32"):
        V.grow_level(a, off[:, :, :2], sc.double(), mask, feat, 0.1)
    with pytest.raises(TypeError, match="candidate_mask must be bool"):
        V.grow_level(a, off, sc, mask.int(), feat, 0.1)
    with pytest.raises(ValueError, match="K offsets"):
        V.grow_level(a, off[:, :, :2], sc, mask, feat, 0.1)
    with pytest.raises(ValueError, match="scaling must be"):
        V.grow_level(a, off, sc[:, :2], mask, feat, 0.1)
    with pytest.raises(ValueError, match=r"candidate_mask must be \[20\]"):
        V.grow_level(a, off, sc, mask[:19], feat, 0.1)
    with pytest.raises(ValueError, match="no CPU path"):
        V.grow_level(a, off, sc, mask, feat, 0.1)
    # the status words of a refused call
    with pytest.raises(ValueError, match="^who: 3 invalid row"):
        V.raise_status("who", [0, 3, 0, 1, 0, 0, 0, 0])
    with pytest.raises(ValueError, match=r"32 \+ 32 \+ 1 = 65 key bits"):
        V.raise_status("who", [0, 0, 65, 2, 32, 32, 1, 0])
    V.raise_status("who", [5, 0, 17, 0, 6, 6, 5, 0])
