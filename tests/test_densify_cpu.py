"""Densification, CPU side (include/bloomscene_densify.h): the restatements of tests/densify_reference.py against
torch's own scatter_reduce and hand-written cases (ties, signed zeros, NaN, infinities, empty groups, entries out of
range), the membership restatement against a set, the torch_scatter shim's import and rejections without a GPU, and
the scratch size function."""
import ctypes
import os

import numpy as np
import pytest
import torch

import densify_reference as DR

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("E,F,G", [(1, 1, 1), (257, 1, 3), (1000, 50, 37), (500, 7, 900)])
def test_restatement_equals_scatter_reduce_amax_on_tie_free_input(E, F, G):
    rng = np.random.default_rng(E + F)
    src = rng.permutation(E * F).astype(F32).reshape(E, F) - F32(E * F // 2)   # all values distinct: no ties, no NaN
    index = rng.integers(0, G, E)
    out, arg = DR.scatter_max_ref(src, index, G)
    t_index = torch.from_numpy(index)[:, None].expand(E, F)
    ref = torch.zeros(G, F).scatter_reduce(0, t_index, torch.from_numpy(src), "amax", include_self=False)
    assert np.array_equal(DR.bits(out), DR.bits(ref))
    # the argmax points at the winner, and empty groups carry E
    filled = arg < E
    assert np.array_equal(filled, np.isin(np.arange(G), index)[:, None].repeat(F, 1))
    gg, ff = np.nonzero(filled)
    assert np.array_equal(src[arg[gg, ff], ff], out[gg, ff]) and (index[arg[gg, ff]] == gg).all()
    assert (out[~filled] == 0).all()


def test_ties_first_row_wins():
    src = np.array([[1, 5], [3, 5], [3, 2], [0, 5]], F32)
    out, arg = DR.scatter_max_ref(src, np.zeros(4, np.int64), 1)
    assert out.tolist() == [[3, 5]] and arg.tolist() == [[1, 0]]


def test_signed_zeros_compare_equal_and_keep_their_bits():
    out, arg = DR.scatter_max_ref(np.array([-0.0, 0.0, -0.0], F32), np.array([0, 0, 1]), 2)
    assert arg.tolist() == [0, 2]
    assert DR.bits(out).tolist() == [0x80000000, 0x80000000]          # the first of (-0, +0) is -0 and stays -0
    out, arg = DR.scatter_max_ref(np.array([0.0, -0.0, -1.0], F32), np.zeros(3, np.int64), 1)
    assert arg.tolist() == [0] and DR.bits(out).tolist() == [0]


def test_nan_is_above_everything_and_the_first_keeps_its_payload():
    src = np.array([1.0, 0.0, INF, 0.0, 2.0], F32)
    b = src.view(np.uint32)
    b[1], b[3] = 0x7fc12345, 0xffc00001          # two NaNs, different payloads and signs
    out, arg = DR.scatter_max_ref(src, np.zeros(5, np.int64), 1)
    assert arg.tolist() == [1] and DR.bits(out).tolist() == [0x7fc12345]
    ref = torch.zeros(1).scatter_reduce(0, torch.zeros(5, dtype=torch.int64), torch.from_numpy(src), "amax",
                                        include_self=False)
    assert torch.isnan(ref).all()                # torch.amax propagates NaN too


def test_infinities():
    src = np.array([-INF, -INF, 3.0, INF, INF, -INF], F32)
    out, arg = DR.scatter_max_ref(src, np.array([0, 0, 1, 1, 1, 2]), 4)
    assert out[:3].tolist() == [-INF, INF, -INF] and arg.tolist() == [0, 3, 5, 6]
    assert DR.bits(out)[3] == 0                  # the empty group: +0.0, argmax == E


def test_empty_groups_and_out_of_range_entries():
    src = np.arange(12, dtype=F32).reshape(6, 2)
    index = np.array([-1, 4, 1, 5, 1, 2 ** 40])
    out, arg = DR.scatter_max_ref(src, index, 5)
    assert arg.tolist() == [[6, 6], [4, 4], [6, 6], [6, 6], [1, 1]]
    assert out.tolist() == [[0, 0], [8, 9], [0, 0], [0, 0], [2, 3]]
    # row_map: contribution e reads row row_map[e]; a row out of range contributes nothing; argmax numbers contributions
    out, arg = DR.scatter_max_ref(src, np.array([0, 0, 0, 1]), 2, row_map=np.array([2, 6, 5, -1]))
    assert out.tolist() == [[10, 11], [0, 0]] and arg.tolist() == [[2, 2], [4, 4]]
    # E == 0
    out, arg = DR.scatter_max_ref(np.zeros((0, 3), F32), np.zeros(0, np.int64), 2)
    assert out.shape == (2, 3) and (out == 0).all() and (arg == 0).all()
    # a dense index whose columns differ
    out, arg = DR.scatter_max_ref(np.array([[1, 2], [3, 4]], F32), np.array([[0, 1], [1, 1]]), 2)
    assert out.tolist() == [[1, 0], [3, 4]] and arg.tolist() == [[0, 2], [1, 1]]


def test_row_map_equals_gathering_first():
    rng = np.random.default_rng(3)
    src = rng.integers(-3, 4, (40, 5)).astype(F32)
    row_map = rng.integers(0, 40, 300)
    index = rng.integers(0, 11, 300)
    a = DR.scatter_max_ref(src, index, 11, row_map=row_map)
    b = DR.scatter_max_ref(src[row_map], index, 11)
    assert np.array_equal(DR.bits(a[0]), DR.bits(b[0])) and np.array_equal(a[1], b[1])


def test_packed_key_order_is_the_headers_order():
    """csrc/densify.hip takes an unsigned maximum of (key, inverted row): the key must order values as the header says."""
    rng = np.random.default_rng(8)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff,
                        0x7f800000, 0xff800000, 0x7f800001, 0xffc00000, 0x7fffffff, 0xffffffff, 0x3f800000, 0xbf800000],
                       np.uint32)
    b = np.concatenate([special, rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)])
    v, k = b.view(F32), DR.order_key(b)
    assert k.min() >= 0x007fffff                      # 0 stays free for "no contribution"
    a, c = np.meshgrid(np.arange(b.size), np.arange(b.size), indexing="ij")
    with np.errstate(invalid="ignore"):
        above = (np.isnan(v[a]) & ~np.isnan(v[c])) | (v[a] > v[c])
    assert np.array_equal(k[a] > k[c], above)
    # and the whole packed route equals the restatement, ties, zeros, NaNs and entries out of range included
    pool = np.array([-1.0, -0.0, 0.0, 1.0, INF, -INF, NAN, 2.5], F32)
    src = pool[rng.integers(0, 8, (600, 5))]
    index = rng.integers(-1, 41, 600)
    row_map = rng.integers(-1, 601, 600)
    for rm in (None, row_map):
        want, got = DR.scatter_max_ref(src, index, 40, rm), DR.scatter_max_packed(src, index, 40, rm)
        assert np.array_equal(DR.bits(want[0]), DR.bits(got[0])) and np.array_equal(want[1], got[1])


def test_voxel_isin_restatement_against_a_set():
    rng = np.random.default_rng(0)
    keys = rng.integers(-5, 6, (400, 3)).astype(np.int32)
    query = rng.integers(-6, 7, (600, 3)).astype(np.int32)
    have = set(map(tuple, keys.tolist()))
    want = np.array([tuple(q) in have for q in query.tolist()])
    assert np.array_equal(DR.voxel_isin_ref(query, keys), want) and 0 < want.sum() < 600
    assert not DR.voxel_isin_ref(query, np.zeros((0, 3), np.int32)).any()
    assert DR.voxel_isin_ref(np.zeros((0, 3), np.int32), keys).shape == (0,)
    lim = np.iinfo(np.int32)
    k = np.array([[lim.min, lim.max, 0]], np.int32)
    assert DR.voxel_isin_ref(np.array([[lim.min, lim.max, 0], [lim.max, lim.min, 0]], np.int32), k).tolist() == [True, False]


def test_growth_restatement_shapes_and_occupancy():
    sizes = (0.01, 0.1, 0.5)
    anchor, all_xyz, mask, feat = DR.make_growth_case(300, 4, 6, seed=1, cur_sizes=sizes)
    m = []
    for s in sizes:
        cand, new_feat = DR.grow_candidates_ref(anchor, all_xyz, mask, feat, s, 4)
        assert cand.dtype == torch.float32 and cand.shape[1] == 3 and tuple(new_feat.shape) == (cand.shape[0], 6)
        m.append(cand.shape[0])
        # no candidate voxel holds an anchor, and every new feature is some anchor's
        occupied = set(map(tuple, torch.round(anchor / s).int().tolist()))
        assert not occupied & set(map(tuple, torch.round(cand / s).int().tolist()))
        assert np.isin(DR.bits(new_feat), DR.bits(feat)).all()
    assert m[0] > m[1] > m[2]      # the coarser the level, the more candidate voxels are occupied already
    none = torch.zeros_like(mask)
    cand, new_feat = DR.grow_candidates_ref(anchor, all_xyz, none, feat, 0.1, 4)
    assert tuple(cand.shape) == (0, 3) and tuple(new_feat.shape) == (0, 6)


def test_torch_scatter_shim_imports_without_a_gpu_and_rejects_bad_input():
    from torch_scatter import scatter_max
    from bloomscene_amd.densify import scatter_max as native_scatter_max, voxel_isin, grow_candidates
    assert callable(scatter_max) and callable(grow_candidates)
    src, index = torch.zeros(6, 4), torch.zeros(6, dtype=torch.int64)
    with pytest.raises(ValueError, match="no CPU path"):
        scatter_max(src, index, dim=0)
    with pytest.raises(ValueError, match="no CPU path"):
        native_scatter_max(src, index, 3)
    with pytest.raises(TypeError, match="float32"):
        scatter_max(src.double(), index, dim=0)
    with pytest.raises(TypeError, match="float32"):
        native_scatter_max(src.half(), index, 3)
    with pytest.raises(TypeError, match="int64"):
        scatter_max(src, index.int(), dim=0)
    with pytest.raises(TypeError, match="int64"):
        native_scatter_max(src, index.int(), 3)
    with pytest.raises(ValueError):
        native_scatter_max(torch.zeros(6, 4, 2), index, 3)
    with pytest.raises(ValueError):
        native_scatter_max(src, torch.zeros(6, 3, dtype=torch.int64), 3)      # neither [E] nor [E, F]
    with pytest.raises(ValueError):
        native_scatter_max(src, torch.zeros(5, dtype=torch.int64), 3)         # E != S without a row_map
    with pytest.raises(ValueError, match="no CPU path"):
        voxel_isin(torch.zeros(4, 3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(TypeError, match="int32"):
        voxel_isin(torch.zeros(4, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError):
        voxel_isin(torch.zeros(4, 2, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32))


def test_torch_scatter_shim_names_what_it_does_not_support():
    import torch_scatter
    src, index = torch.zeros(6, 4), torch.zeros(6, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="out="):
        torch_scatter.scatter_max(src, index, dim=0, out=(torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int64)))
    with pytest.raises(NotImplementedError, match="dim=1"):
        torch_scatter.scatter_max(src, index, dim=1)
    with pytest.raises(NotImplementedError, match="dim=-1"):
        torch_scatter.scatter_max(src, index)             # the default dim of a 2-D src is the last one
    with pytest.raises(NotImplementedError, match="3 dimensions"):
        torch_scatter.scatter_max(torch.zeros(6, 4, 2), index, dim=0)
    for name in ("scatter_min", "scatter_add", "scatter_mean", "scatter", "segment_csr", "segment_max_coo", "gather_csr",
                 "scatter_softmax"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(torch_scatter, name)(src, index)


def test_voxel_scratch_bytes_monotone_and_aligned():
    lib = ctypes.CDLL(os.path.join(ROOT, "bloomscene_amd", "libbloomscene_rast.so"))
    fn = lib.bsr_voxel_isin_scratch_bytes
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int]
    prev = 0
    for N in [1, 2, 31, 32, 33, 4096, 4097, 100_000, 10 ** 6, 1 << 29]:
        b = fn(N)
        assert b % 256 == 0 and b >= prev and b >= 8 * N, (N, b)     # at least 2 N slots of 4 bytes
        assert b <= max(16 * N, 256), (N, b)                         # ... and below 4 N slots
        prev = b
    assert fn(0) == 0 and fn(-3) == 0 and fn((1 << 29) + 1) == 0
