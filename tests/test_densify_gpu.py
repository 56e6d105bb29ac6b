"""Densification on the GPU (include/bloomscene_densify.h): scatter_max, voxel_isin, the torch_scatter shim and
grow_candidates, every output bit-equal to the restatements of tests/densify_reference.py."""
import numpy as np
import pytest
import torch

import densify_reference as DR

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")


def _scatter_max(*a, **k):
    from bloomscene_amd.densify import scatter_max
    return scatter_max(*a, **k)


def _voxel_isin(q, k):
    from bloomscene_amd.densify import voxel_isin
    return voxel_isin(q, k)


def _check_scatter(src, index, G, row_map=None, index_t=None):
    """Run the GPU scatter on numpy inputs (index_t: the index as the GPU tensor to hand over, for strided views) and
    compare out (as bits) and arg with the restatement."""
    ref_out, ref_arg = DR.scatter_max_ref(src, index, G, row_map)
    src_t = torch.from_numpy(np.ascontiguousarray(src)).to(DEV)
    if index_t is None:
        index_t = torch.from_numpy(np.ascontiguousarray(index, np.int64)).to(DEV)
    rm_t = None if row_map is None else torch.from_numpy(np.ascontiguousarray(row_map, np.int64)).to(DEV)
    out, arg = _scatter_max(src_t, index_t, G, row_map=rm_t)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and arg.dtype == torch.int64
    assert tuple(out.shape) == ref_out.shape and tuple(arg.shape) == ref_arg.shape
    bad = np.flatnonzero(DR.bits(out).reshape(-1) != DR.bits(ref_out).reshape(-1))
    assert bad.size == 0, (bad.size, bad[:5])
    assert np.array_equal(arg.cpu().numpy(), ref_arg)
    return out, arg


@pytest.mark.parametrize("E,F,G", [(1, 1, 1), (257, 1, 3), (1000, 50, 37), (4099, 67, 1)])
def test_scatter_max_bit_equal_to_restatement(E, F, G):
    rng = np.random.default_rng(E + F + G)
    src = rng.standard_normal((E, F)).astype(F32)
    _check_scatter(src, rng.integers(0, G, E), G)


def test_scatter_max_permutation_index_every_group_one_row():
    rng = np.random.default_rng(1)
    src = rng.standard_normal((3000, 50)).astype(F32)
    perm = rng.permutation(3000)
    out, arg = _check_scatter(src, perm, 3000)
    assert torch.equal(arg[:, 0].cpu(), torch.from_numpy(np.argsort(perm)))


def test_scatter_max_trailing_and_interior_empty_groups():
    rng = np.random.default_rng(2)
    src = rng.standard_normal((2000, 8)).astype(F32)
    index = rng.integers(0, 200, 2000) * 2          # odd groups stay empty, and everything from 400 on
    out, arg = _check_scatter(src, index, 500)
    assert (arg[1::2] == 2000).all() and (out[1::2] == 0).all() and (arg[400:] == 2000).all()


def test_scatter_max_no_contributions():
    out, arg = _scatter_max(torch.empty(0, 4, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV), 5)
    assert tuple(out.shape) == (5, 4) and (out == 0).all() and (arg == 0).all() and out.device.type == "cuda"
    out, arg = _scatter_max(torch.ones(3, 4, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV), 0)
    assert tuple(out.shape) == (0, 4) and tuple(arg.shape) == (0, 4)


def test_scatter_max_special_values_with_heavy_ties():
    rng = np.random.default_rng(3)
    pool = np.array([-1.0, -0.0, 0.0, 1.0, INF, -INF, NAN], F32)
    pb = pool.view(np.uint32).copy()
    src_bits = pb[rng.integers(0, 7, (1500, 9))]
    nan = src_bits == pb[6]
    src_bits[nan] = (0x7fc00000 | rng.integers(0, 1 << 20, int(nan.sum()))).astype(np.uint32)   # payloads differ
    src_bits[nan & (rng.random(nan.shape) < 0.3)] |= np.uint32(0x80000000)                                 # some negative NaNs
    src = src_bits.view(F32)
    index = rng.integers(0, 400, 1500)          # about four rows a group: many groups have no NaN
    out, arg = _check_scatter(src, index, 401)
    # groups without a NaN that hold both zeros and nothing above: the first zero's sign survives
    assert (DR.bits(out) == 0x80000000).any() and np.isnan(out.cpu().numpy()).any()
    # a group of -inf alone is not an empty group
    _check_scatter(np.full((5, 2), -INF, F32), np.zeros(5, np.int64), 2)


def test_scatter_max_index_forms():
    rng = np.random.default_rng(4)
    E, F, G = 700, 13, 29
    src = rng.standard_normal((E, F)).astype(F32)
    idx = rng.integers(0, G, E)
    idx_t = torch.from_numpy(idx).to(DEV)
    expanded = idx_t.unsqueeze(1).expand(-1, F)
    assert expanded.stride() == (1, 0)
    a_out, a_arg = _check_scatter(src, idx, G, index_t=expanded)
    b_out, b_arg = _check_scatter(src, idx, G)                            # the same, as a 1-D index
    assert torch.equal(a_out, b_out) and torch.equal(a_arg, b_arg)
    dense = rng.integers(0, G, (E, F))                                    # columns differ
    _check_scatter(src, dense, G)
    wide = torch.from_numpy(np.concatenate([dense, dense[:, :3]], 1)).to(DEV)[:, :F]   # a dense index with a row pitch
    assert wide.stride() == (F + 3, 1)
    _check_scatter(src, dense, G, index_t=wide)
    every_other = torch.from_numpy(np.repeat(idx, 2)).to(DEV)[::2]        # a 1-D index with stride 2
    assert every_other.stride() == (2,)
    _check_scatter(src, idx, G, index_t=every_other)
    out, arg = _check_scatter(src[:, 0].copy(), idx, G)                   # a 1-D src
    assert tuple(out.shape) == (G,) and torch.equal(out, a_out[:, 0])


def test_scatter_max_row_map_equals_gathering_first():
    rng = np.random.default_rng(5)
    S, E, F, G = 300, 2500, 50, 111
    src = rng.standard_normal((S, F)).astype(F32)
    row_map = rng.integers(0, S, E)                 # every row about eight times
    index = rng.integers(0, G, E)
    a_out, a_arg = _check_scatter(src, index, G, row_map=row_map)
    b_out, b_arg = _check_scatter(src[row_map], index, G)
    assert torch.equal(a_out.view(torch.int32), b_out.view(torch.int32)) and torch.equal(a_arg, b_arg)


def test_scatter_max_skips_out_of_range_entries_and_writes_nothing_else():
    rng = np.random.default_rng(6)
    S, E, F, G = 64, 900, 5, 17
    src = rng.standard_normal((S, F)).astype(F32)
    row_map = rng.integers(0, S, E)
    row_map[rng.random(E) < 0.1] = -1
    row_map[rng.random(E) < 0.1] = S
    row_map[0] = 2 ** 40
    index = rng.integers(0, G, E)
    index[rng.random(E) < 0.1] = -1
    index[rng.random(E) < 0.1] = G
    index[1] = -2 ** 40
    _check_scatter(src, index, G, row_map=row_map)
    dense = rng.integers(-1, G + 1, (S, F))         # per-element entries of -1 and G, no row_map
    _check_scatter(src, dense, G)
    # out, arg and two guards from one block of memory, so that the guards lie directly behind out and arg
    block = torch.full((4 * G * F * 8,), 0x5A, dtype=torch.uint8, device=DEV)
    n_out, n_arg = G * F * 4, G * F * 8
    arg = block[:n_arg].view(torch.int64).view(G, F)
    guard_a = block[n_arg:n_arg + 256]
    out = block[n_arg + 256:n_arg + 256 + n_out].view(torch.float32).view(G, F)
    guard_b = block[n_arg + 256 + n_out:]
    from bloomscene_amd import _capi
    src_t, idx_t, rm_t = (torch.from_numpy(a).to(DEV) for a in (src, index, row_map))
    _capi.check(_capi.lib().bsr_scatter_max(E, S, F, G, src_t.data_ptr(), rm_t.data_ptr(), idx_t.data_ptr(), 1, 0,
                                            out.data_ptr(), arg.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "bsr_scatter_max")
    torch.cuda.synchronize()
    ref_out, ref_arg = DR.scatter_max_ref(src, index, G, row_map)
    assert np.array_equal(DR.bits(out), DR.bits(ref_out)) and np.array_equal(arg.cpu().numpy(), ref_arg)
    assert (guard_a == 0x5A).all() and (guard_b == 0x5A).all()


def test_scatter_max_two_runs_bit_identical():
    rng = np.random.default_rng(7)
    src = torch.from_numpy(rng.integers(-2, 3, (20000, 50)).astype(F32)).to(DEV)      # ties everywhere
    index = torch.from_numpy(rng.integers(0, 300, 20000)).to(DEV)
    a = _scatter_max(src, index, 300)
    b = _scatter_max(src, index, 300)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    # the first of the tied rows: no earlier row of the group holds the winning value
    arg = a[1][:, 0].cpu().numpy()
    s0, idx = src[:, 0].cpu().numpy(), index.cpu().numpy()
    for g in range(0, 300, 37):
        rows = np.flatnonzero(idx == g)
        assert arg[g] == rows[np.argmax(s0[rows])]       # (numpy's argmax returns the first maximum)


def test_scatter_max_graph_capture_and_replay():
    rng = np.random.default_rng(8)
    E, F, G = 5000, 50, 200
    src = torch.from_numpy(rng.standard_normal((E, F)).astype(F32)).to(DEV)
    index = torch.from_numpy(rng.integers(0, G, E)).to(DEV)
    eager = _scatter_max(src, index, G)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        _scatter_max(src, index, G)   # warm-up on the capture stream
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, arg = _scatter_max(src, index, G)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0]) and torch.equal(arg, eager[1])
    src.copy_(torch.from_numpy(rng.standard_normal((E, F)).astype(F32)).to(DEV))
    g.replay()
    torch.cuda.synchronize()
    again = _scatter_max(src, index, G)
    assert torch.equal(out, again[0]) and torch.equal(arg, again[1])


def test_shim_autograd_routes_the_gradient_to_the_winners():
    from torch_scatter import scatter_max
    rng = np.random.default_rng(9)
    E, F, G = 400, 6, 50
    vals = rng.permutation(E * F).astype(F32).reshape(E, F)            # tie-free
    idx = rng.integers(0, G - 5, E)                                    # the last groups stay empty
    src = torch.from_numpy(vals).to(DEV).requires_grad_(True)
    index = torch.from_numpy(idx).to(DEV)
    out, arg = scatter_max(src, index.unsqueeze(1).expand(-1, F), dim=0, dim_size=G)
    assert not arg.requires_grad and tuple(out.shape) == (G, F)
    out.sum().backward()
    cpu_src = torch.from_numpy(vals).requires_grad_(True)
    ref = torch.zeros(G, F).scatter_reduce(0, torch.from_numpy(idx)[:, None].expand(E, F), cpu_src, "amax",
                                           include_self=False)
    assert torch.equal(out.detach().cpu(), ref.detach())
    ref.sum().backward()
    assert torch.equal(src.grad.cpu(), cpu_src.grad)
    # dim_size derived from the index, a 1-D src with dim=-1, and weighted gradients
    src1 = torch.from_numpy(vals[:, 0].copy()).to(DEV).requires_grad_(True)
    out1, arg1 = scatter_max(src1, index)
    assert tuple(out1.shape) == (int(idx.max()) + 1,)
    w = torch.arange(out1.shape[0], dtype=torch.float32, device=DEV)
    (out1 * w).sum().backward()
    want = torch.zeros(E)
    filled = arg1.cpu() < E
    want[arg1.cpu()[filled]] = w.cpu()[filled]
    assert torch.equal(src1.grad.cpu(), want)


# ---- voxel_isin ----

def _check_isin(query, keys):
    got = _voxel_isin(torch.from_numpy(query).to(DEV), torch.from_numpy(keys).to(DEV))
    torch.cuda.synchronize()
    assert got.dtype == torch.bool and tuple(got.shape) == (query.shape[0],)
    want = DR.voxel_isin_ref(query, keys)
    assert np.array_equal(got.cpu().numpy(), want)
    return want


def test_voxel_isin_degenerate_sizes():
    rng = np.random.default_rng(0)
    q = rng.integers(-3, 4, (50, 3)).astype(np.int32)
    assert not _check_isin(q, np.zeros((0, 3), np.int32)).any()                    # N = 0
    assert _check_isin(np.zeros((0, 3), np.int32), q).shape == (0,)                # U = 0
    q[7] = q[0]
    want = _check_isin(q, q[:1].copy())                                            # N = 1
    assert want[0] and want[7] and want.sum() >= 2


def test_voxel_isin_distinct_keys_half_of_the_queries_present():
    rng = np.random.default_rng(1)
    N = 4097
    codes = rng.choice(1 << 21, 2 * N + 5000, replace=False)                       # distinct cells of a 128^3 cube
    cells = np.stack([codes & 127, (codes >> 7) & 127, codes >> 14], 1).astype(np.int32) - 64
    keys, absent = cells[:N], cells[N:]
    query = np.concatenate([keys[rng.integers(0, N, 5000)], absent[:5000]])
    query = query[rng.permutation(10000)]
    want = _check_isin(query, keys)
    assert want.sum() == 5000


def test_voxel_isin_massive_duplicates():
    rng = np.random.default_rng(2)
    keys = rng.integers(0, 8, (20000, 3)).astype(np.int32)                         # 512 cells, ~40 copies each
    query = rng.integers(-2, 10, (5000, 3)).astype(np.int32)
    want = _check_isin(query, keys)
    assert 0 < want.sum() < 5000


def test_voxel_isin_two_of_three_components_is_no_match():
    rng = np.random.default_rng(3)
    keys = (rng.integers(0, 1000, (3000, 3)) * 2).astype(np.int32)                 # even coordinates only
    query = keys[rng.integers(0, 3000, 3000)].copy()
    query[np.arange(3000), rng.integers(0, 3, 3000)] += 1                          # one component made odd
    want = _check_isin(np.concatenate([query, keys[:100]]), keys)
    assert not want[:3000].any() and want[3000:].all()


def test_voxel_isin_extreme_coordinates():
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    corners = np.array([[a, b, c] for a in (lo, hi, 0, -1) for b in (lo, hi, 0, -1) for c in (lo, hi, 0, -1)], np.int32)
    keys = corners[::2]
    want = _check_isin(corners, keys)
    assert want.tolist() == [i % 2 == 0 for i in range(64)]


@pytest.mark.parametrize("lattice", ["diagonal", "multiples_of_65536", "axis"])
def test_voxel_isin_lattices_that_weak_hashes_collapse(lattice):
    n = 6000
    i = np.arange(-n // 2, n // 2, dtype=np.int64)
    if lattice == "diagonal":
        pts = np.stack([i, i, i], 1)                                               # all components equal
    elif lattice == "multiples_of_65536":
        pts = np.stack([(i % 30) << 16, ((i // 30) % 30) << 16, (i // 900) << 16], 1)
    else:
        pts = np.stack([i * 0, i * 0, i << 10], 1)
    pts = pts.astype(np.int32)
    want = _check_isin(pts, pts[::2].copy())
    assert want.sum() == n // 2


def test_voxel_isin_ignores_what_the_scratch_held():
    from bloomscene_amd import _capi
    rng = np.random.default_rng(4)
    keys = rng.integers(-20, 20, (1000, 3)).astype(np.int32)
    query = rng.integers(-25, 25, (3000, 3)).astype(np.int32)
    lib = _capi.lib()
    k_t, q_t = torch.from_numpy(keys).to(DEV), torch.from_numpy(query).to(DEV)
    want = DR.voxel_isin_ref(query, keys)
    for fill in (0xFF, 0x00, 0x01):
        scratch = torch.full((lib.bsr_voxel_isin_scratch_bytes(1000),), fill, dtype=torch.uint8, device=DEV)
        mask = torch.full((3000 + 64,), 0x5A, dtype=torch.uint8, device=DEV)
        _capi.check(lib.bsr_voxel_isin(3000, 1000, q_t.data_ptr(), k_t.data_ptr(), mask.data_ptr(), scratch.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "bsr_voxel_isin")
        torch.cuda.synchronize()
        assert np.array_equal(mask[:3000].cpu().numpy().astype(bool), want), fill
        assert (mask[3000:] == 0x5A).all()


# ---- grow_candidates ----

GROW_SIZES = (0.01, 0.1, 0.25)     # 0.25: 2000 anchors in about 9^3 cells, most candidate voxels are occupied


@pytest.fixture(scope="module")
def growth_case():
    return DR.make_growth_case(2000, 10, 50, seed=11, cur_sizes=GROW_SIZES)


@pytest.mark.parametrize("cur_size", GROW_SIZES)
def test_grow_candidates_equals_the_restatement(growth_case, cur_size):
    from bloomscene_amd.densify import grow_candidates
    anchor, all_xyz, mask, feat = growth_case
    ref_anchor, ref_feat = DR.grow_candidates_ref(anchor, all_xyz, mask, feat, cur_size, 10)
    n_unique = torch.unique(torch.round(all_xyz.view(-1, 3)[mask] / cur_size).int(), dim=0).shape[0]
    assert ref_anchor.shape[0] > 0
    if cur_size == 0.25:
        assert ref_anchor.shape[0] < n_unique // 2          # most candidates are occupied at the coarse level
    got_anchor, got_feat = grow_candidates(anchor.to(DEV), all_xyz.to(DEV), mask.to(DEV), feat.to(DEV), cur_size)
    assert got_anchor.dtype == torch.float32 and got_feat.dtype == torch.float32
    assert tuple(got_anchor.shape) == tuple(ref_anchor.shape) and tuple(got_feat.shape) == tuple(ref_feat.shape)
    assert torch.equal(got_anchor.cpu().view(torch.int32), ref_anchor.view(torch.int32))
    assert torch.equal(got_feat.cpu().view(torch.int32), ref_feat.view(torch.int32))
    # the flat [N * K, 3] form of all_xyz is the same call
    flat_anchor, flat_feat = grow_candidates(anchor.to(DEV), all_xyz.view(-1, 3).to(DEV), mask.to(DEV), feat.to(DEV),
                                             cur_size)
    assert torch.equal(flat_anchor, got_anchor) and torch.equal(flat_feat, got_feat)


def test_grow_candidates_without_candidates(growth_case):
    from bloomscene_amd.densify import grow_candidates
    anchor, all_xyz, mask, feat = growth_case
    got_anchor, got_feat = grow_candidates(anchor.to(DEV), all_xyz.to(DEV), torch.zeros_like(mask).to(DEV),
                                           feat.to(DEV), 0.1)
    assert tuple(got_anchor.shape) == (0, 3) and tuple(got_feat.shape) == (0, 50)
    assert got_anchor.dtype == torch.float32 and got_feat.dtype == torch.float32 and got_feat.device.type == "cuda"
