"""Voxel unique on the GPU (include/bloomscene_voxelize.h): every output equal to the restatement of
tests/voxel_reference.py, the quantisation rules pinned to eager torch on the same device on points at the rounding
boundaries, grow_level against densify.grow_candidates and against the GM lines evaluated eagerly.  Every comparison is
exact: this feature has no tolerance."""
import numpy as np
import pytest
import torch

import densify_reference as DR
import voxel_reference as VR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = 1024                       # rows one workgroup of the scatter kernel owns (csrc/voxelize.hip: BSR_VX_CHUNK_MIN)
TEST_CHUNK = 64                # ... with the test flag (BSR_VX_CHUNK_TEST)
SIZES = (0.001, 0.004, 0.016)
GUARD = 0x5A


def _V():
    import bloomscene_amd.voxelize as V
    return V


def _cpu(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _check_coords(coords, flags=0):
    """voxel_unique on int32 rows (numpy) against the restatement; -> the restatement's result."""
    coords = np.ascontiguousarray(coords, np.int32).reshape(-1, 3)
    want = VR.voxel_unique_ref(coords)
    got = _V().voxel_unique(torch.from_numpy(coords).to(DEV), _flags=flags)
    assert [t.dtype for t in got] == [torch.int32, torch.int64, torch.int64, torch.int64]
    for name, g, w in zip(("coords", "inverse", "first", "counts"), _cpu(got), want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1)) if len(w) else np.zeros(0, int)
        assert bad.size == 0, (name, bad.size, bad[:5])
    return want


class _Raw:
    """One direct bsr_voxel_unique call whose outputs lie in ONE block of memory, a guard directly behind each."""
    NAMES = ("coords", "inverse", "first", "counts", "points", "status")

    def __init__(self, E, point_bytes=4):
        sizes = dict(coords=12 * E, inverse=8 * E, first=8 * E, counts=8 * E, points=3 * point_bytes * E, status=32)
        self.span, off = {}, 256
        for n in self.NAMES:
            self.span[n] = (off, off + sizes[n])
            off = (off + sizes[n] + 256 + 255) // 256 * 256          # at least 256 guard bytes, the next start aligned
        self.block = torch.full((off,), GUARD, dtype=torch.uint8, device=DEV)
        self.E = E

    def out(self, name, dtype):
        a, b = self.span[name]
        return self.block[a:b].view(dtype)

    def call(self, source, flags=0, scratch=None, with_points=True):
        """source: the twelve source arguments (form .. voxel_size)."""
        from bloomscene_amd import _capi
        lib = _capi.lib()
        if scratch is None:
            scratch = torch.empty(lib.bsr_voxel_unique_scratch_bytes(self.E), dtype=torch.uint8, device=DEV)
        ptr = lambda n: self.block.data_ptr() + self.span[n][0]
        _capi.check(lib.bsr_voxel_unique(*source, ptr("coords"), ptr("inverse"), ptr("first"), ptr("counts"),
                                         ptr("points") if with_points else None, ptr("status"), scratch.data_ptr(), flags,
                                         torch.cuda.current_stream().cuda_stream), "bsr_voxel_unique")
        torch.cuda.synchronize()
        return [int(v) & 0xffffffff for v in self.out("status", torch.int32).tolist()]

    def guards_intact(self):
        keep = torch.ones(self.block.shape[0], dtype=torch.bool, device=DEV)
        for a, b in self.span.values():
            keep[a:b] = False
        return bool((self.block[keep] == GUARD).all())

    def untouched(self, names):
        return all(bool((self.block[self.span[n][0]:self.span[n][1]] == GUARD).all()) for n in names)


def _coords_source(t):
    return (0, 0, t.shape[0], t.shape[0], t.data_ptr(), 3, None, None, 0, 0, None, 1.0)


def _points_source(t, s, rows=None, rule=0):
    form = 1 if t.dtype == torch.float32 else 2
    E = t.shape[0] if rows is None else rows.shape[0]
    return (form, rule, E, t.shape[0], t.data_ptr(), t.stride(0), None, None, 0, 0, None if rows is None else rows.data_ptr(),
            float(s))


# ---- sizes ----

@pytest.mark.parametrize("E", [0, 1, 2, 63, 64, 65, C - 1, C, C + 1, 3 * C + 17])
def test_sizes_against_the_restatement(E):
    rng = np.random.default_rng(E)
    coords = rng.integers(-9, 10, (E, 3)).astype(np.int32) * np.array([1, 3, 1], np.int32)     # 5 + 6 + 5 bits: two passes
    want = _check_coords(coords)
    assert want[3].sum() == E and (E < 3 or 1 < len(want[3]) <= E)
    if E:
        _check_coords(coords, flags=_V().FLAG_TEST_SMALL_CHUNK)      # the same rows through 64-row workgroups


def test_more_sort_workgroups_than_one_step_of_the_row_scan():
    """With the test flag a sort workgroup owns 64 rows: 257 of them are one more than a step of k_voxel_rowscan
    handles, and the last owns a single row."""
    E = 256 * TEST_CHUNK + 1
    rng = np.random.default_rng(7)
    coords = rng.integers(-40, 41, (E, 3)).astype(np.int32)          # 7 + 7 + 7 bits: three passes, the last 5 bits wide
    want = _check_coords(coords, flags=_V().FLAG_TEST_SMALL_CHUNK)
    assert 1000 < len(want[3]) < E
    _check_coords(coords)                                            # and through 17 workgroups of 1024


# ---- key widths ----

def test_all_rows_equal_is_one_voxel_of_width_zero():
    coords = np.tile(np.array([[-7, VR.I32_MAX, VR.I32_MIN]], np.int32), (2500, 1))
    want = _check_coords(coords)
    assert want[0].tolist() == [[-7, VR.I32_MAX, VR.I32_MIN]] and want[2].tolist() == [0] and want[3].tolist() == [2500]
    raw, t = _Raw(2500), torch.from_numpy(coords).to(DEV)
    status = raw.call(_coords_source(t), with_points=False)
    assert status == [1, 0, 0, 0, 0, 0, 0, 0] and raw.guards_intact() and raw.untouched(["points"])


def test_all_rows_distinct():
    rng = np.random.default_rng(2)
    codes = rng.permutation(1 << 15)[:5000]
    coords = np.stack([(codes & 31) - 16, ((codes >> 5) & 31) - 3, (codes >> 10) - 31], 1).astype(np.int32)
    want = _check_coords(coords)
    assert len(want[3]) == 5000 and (want[3] == 1).all() and np.array_equal(np.sort(want[2]), np.arange(5000))


@pytest.mark.parametrize("bits", [(3, 5, 0), (0, 8, 0), (9, 0, 0), (2, 3, 4), (1, 0, 32), (11, 11, 11), (32, 32, 0),
                                  (0, 32, 32), (32, 0, 32), (22, 21, 21), (32, 0, 0), (0, 32, 0), (0, 0, 32)])
def test_key_widths(bits):
    """8, 9, 33 and 64 key bits -- a pass boundary, one bit past it, one bit past a word, the full key -- and one axis
    spanning INT_MIN .. INT_MAX with the other two constant; negative coordinates throughout."""
    assert sum(bits) in (8, 9, 32, 33, 64)
    rng = np.random.default_rng(sum(bits) * 11 + bits[2])
    coords = VR.case_with_bits(bits, rng, E=1500)
    if bits in ((32, 0, 0), (0, 32, 0), (0, 0, 32)):
        k = bits.index(32)
        coords[:2, k] = [VR.I32_MIN, VR.I32_MAX]
        assert (coords[:, (k + 1) % 3] == coords[0, (k + 1) % 3]).all()
    if not (coords < 0).any():
        coords = ~coords                                             # (-1 - c: the same spans, below zero)
    _check_coords(coords)
    raw, t = _Raw(1500), torch.from_numpy(coords).to(DEV)
    status = raw.call(_coords_source(t), with_points=False)
    assert status[1:] == [0, sum(bits), 0, bits[0], bits[1], bits[2], 0] and raw.guards_intact()
    assert status[0] == len(VR.voxel_unique_ref(coords)[3])


@pytest.mark.parametrize("bits", [(32, 32, 1), (1, 32, 32), (22, 22, 21), (32, 32, 32)])
def test_sixty_five_bits_are_refused_and_nothing_is_written(bits):
    coords = VR.case_with_bits(bits, np.random.default_rng(3), E=1500)
    t = torch.from_numpy(coords).to(DEV)
    with pytest.raises(ValueError, match=rf"{bits[0]} \+ {bits[1]} \+ {bits[2]} = {sum(bits)} key bits"):
        _V().voxel_unique(t)
    raw = _Raw(1500)
    status = raw.call(_coords_source(t))
    assert status == [0, 0, sum(bits), 2, bits[0], bits[1], bits[2], 0]
    assert raw.guards_intact() and raw.untouched(["coords", "inverse", "first", "counts", "points"])


# ---- stability ----

def test_heavy_duplicates_first_is_the_smallest_position():
    rng = np.random.default_rng(4)
    voxels = np.array([[0, 0, 0], [0, 0, 1], [-1, 2, 0], [5, -5, 5], [5, -5, 6], [-300, 0, 0], [0, 0, -1]], np.int32)
    which = rng.integers(0, 7, 5000)
    coords = voxels[which]
    want = _check_coords(coords)
    coords_u, inverse, first, counts = want
    assert len(counts) == 7 and counts.sum() == 5000
    assert np.array_equal(coords_u[inverse], coords)
    for v in range(7):
        assert first[v] == np.flatnonzero(inverse == v)[0]
    _check_coords(coords, flags=_V().FLAG_TEST_SMALL_CHUNK)


# ---- the rules against eager torch on the same device ----

@pytest.fixture(scope="module")
def boundary():
    x = VR.boundary_points(20000, SIZES, seed=12, spread=0.04)   # about 16 000, 1 200 and 70 voxels at the three sizes
    return x, torch.from_numpy(x).to(DEV)


@pytest.mark.parametrize("s", SIZES)
def test_reciprocal_rule_equals_eager_torch_on_boundary_points(boundary, s):
    """torch.round(x / s).int() on the GPU is rintf(x * float(1.0 / s)), the reciprocal taken in double: bit for bit on
    points within 2 ulp of a rounding boundary, where x / s and x * (1 / s) part ways."""
    V = _V()
    x, xt = boundary
    eager = torch.round(xt / s).int()
    got = V.quantise(xt, s, rule="reciprocal")
    assert got.dtype == torch.int32 and torch.equal(got, eager)
    ref, valid = VR.quantise_ref(x, s, "reciprocal")
    assert valid.all() and np.array_equal(got.cpu().numpy(), ref)
    # the sample tells the rules apart (at 0.016 the quotients of this box are below 3 and the rules agree), and the
    # divide rule is the CPU's
    div = V.quantise(xt, s, rule="divide")
    assert s == 0.016 or (div != got).any(dim=1).sum() > 50
    assert np.array_equal(div.cpu().numpy(), VR.quantise_ref(x, s, "divide")[0])
    assert torch.equal(div.cpu(), torch.round(torch.from_numpy(x) / s).int())
    # the unique of it: torch.unique's rows, inverse and counts
    tu, tinv, tcnt = torch.unique(eager, dim=0, return_inverse=True, return_counts=True)
    coords, inverse, first, counts, points = V.voxel_unique(xt, s, rule="reciprocal", return_points=True)
    assert torch.equal(coords, tu) and torch.equal(inverse, tinv) and torch.equal(counts, tcnt)
    assert torch.equal(eager[first], coords)
    want = VR.voxel_unique_ref(ref)
    assert np.array_equal(first.cpu().numpy(), want[2])
    assert torch.equal(points, tu * s)                                # GM:850's product
    assert not torch.signbit(points[points == 0]).any()


def test_float64_divide_rows_and_strides_against_the_restatement(boundary):
    V = _V()
    x = boundary[0].astype(np.float64) + 1e-9 * np.arange(60000).reshape(20000, 3)
    x[:3] = [[0.5, -0.5, 1.5], [2.5, -0.0, 0.0], [-1.5, -2.5, 3.5]]
    s = 0.004
    n_bad, want = VR.unique_rows_ref(x, s)
    got = V.voxel_unique(torch.from_numpy(x).to(DEV), s, return_points=True)
    assert n_bad == 0 and got[4].dtype == torch.float64
    for g, w in zip(_cpu(got[:4]), want):
        assert np.array_equal(g, w)
    assert np.array_equal(got[4].cpu().numpy(), VR.voxel_points_ref(want[0], s, np.float64))
    assert np.array_equal(V.quantise(torch.from_numpy(x).to(DEV), s).cpu().numpy(), VR.quantise_ref(x, s)[0])
    # a rows list with repeats, out of order, on a padded tensor read in place (row stride 5)
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 20000, 7001)
    padded = torch.zeros(20000, 5, dtype=torch.float64, device=DEV)
    padded[:, 1:4] = torch.from_numpy(x).to(DEV)
    view = padded[:, 1:4]
    assert view.stride() == (5, 1)
    n_bad, want = VR.unique_rows_ref(x, s, rows=rows)
    got = V.voxel_unique(view, s, rows=torch.from_numpy(rows).to(DEV))
    for g, w in zip(_cpu(got), want):
        assert np.array_equal(g, w)
    # float32 through the same path
    x32 = boundary[0]
    n_bad, want = VR.unique_rows_ref(x32, s, rows=rows)
    got = V.voxel_unique(boundary[1], s, rows=torch.from_numpy(rows).to(DEV))
    for g, w in zip(_cpu(got), want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_voxelize_sample_equals_gm437(dtype):
    V = _V()
    rng = np.random.default_rng(6)
    data = (rng.standard_normal((15000, 3)) * 0.02).astype(dtype)
    data[:3] = [[0.0, -0.0, 0.0004], [-0.0004, 0.0005, -0.0005], [0.0015, 0.0025, -0.0015]]
    want = VR.voxelize_sample_numpy(data, 0.001)
    got = V.voxelize_sample(data, 0.001)
    assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == want.shape
    assert (got == want).all() and not np.signbit(got[got == 0]).any()
    t = torch.from_numpy(data)
    on_cpu = V.voxelize_sample(t, 0.001)
    assert on_cpu.device.type == "cpu" and np.array_equal(on_cpu.numpy(), got)
    on_gpu = V.voxelize_sample(t.to(DEV), 0.001)
    assert on_gpu.device.type == "cuda" and np.array_equal(on_gpu.cpu().numpy(), got)
    assert torch.equal(V.voxelize(t.to(DEV), 0.001), on_gpu)


# ---- grow_level ----

GROW_SIZES = (0.01, 0.1, 0.25)


@pytest.fixture(scope="module")
def growth_case():
    """tests/densify_reference.make_growth_case(2000, 10, 50, ...) with its all_xyz split into offset * scaling: powers
    of two as scaling, so that the product is exact and anchor + offset * scaling is the case's all_xyz again."""
    anchor, all_xyz, mask, feat = DR.make_growth_case(2000, 10, 50, seed=11, cur_sizes=GROW_SIZES)
    g = torch.Generator().manual_seed(1)
    scaling = torch.rand(2000, 6, generator=g) + 0.5
    scaling[:, :3] = 2.0 ** torch.randint(-2, 3, (2000, 3), generator=g).float()
    offset = (all_xyz - anchor.unsqueeze(1)) / scaling[:, :3].unsqueeze(1)
    rebuilt = anchor.unsqueeze(1) + offset * scaling[:, :3].unsqueeze(1)
    assert (rebuilt == all_xyz).float().mean() > 0.9
    return [t.to(DEV) for t in (anchor, offset, scaling, mask, feat)]


@pytest.mark.parametrize("cur_size", GROW_SIZES)
def test_grow_level_equals_grow_candidates(growth_case, cur_size):
    from bloomscene_amd.densify import grow_candidates
    anchor, offset, scaling, mask, feat = growth_case
    all_xyz = anchor.unsqueeze(1) + offset * scaling[:, :3].unsqueeze(1)          # GM:824, eagerly
    ref_anchor, ref_feat = grow_candidates(anchor, all_xyz, mask, feat, cur_size)
    got_anchor, got_feat = _V().grow_level(anchor, offset, scaling, mask, feat, cur_size)
    assert ref_anchor.shape[0] > 0 and got_anchor.dtype == torch.float32 and got_feat.dtype == torch.float32
    assert tuple(got_anchor.shape) == tuple(ref_anchor.shape) and tuple(got_feat.shape) == tuple(ref_feat.shape)
    assert torch.equal(got_anchor.view(torch.int32), ref_anchor.view(torch.int32))
    assert torch.equal(got_feat.view(torch.int32), ref_feat.view(torch.int32))
    flat_anchor, flat_feat = _V().grow_level(anchor, offset.reshape(-1, 3), scaling, mask, feat, cur_size)
    assert torch.equal(flat_anchor, got_anchor) and torch.equal(flat_feat, got_feat)


@pytest.mark.parametrize("cur_size", SIZES)
def test_grow_level_equals_the_gm_lines_on_boundary_points(cur_size):
    """A level whose anchors and candidate positions lie within a few ulp of the rounding boundaries (the points
    make_growth_case draws again), with scalings that are no powers of two: the product rounds, then the sum."""
    N, K, F = 1500, 10, 8
    rng = np.random.default_rng(13)
    anchor = VR.boundary_points(N, SIZES, seed=14, spread=0.1)
    target = VR.boundary_points(N * K, SIZES, seed=15, spread=0.1).reshape(N, K, 3)
    scaling = (rng.random((N, 6)) * 1.5 + 0.5).astype(np.float32)
    offset = ((target - anchor[:, None]) / scaling[:, None, :3]).astype(np.float32)
    mask = rng.random(N * K) < 0.2
    mask[:K] = True
    offset[0] = 0.0                                                   # candidates in an occupied voxel: the anchor's own
    feat = rng.standard_normal((N, F)).astype(np.float32)
    a, o, sc, m, f = (torch.from_numpy(t).to(DEV) for t in (anchor, offset, scaling, mask, feat))
    ref_anchor, ref_feat = VR.grow_level_eager(a, o, sc, m, f, cur_size)
    got_anchor, got_feat = _V().grow_level(a, o, sc, m, f, cur_size)
    assert 50 < ref_anchor.shape[0] < int(mask.sum()) - 10            # (at the coarsest size most voxels are occupied)
    assert tuple(got_anchor.shape) == tuple(ref_anchor.shape) and tuple(got_feat.shape) == tuple(ref_feat.shape)
    assert torch.equal(got_anchor.view(torch.int32), ref_anchor.view(torch.int32))
    assert torch.equal(got_feat.view(torch.int32), ref_feat.view(torch.int32))
    # the sample is at the boundaries: the CPU's rule gives other voxels
    all_xyz = (a.unsqueeze(1) + o * sc[:, :3].unsqueeze(1)).view(-1, 3)[m]
    assert (_V().quantise(all_xyz, cur_size, "divide") != _V().quantise(all_xyz, cur_size, "reciprocal")).any()


def test_grow_level_without_candidates(growth_case):
    anchor, offset, scaling, mask, feat = growth_case
    got_anchor, got_feat = _V().grow_level(anchor, offset, scaling, torch.zeros_like(mask), feat, 0.1)
    assert tuple(got_anchor.shape) == (0, 3) and tuple(got_feat.shape) == (0, 50)
    assert got_anchor.dtype == torch.float32 and got_feat.dtype == torch.float32 and got_feat.device.type == "cuda"


# ---- invalid input ----

@pytest.mark.parametrize("what", ["nan", "inf", "two_to_31", "row_minus_one", "row_P"])
def test_invalid_rows_are_counted_and_refused(what):
    V = _V()
    P, s = 3000, 0.5
    rng = np.random.default_rng(8)
    x = (rng.random((P, 3)) * 20 - 10).astype(np.float32)
    rows = rng.integers(0, P, 2000)
    rows = np.where(np.isin(rows, [5, 2999, 0, 77, 9]), 1, rows)      # the points made bad below: only where placed
    n_bad = 2
    if what == "nan":
        x[5, 1] = x[2999, 0] = np.nan
        rows[:2] = [5, 2999]
    elif what == "inf":
        x[0, 2], x[77, 0] = np.inf, -np.inf
        rows[:2] = [0, 77]
    elif what == "two_to_31":
        x[9, 0] = 2.0 ** 30                       # / 0.5 = 2^31: one past INT_MAX
        x[10, 0] = -2.0 ** 30                     # INT_MIN: valid
        rows[:3] = [9, 10, 9]
    elif what == "row_minus_one":
        rows[[3, 1999]] = -1
    else:
        rows[[0, 1000, 1500]] = [P, P + 1, 2 ** 40]
        n_bad = 3
    xt, rt = torch.from_numpy(x).to(DEV), torch.from_numpy(rows).to(DEV)
    assert VR.unique_rows_ref(x, s, rows=rows)[0] == n_bad
    with pytest.raises(ValueError, match=f"voxel_unique: {n_bad} invalid row"):
        V.voxel_unique(xt, s, rows=rt)
    for rule in (0, 1):
        raw = _Raw(2000)
        status = raw.call(_points_source(xt, s, rows=rt, rule=rule))
        assert status[:2] == [0, n_bad] and status[3] == 1
        assert raw.guards_intact() and raw.untouched(["coords", "inverse", "first", "counts", "points"])
    if what in ("nan", "inf", "two_to_31"):
        # quantise writes (0, 0, 0) for such a row and counts it
        from bloomscene_amd import _capi
        q = torch.full((P + 64, 3), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        count = torch.full((65,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        _capi.check(_capi.lib().bsr_voxel_quantise(*_points_source(xt, s), q.data_ptr(), count.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream), "bsr_voxel_quantise")
        ref, valid = VR.quantise_ref(x, s)
        assert np.array_equal(q[:P].cpu().numpy(), ref) and count[0].item() == int((~valid).sum()) > 0
        assert (q[P:] == 0x5A5A5A5A).all() and (count[1:] == 0x5A5A5A5A).all()
        assert torch.equal(V.quantise(xt, s), q[:P])


# ---- reproducibility, scratch, allocation, capture ----

def test_two_runs_are_bit_identical(boundary):
    V = _V()
    a = V.voxel_unique(boundary[1], 0.004, rule="reciprocal", return_points=True)
    b = V.voxel_unique(boundary[1], 0.004, rule="reciprocal", return_points=True)
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_the_result_does_not_depend_on_what_the_scratch_held(boundary):
    from bloomscene_amd import _capi
    x, xt = boundary
    s, E = 0.004, 20000
    n_bad, want = VR.unique_rows_ref(x, s)
    U = len(want[3])
    nbytes = _capi.lib().bsr_voxel_unique_scratch_bytes(E)
    for fill in (0x00, 0xFF, 0x01):
        raw = _Raw(E)
        scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        status = raw.call(_points_source(xt, s), scratch=scratch)
        assert status[:4] == [U, 0, sum(status[4:7]), 0] and raw.guards_intact(), fill
        assert np.array_equal(raw.out("coords", torch.int32).view(E, 3)[:U].cpu().numpy(), want[0]), fill
        assert np.array_equal(raw.out("inverse", torch.int64).cpu().numpy(), want[1]), fill
        assert np.array_equal(raw.out("first", torch.int64)[:U].cpu().numpy(), want[2]), fill
        assert np.array_equal(raw.out("counts", torch.int64)[:U].cpu().numpy(), want[3]), fill
        assert np.array_equal(raw.out("points", torch.float32).view(E, 3)[:U].cpu().numpy(),
                              VR.voxel_points_ref(want[0], s, np.float32)), fill
        # rows U .. E-1 of the outputs are not written
        assert (raw.out("first", torch.int64)[U:].view(torch.uint8) == GUARD).all()


def test_no_device_memory_outside_torch():
    from bloomscene_amd import _capi
    V = _V()
    P = 1_000_000
    x = torch.rand(P, 3, device=DEV)
    V.voxel_unique(x[:1000], 0.01)    # library loaded, kernels resident
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, total = torch.cuda.mem_get_info()
    outside0 = total - free0 - torch.cuda.memory_reserved()
    alloc0 = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    coords, inverse, first, counts = V.voxel_unique(x, 0.01)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    outside1 = total - free1 - torch.cuda.memory_reserved()
    assert outside1 - outside0 < (8 << 20), (outside0, outside1)
    # the scratch is on torch's books
    assert torch.cuda.max_memory_allocated() - alloc0 >= _capi.lib().bsr_voxel_unique_scratch_bytes(P)
    assert counts.sum().item() == P and 100_000 < coords.shape[0] <= 101 ** 3
    assert torch.equal(coords[inverse], V.quantise(x, 0.01))


def test_quantise_graph_capture_and_replay(boundary):
    V = _V()
    x = boundary[1].clone()
    eager = V.quantise(x, 0.004, rule="reciprocal")
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        V.quantise(x, 0.004, rule="reciprocal")   # warm-up on the capture stream
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        q = V.quantise(x, 0.004, rule="reciprocal")
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(q, eager)
    x.mul_(1.7)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(q, torch.round(x / 0.004).int()) and not torch.equal(q, eager)
