"""CPU tests of tests/anchor_expand_reference.py, the restatement tests/test_anchor_expand_edges_gpu.py holds the
kernels of bloomscene_amd/csrc/anchors.hip against.

1. In float64 the restated backward is torch.autograd through oracle/anchors.py, for every subset of upstream gradients
   the GPU tests use and with the rows that take F.normalize's clamped branch (|v| = 0, 3e-13, 2e-13) included.
2. The selection model's destinations are mask.nonzero() order.
3. The GPU tests' inputs discriminate, stated as conditions on the inputs alone:
   - slot-order and tree-order fp32 sums of d_anchor differ in bits for at least a quarter of the anchors at every K
     used (K = 2 excepted, where no order can differ: a two-term sum is one addition);
   - at every multi-round shape a dropped and a doubled scan carry each move a destination;
   - on every clamped row the normal-branch formula is further from the gradient than any tolerance the GPU test can
     arrive at.
"""
import numpy as np
import pytest
import torch

import anchor_expand_reference as AE
from oracle import anchors as OA


def _autograd_f64(inp, up):
    leaves = [t.double().requires_grad_(True) for t in inp]
    out = OA.expand_anchors_reference(*leaves)
    idx = [i for i, n in enumerate(AE.UPSTREAMS) if up[n] is not None]
    if idx:
        torch.autograd.backward([out[i] for i in idx], [up[AE.UPSTREAMS[i]].double() for i in idx])
    return [np.zeros(tuple(l.shape)) if l.grad is None else l.grad.numpy() for l in leaves]


def _assert_matches_autograd(inp, up, K):
    N = inp[0].shape[0]
    got = AE.restate(inp, up, K, dtype=np.float64)
    d_anchor, d_gs, d_off, d_nop, d_col, d_sr = _autograd_f64(inp, up)
    pairs = (("d_anchor", got["d_anchor"], d_anchor), ("d_gs_xyz", got["d_gs_xyz"], d_gs[:, :3]),
             ("d_gs_scale", got["d_gs_scale"], d_gs[:, 3:]), ("d_offsets", got["d_offsets"], d_off.reshape(N * K, 3)),
             ("d_neural_opacity", got["d_neural_opacity"], d_nop.reshape(-1)), ("d_color", got["d_color"], d_col),
             ("d_sr 0:3", got["d_sr"][:, :3], d_sr[:, :3]), ("d_sr 3:7", got["d_sr"][:, 3:], d_sr[:, 3:]))
    for name, a, b in pairs:
        assert a.shape == b.shape and np.isfinite(b).all(), name
        # float64 with different summation orders and (normalize) different but equivalent formulas; the rows with
        # |v| ~ 1e-7 amplify the rounding of r by 1 / |v|, hence relative to the row's largest entry
        tol = 1e-12 * np.maximum(np.abs(b).max(axis=-1, keepdims=True) if b.ndim > 1 else np.abs(b), 1e-300)
        assert (np.abs(a - b) <= tol).all(), (name, float(np.abs(a - b).max()))


@pytest.mark.parametrize("names", AE.SUBSETS + (AE.UPSTREAMS,), ids=lambda n: "+".join(n) or "none")
def test_restatement_is_float64_autograd_for_every_upstream_subset(names):
    inp = AE.subset_inputs()
    S = int((inp[3] > 0).sum())
    assert 0.35 * 500 < S < 0.65 * 500
    _assert_matches_autograd(inp, AE.upstreams(S, seed=7, names=names), 10)


def test_restatement_is_float64_autograd_on_the_clamped_rows():
    inp, kind = AE.clamped_inputs()
    assert bool((inp[3] > 0).all())
    for dtype in (torch.float32, torch.float64):   # the same branch in both precisions, a factor 1.5 clear of eps
        length = inp[5][:, 3:7].to(dtype).norm(dim=1)
        for k, clamped in enumerate(AE.CLAMPED):
            rows = length[kind == k]
            assert rows.numel() >= 60
            assert bool((rows * 1.5 <= AE.EPS).all()) if clamped else bool((rows >= 1.5 * AE.EPS).all()), AE.CLAMP_KINDS[k]
    # F.normalize's gradient on those rows is g / eps, in fp32 and in float64
    for dtype in (torch.float32, torch.float64):
        v = inp[5][:, 3:7].to(dtype).clone().requires_grad_(True)
        g = AE.upstreams(400, seed=8)["rot"].to(dtype)
        torch.nn.functional.normalize(v).backward(g)
        clamped = torch.tensor(AE.CLAMPED)[kind]
        assert torch.allclose(v.grad[clamped], g[clamped] / AE.EPS, rtol=1e-6, atol=0.0)
    _assert_matches_autograd(inp, AE.upstreams(400, seed=8), 10)


@pytest.mark.parametrize("K", AE.AWKWARD_K)
def test_restatement_is_float64_autograd_at_the_awkward_K(K):
    inp = AE.awkward_inputs(K)
    _assert_matches_autograd(inp, AE.upstreams(int((inp[3] > 0).sum()), seed=K), K)


# ------------------------------------------------------------------------------------------------ selection model
def _masks():
    for N, K in AE.SCAN_SHAPES:
        yield (N, K), K, AE.regional_opacity(N, K, seed=K).numpy().reshape(-1) > 0
    yield "visible", 1, AE.visible_pattern()
    for K in AE.AWKWARD_K:
        yield ("awkward", K), K, AE.awkward_inputs(K)[3].numpy().reshape(-1) > 0


def test_selection_model_is_nonzero_order_and_sees_a_wrong_carry():
    for name, K, mask in _masks():
        counts, bases, dest, total = AE.selection_model(mask, K)
        assert total == int(mask.sum()) and 0 < total < mask.size, name
        assert np.array_equal(dest, np.arange(total)), name     # destination of the j-th selected candidate is row j
        rounds = -(-counts.size // AE.SCAN_ROUND)
        if rounds == 1:
            continue
        # every round after the first writes rows, so each of them needs its carry
        for r0 in range(AE.SCAN_ROUND, counts.size, AE.SCAN_ROUND):
            assert counts[r0:r0 + AE.SCAN_ROUND].sum() > 0, (name, r0)
        for mutation in ("dropped", "doubled"):
            moved = AE.selection_model(mask, K, carry=mutation)[2]
            assert (moved != dest).any(), (name, mutation)


def test_scan_shapes_are_the_rounds_they_claim():
    assert [AE.workgroups(N, K) for N, K in AE.SCAN_SHAPES] == [8192, 8193, 16385]
    assert -(-AE.VISIBLE_P // 256) == 8194
    for N, K in AE.SCAN_SHAPES:
        mask = AE.regional_opacity(N, K, seed=K).numpy().reshape(-1) > 0
        counts = AE.selection_model(mask, K)[0]
        n = mask.size
        dens = [mask[i * n // 3:(i + 1) * n // 3].mean() for i in range(3)]
        assert dens[0] < 0.2 and dens[1] > 0.5 and 0.3 < dens[2] < 0.7, dens       # (the empty stretch lowers one of them)
        empty = counts[AE.SCAN_ROUND - 150:AE.SCAN_ROUND + 150]
        assert empty.size > 0 and not empty[:-1].any()   # nothing selected across the boundary (the last anchor apart)
        assert counts[-1] == K                           # the last workgroup: one anchor, fully selected
    front = AE.visible_pattern()
    assert 0.3 < front.mean() < 0.7
    flips = np.flatnonzero(front[1:] != front[:-1])
    assert flips.size > 4000 and np.unique(np.diff(flips)).size > 300     # many blocks, irregular lengths


# ------------------------------------------------------------------------------------------------ discrimination
@pytest.mark.parametrize("K", AE.AWKWARD_K + (10,))
def test_slot_order_differs_from_tree_order_in_bits(K):
    inp = AE.subset_inputs() if K == 10 else AE.awkward_inputs(K)
    N = inp[0].shape[0]
    sel = inp[3].numpy().reshape(-1) > 0
    up = AE.upstreams(int(sel.sum()), seed=K)
    gx = AE._scatter(up["xyz"].numpy(), sel, 3, np.float32).reshape(N, K, 3)
    slot, tree = AE.slot_order_sum(gx), AE.tree_sum(gx)
    assert AE.bits_equal(slot, AE.restate(inp, up, K)["d_anchor"])
    differ = (slot.view(np.uint32) != tree.view(np.uint32)).any(axis=1)
    if K == 2:
        assert not differ.any()     # (0 + a) + b and a + b are one rounding of the same sum: nothing to tell apart
        return
    assert differ.mean() >= 0.25, (K, float(differ.mean()))
    np.testing.assert_allclose(slot, tree, rtol=0, atol=1e-4)   # (the same sum all the same)


def test_slot_order_differs_from_tree_order_at_the_two_round_shape():
    N, K = AE.SCAN_SHAPES[1]
    inp = AE.scan_inputs(N, K)
    sel = inp[3].numpy().reshape(-1) > 0
    g = torch.randn(int(sel.sum()), 3, generator=torch.Generator().manual_seed(3)).numpy()
    gx = AE._scatter(g, sel, 3, np.float32).reshape(N, K, 3)
    differ = (AE.slot_order_sum(gx).view(np.uint32) != AE.tree_sum(gx).view(np.uint32)).any(axis=1)
    assert differ.mean() >= 0.25


def test_clamped_rows_are_far_from_the_normal_branch():
    """Without the `len <= eps` branch the kernel would evaluate (g - r (r.g)) / |v| on the clamped rows.  On every one
    of them that is non-finite or at least AE.CLAMP_MARGIN of the class's scale away from the true gradient, in some
    component; the GPU test asserts that the tolerance it arrives at stays below that margin."""
    inp, kind = AE.clamped_inputs()
    up = AE.upstreams(400, seed=8)
    ref = AE.restate(inp, up, 10)["d_sr"][:, 3:]
    wrong = AE.normal_branch_rot_gradient(inp[5].numpy(), up["rot"].numpy())
    clamped = np.asarray(AE.CLAMPED)[kind.numpy()]
    scale = np.abs(ref[clamped]).max()
    assert 1e11 < scale < 1e13
    with np.errstate(invalid="ignore"):
        dist = np.abs(wrong - ref).max(axis=1)
    far = ~np.isfinite(dist) | (dist > AE.CLAMP_MARGIN * scale)
    assert far[clamped].all()
    assert np.abs(wrong - ref)[~clamped].max() <= 1e-9 * np.abs(ref[~clamped]).max()   # and the formula itself is right
