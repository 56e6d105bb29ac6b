"""Hash-grid encoder, CPU side: the restatement (tests/grid_reference.py) against its float64 twin and hand-computed
cases, the table rule of GridEncoder, the _gridencoder shim's surface and checks, and the scratch size function."""
import inspect

import numpy as np
import pytest
import torch

import grid_reference as GR

F32 = np.float32

# BloomScene's configurations (scene/gaussian_model.py:131-135)
RES_3D = (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514)
RES_2D = (130, 258, 514, 1026)


def _table(D, F, res, log2, seed=0):
    from bloomscene_amd.grid_encoder import table_offsets
    offs = np.array(table_offsets(D, res, log2), np.int64)
    emb = np.random.default_rng(seed).uniform(-1, 1, (int(offs[-1]), F)).astype(F32)
    return offs, np.array(res, np.int64), emb


def test_restatement_matches_float64_twin():
    rng = np.random.default_rng(1)
    for D, res, log2 in ((3, RES_3D[:8], 14), (2, (10, 40, 130), 10), (1, (7, 300), 6)):
        offs, r, emb = _table(D, 2, res, log2)
        x = rng.uniform(0, 1, (3000, D)).astype(F32)
        x[:5] = 0.0
        x[5:10] = 1.0
        out, _ = GR.forward(x, emb, offs, r, with_dy_dx=False)
        twin = GR.forward_f64(torch.from_numpy(x).double(), torch.from_numpy(emb).double(), offs, r).numpy()
        assert np.abs(out - twin).max() < 1e-6


def test_dy_dx_is_the_twin_derivative_at_interior_points():
    rng = np.random.default_rng(2)
    for D, res, log2 in ((3, (18, 24, 59), 19), (2, (20, 130), 10)):
        offs, r, emb = _table(D, 1, res, log2, seed=3)
        x = rng.uniform(0.05, 0.95, (400, D)).astype(F32)
        _, dy = GR.forward(x, emb, offs, r)
        xt = torch.from_numpy(x).double().requires_grad_(True)
        twin = GR.forward_f64(xt, torch.from_numpy(emb).double(), offs, r)
        for l in range(len(res)):
            (gx,) = torch.autograd.grad(twin[l, :, 0].sum(), xt, retain_graph=True)
            # interior: every corner of the cell included (pg >= 1 and pg + 1 <= res - 2 in every dimension)
            pos = x * F32(res[l] - 2) + F32(0.5)
            pg = np.floor(pos)
            interior = np.all((pg >= 1) & (pg + 1 <= res[l] - 2), axis=1)
            assert interior.sum() > 100
            err = np.abs(dy[interior, l, :, 0] - gx.numpy()[interior])
            assert err.max() <= 1e-5 * max(1.0, np.abs(gx.numpy()[interior]).max()), (D, l, err.max())


def test_fixed_point_backward_within_its_bound():
    rng = np.random.default_rng(4)
    for D, res, log2, N in ((3, RES_3D[:6] + (201,), 15, 5000), (2, RES_2D, 12, 3000)):
        offs, r, emb = _table(D, 2, res, log2)
        x = rng.uniform(0, 1, (N, D)).astype(F32)
        g = rng.normal(0, 1, (len(res), N, 2)).astype(F32)
        ge, _, s = GR.backward(x, offs, r, emb.shape[0], g)
        s64, bound, cnt = GR.fixed_point_bound(x, offs, r, emb.shape[0], g)
        assert cnt.max() > 1
        assert (np.abs(ge.astype(np.float64) - s64) <= bound).all()
        assert all(isinstance(v, int) for v in s)


def test_hand_computed_cases():
    # dense 2D level, res 6: x = (0.5, 0.5) -> pos 2.5, corners (2,2), (3,2), (2,3), (3,3), weights 1/4
    emb = np.arange(36 * 1, dtype=F32).reshape(36, 1)
    offs, r = np.array([0, 36]), np.array([6])
    x = np.array([[0.5, 0.5]], F32)
    out, _ = GR.forward(x, emb, offs, r)
    assert out[0, 0, 0] == F32((14 + 15 + 20 + 21) / 4)
    # border: x = (0, 0) -> pos 0.5, pg 0: only corner (1, 1) is included, its weight 1/4 renormalised to 1
    out, _ = GR.forward(np.array([[0.0, 0.0]], F32), emb, offs, r)
    assert out[0, 0, 0] == F32(7)
    # x = 1 exactly is inside: pos 4.5, pg 4: corner 5 = res - 1 is excluded, (4, 4) alone
    out, _ = GR.forward(np.array([[1.0, 1.0]], F32), emb, offs, r)
    assert out[0, 0, 0] == F32(4 + 4 * 6)
    # outside [0, 1] (and NaN): 0, dy_dx 0
    out, dy = GR.forward(np.array([[-1e-7, 0.5], [0.5, 1.0000001], [np.nan, 0.5]], F32), emb, offs, r)
    assert (out == 0).all() and (dy == 0).all()
    # wn == 0: res 2 has no included corner at all -> wn = 1e-9, output 0, no contribution
    out, _ = GR.forward(np.array([[0.3, 0.7]], F32), np.ones((8, 1), F32), np.array([0, 8]), np.array([2]))
    assert out[0, 0, 0] == 0
    ge, _, _ = GR.backward(np.array([[0.3, 0.7]], F32), np.array([0, 8]), np.array([2]), 8, np.ones((1, 1, 1), F32))
    assert (ge == 0).all()
    # hashed level: res 10, hashmap 16 -> stride 100 > 16: row = (p0 * 1 ^ p1 * 2654435761) mod 2^32 % 16
    emb = np.arange(16, dtype=F32)[:, None] * F32(10)
    x = np.array([[0.5, 0.5]], F32)   # pos 4.5: corners (4,4), (5,4), (4,5), (5,5), all weights 1/4
    want = 0.0
    for p0, p1 in ((4, 4), (5, 4), (4, 5), (5, 5)):
        row = ((p0 * 1) ^ ((p1 * 2654435761) & 0xFFFFFFFF)) % 16
        want += row * 10 / 4
    out, _ = GR.forward(x, emb, np.array([0, 16]), np.array([10]))
    assert out[0, 0, 0] == F32(want)


def test_grid_encoder_offsets_follow_the_reference_rule():
    from bloomscene_amd.grid_encoder import GridEncoder, level_rows
    e3 = GridEncoder(3, 2, RES_3D, 19)
    e2 = GridEncoder(2, 2, RES_2D, 17)
    assert int(e3.offsets_list[-1]) == 4_003_896 and tuple(e3.params.shape) == (4_003_896, 2)
    assert int(e2.offsets_list[-1]) == 345_616 and tuple(e2.params.shape) == (345_616, 2)
    assert e3.offsets_list.dtype == torch.int32 and e3.resolutions_list.tolist() == list(RES_3D)
    # levels 0-5 dense, 6-11 hashed (3D); 0-1 dense, 2-3 hashed (2D)
    assert level_rows(3, RES_3D, 19)[:6] == [int(np.ceil(r ** 3 / 8) * 8) for r in RES_3D[:6]]
    assert level_rows(3, RES_3D, 19)[6:] == [2 ** 19] * 6
    assert level_rows(2, RES_2D, 17) == [16_904, 66_568, 2 ** 17, 2 ** 17]   # 130^2, 258^2 rounded up to 8


def test_shim_surface_and_rejections():
    import _gridencoder as G
    assert list(inspect.signature(G.grid_encode_forward).parameters) == [
        "inputs", "embeddings", "offsets_list", "resolutions_list", "outputs", "N", "num_dim", "n_features", "n_levels",
        "max_level", "Rb", "PV", "dy_dx", "binary_vxl", "min_level_id"]
    assert list(inspect.signature(G.grid_encode_backward).parameters) == [
        "grad", "inputs", "embeddings", "offsets_list", "resolutions_list", "grad_embeddings", "N", "num_dim",
        "n_features", "n_levels", "max_level", "Rb", "dy_dx", "grad_inputs", "binary_vxl", "min_level_id"]
    for name in ("grid_encode_mix2D_forward", "grid_encode_mix2D_backward", "avg_2D_forward", "avg_2D_backward",
                 "cnt_np_embed", "cnt_np_embed_backward"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(G, name)()
    x = torch.rand(10, 3)
    emb = torch.zeros(64, 2)
    offs = torch.tensor([0, 64], dtype=torch.int32)
    res = torch.tensor([4], dtype=torch.int32)
    out = torch.empty(1, 10, 2)

    def fwd(**kw):
        a = dict(inputs=x, embeddings=emb, offsets_list=offs, resolutions_list=res, outputs=out, N=10, num_dim=3,
                 n_features=2, n_levels=1, max_level=0, Rb=128, PV=0, dy_dx=None, binary_vxl=None, min_level_id=None)
        a.update(kw)
        G.grid_encode_forward(*a.values())

    with pytest.raises(NotImplementedError, match="binary_vxl"):
        fwd(binary_vxl=torch.ones(128, 128, 128, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="min_level_id"):
        fwd(min_level_id=torch.zeros(10, dtype=torch.int32))
    with pytest.raises(TypeError, match="float32"):
        fwd(embeddings=emb.half())
    with pytest.raises(ValueError, match="num_dim"):
        fwd(num_dim=4)
    with pytest.raises(ValueError, match="n_features"):
        fwd(n_features=16)
    with pytest.raises(ValueError, match="GPU"):
        fwd()   # CPU tensors: no CPU path
    with pytest.raises(NotImplementedError, match="binary_vxl"):
        G.grid_encode_backward(out, x, emb, offs, res, emb, 10, 3, 2, 1, 0, 128, None, None, torch.ones(2), None)
    from bloomscene_amd.grid_encoder import grid_encode
    with pytest.raises(TypeError):
        grid_encode(x.double(), emb, offs, res)
    with pytest.raises(ValueError):
        grid_encode(x, emb, offs, res)


def test_backward_scratch_bytes_is_monotone():
    from bloomscene_amd import _capi
    f = _capi.lib().bsr_grid_backward_scratch_bytes
    prev = 0
    for rows in (0, 1, 31, 32, 33, 1000, 345_616, 4_003_896):
        b = f(rows, 2, 12)
        assert b >= prev and b % 256 == 0 and b >= rows * 2 * 8
        prev = b
    assert f(1000, 4, 12) >= f(1000, 2, 12) >= f(1000, 1, 12)
    assert f(1000, 2, 16) >= f(1000, 2, 12)
