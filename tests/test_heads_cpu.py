"""CPU tests of the anchor heads (include/bloomscene_heads.h, bloomscene_amd/heads.py): the restatements of
tests/heads_reference.py against each other, the library's entry points, and the python interface's checks -- all before
the device is touched."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import heads_reference as HR
from bloomscene_amd import _capi
from bloomscene_amd import heads as H

SHAPES = ((50, 10), (4, 1), (7, 3))


def _modules(F, K, last=(nn.Tanh, None, nn.Sigmoid)):
    out = []
    for outputs, act in zip((1, 7, 3), last):
        layers = [nn.Linear(F + 4, F), nn.ReLU(True), nn.Linear(F, outputs * K)] + ([act()] if act else [])
        out.append(nn.Sequential(*layers))
    return out


def test_vectorised_fma_is_libms_fmaf():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(20000).astype(np.float32)
    b = rng.standard_normal(20000).astype(np.float32)
    c = rng.standard_normal(20000).astype(np.float32)
    c[:7000] = (-(a[:7000].astype(np.float64) * b[:7000])).astype(np.float32)          # cancelling
    c[7000:10000] *= np.float32(2.0) ** rng.integers(-60, 60, 3000).astype(np.float32)  # far-apart magnitudes
    a[10000:11000] *= np.float32(1e-30)                                                   # subnormal results
    c[10000:11000] *= np.float32(1e-38)
    got, ref = HR.fma32(a, b, c), HR.fmaf_libm(a, b, c)
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()
    plain = (a * b + c).astype(np.float32)
    assert (plain.view(np.uint32) != ref.view(np.uint32)).any()     # (the triples do tell an fma from two roundings)


@pytest.mark.parametrize("F,K", SHAPES)
def test_chain_matches_eager_lines_within_fp32_rounding(F, K):
    s = HR.scene(33, F, K, seed=1)
    a = HR.forward_np(s.feat.numpy(), s.anchor.numpy(), s.cam.numpy(), [w.numpy() for w in s.weights], K)
    ref = HR.autograd64(s.feat, s.anchor, s.cam, s.weights, K, gate=a.gate)
    # scale_rot is pre2 of the cov head: a chain of F + 4 and one of F roundings on values of order 1
    cov = a.pre2[:, K:8 * K].reshape(-1, 7)
    bound = (2 * F + 8) * 2.0 ** -24 * max(1.0, float(np.abs(ref.scale_rot).max()))
    assert np.abs(cov - ref.scale_rot).max() <= bound
    # and it is NOT what a GEMM computes: the order is what gets pinned
    eager = HR.restatement(s.feat, s.anchor, s.cam, s.weights, K)[2].numpy()
    assert np.abs(eager - ref.scale_rot).max() <= bound
    assert a.pre1.shape == (33, 3 * F) and a.pre2.shape == (33, 11 * K)


@pytest.mark.parametrize("F,K", SHAPES)
def test_analytic_backward_of_the_header_matches_autograd(F, K):
    s = HR.scene(19, F, K, seed=2)
    a = HR.forward_np(s.feat.numpy(), s.anchor.numpy(), s.cam.numpy(), [w.numpy() for w in s.weights], K)
    ref = HR.autograd64(s.feat, s.anchor, s.cam, s.weights, K, s.mask, s.ups, a.gate)
    got = HR.backward_np64(s.feat, s.anchor, s.cam, s.weights, K, s.mask, s.ups, a.gate)
    pairs = [(got.d_feat, ref.d_feat), (got.d_anchor, ref.d_anchor), (got.d_mask.reshape(ref.d_mask.shape), ref.d_mask)]
    pairs += list(zip(got.d_weights, ref.d_weights))
    for x, y in pairs:
        assert x.shape == y.shape
        assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(y).max())


def test_geometry_jacobian_against_autograd():
    g = torch.Generator().manual_seed(3)
    anchor = torch.randn(40, 3, generator=g, dtype=torch.float64, requires_grad=True)
    cam = torch.tensor([0.3, -0.2, 4.0], dtype=torch.float64)
    gv, gd = torch.randn(40, 3, generator=g, dtype=torch.float64), torch.randn(40, generator=g, dtype=torch.float64)
    d = anchor - cam
    dist = d.norm(dim=1)
    v = d / dist[:, None]
    ((v * gv).sum() + (dist * gd).sum()).backward()
    vn, dn = v.detach(), dist.detach()
    s = (gv * vn).sum(1)
    mine = (gv - vn * s[:, None]) / dn[:, None] + gd[:, None] * vn      # (I - v v^T) / dist and d dist / dd = v
    assert float((mine - anchor.grad).abs().max()) <= 1e-13


def test_activation_forms_hold_their_bound():
    x = np.concatenate([np.linspace(-12, 12, 40001), np.linspace(-0.3, 0.3, 20001), np.float64(10.0) ** np.linspace(-30, -1, 500)])
    x = x.astype(np.float32)
    t, s = HR.tanh_form(x), HR.sigmoid_form(x)
    t64, s64 = np.tanh(x.astype(np.float64)), 1 / (1 + np.exp(-x.astype(np.float64)))
    assert (np.abs(t - t64) <= 4 * np.spacing(np.abs(t64).astype(np.float32))).all()
    assert (np.abs(s - s64) <= 3 * np.spacing(s64.astype(np.float32))).all()
    assert (np.sign(t) == np.sign(x)).all()


def test_entry_points_exist_and_size_their_scratch():
    lib = _capi.lib()
    for name in ("bsr_anchor_heads_forward", "bsr_anchor_heads_backward", "bsr_anchor_heads_scratch_bytes"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES
    size = lib.bsr_anchor_heads_scratch_bytes
    assert size(1000, 50, 10) > 0 and size(1000, 50, 10) % 256 == 0
    assert size(0, 50, 10) > 0
    assert size(1000, 50, 10) < size(2000, 50, 10)
    for n, F, K in ((-1, 50, 10), (10, 0, 10), (10, 65, 10), (10, 50, 0), (10, 50, 17), (2 ** 31 // 54 + 1, 50, 1),
                    (2 ** 31 // 112 + 1, 4, 16)):
        assert size(n, F, K) == 0, (n, F, K)
    # the per-row operands (X, hid, dpre1, dpre2) and one partial per range of 256 rows and element
    tot = 3 * 50 * 54 + 150 + 110 * 50 + 110
    assert size(1000, 50, 10) >= 4 * (1000 * (54 + 150 + 150 + 110) + 4 * tot)


def test_c_entry_points_name_the_argument_they_refuse():
    import threading
    lib = _capi.lib()
    seen = []

    def forward(n, F, K, w, fs=64):
        return lib.bsr_anchor_heads_forward(n, F, K, None, fs, None, None, None, w, None, None, None, None, None)

    def calls():             # (the error string belongs to the calling thread: this one's dies with it)
        none = _capi.HeadsPointers(*([None] * 12))
        for n, F, K, word in ((-1, 4, 1, "n must"), (1, 0, 1, "F must"), (1, 65, 1, "F must"), (1, 4, 17, "K must"),
                              (2 ** 31 // 8, 4, 1, "2^31")):
            seen.append((forward(n, F, K, none), word in _capi.last_error()))
        seen.append((forward(1, 4, 1, none, fs=3), "feat_stride" in _capi.last_error()))
        seen.append((forward(0, 4, 1, none), "NULL weight tensor of head 0" in _capi.last_error()))
        buf = (ctypes.c_float * 64)()
        addr = ctypes.addressof(buf)
        seen.append((1 - forward(0, 4, 1, _capi.HeadsPointers(*([addr] * 12))), True))     # n == 0 launches nothing
        seen.append((forward(0, 4, 1, _capi.HeadsPointers(*([addr] * 7 + [None] + [addr] * 4))), "head 1" in _capi.last_error()))
        seen.append((forward(1, 4, 1, _capi.HeadsPointers(*([addr] * 12))), "NULL operand" in _capi.last_error()))

    t = threading.Thread(target=calls)
    t.start()
    t.join()
    assert seen == [(1, True)] * 10, seen


def test_python_checks_come_before_the_device_in_the_siblings_order():
    F, K, n = 6, 2, 5
    s = HR.scene(n, F, K)
    ok = dict(feat=s.feat, anchor=s.anchor, camera_center=s.cam, weights=s.weights, K=K, offset_mask=s.mask)

    def call(**kw):
        return H.anchor_heads_tensors(**{**ok, **kw})

    # a wrong dtype first, even with a wrong shape and a camera that wants a gradient beside it
    with pytest.raises(TypeError, match="feat must be float32"):
        call(feat=s.feat.double()[:, :3], camera_center=s.cam.clone().requires_grad_(True))
    with pytest.raises(TypeError, match="mlp_cov.W2 must be float32"):
        call(weights=s.weights[:6] + [s.weights[6].half()] + s.weights[7:])
    with pytest.raises(TypeError, match="anchor must be a torch.Tensor"):
        call(anchor=s.anchor.numpy())
    # then what is not implemented, before any shape
    with pytest.raises(NotImplementedError, match="camera_center requires a gradient"):
        call(camera_center=s.cam.clone().requires_grad_(True), anchor=s.anchor[:, :2])
    # then shapes
    with pytest.raises(ValueError, match=r"anchor must be \[5, 3\]"):
        call(anchor=s.anchor[:, :2])
    with pytest.raises(ValueError, match="offset_mask must be"):
        call(offset_mask=s.mask[:, :1])
    with pytest.raises(ValueError, match="mlp_color.b2 must be"):
        call(weights=s.weights[:11] + [s.weights[11][:-1]])
    with pytest.raises(ValueError, match="K must be in"):
        call(K=17)
    with pytest.raises(ValueError, match="F = feat.shape"):
        call(feat=torch.zeros(n, 65))
    with pytest.raises(ValueError, match="twelve"):
        call(weights=s.weights[:11])
    # and the device last: everything else is right, there is no CPU path
    with pytest.raises(ValueError, match="feat must be on the GPU"):
        call()
    for shape in ((n, K, 1), (n, K), (n * K, 1)):
        with pytest.raises(ValueError, match="on the GPU"):
            call(offset_mask=s.mask.reshape(shape))


def test_module_checker_refuses_a_wrong_layer_and_names_it():
    F, K = 6, 2
    s = HR.scene(3, F, K)
    mo, mc, mcol = _modules(F, K)
    w = H.head_weights(mo, mc, mcol)
    assert len(w) == 12 and w[0] is mo[0].weight and w[7] is mc[2].bias and w[10] is mcol[2].weight    # live parameters
    assert [tuple(t.shape) for t in w[4:8]] == [(F, F + 4), (F,), (7 * K, F), (7 * K,)]
    bad = nn.Sequential(nn.Linear(F + 4, F), nn.LeakyReLU(), nn.Linear(F, K), nn.Tanh())
    with pytest.raises(NotImplementedError, match=r"mlp_opacity\[1\] is a LeakyReLU"):
        H.anchor_heads(s.feat, s.anchor, s.cam, bad, mc, mcol)
    with pytest.raises(NotImplementedError, match=r"mlp_cov\[3\] is a Tanh"):
        H.anchor_heads(s.feat, s.anchor, s.cam, mo, nn.Sequential(*mc, nn.Tanh()), mcol)
    with pytest.raises(NotImplementedError, match=r"mlp_color\[3\] is missing"):
        H.anchor_heads(s.feat, s.anchor, s.cam, mo, mc, nn.Sequential(*list(mcol)[:3]))
    with pytest.raises(NotImplementedError, match=r"mlp_color\[3\] is a Tanh"):
        H.AnchorHeads(mo, mc, nn.Sequential(*list(mcol)[:3], nn.Tanh()))
    with pytest.raises(NotImplementedError, match="must be an nn.Sequential"):
        H.anchor_heads(s.feat, s.anchor, s.cam, mo[0], mc, mcol)
    # dtypes still come first, and a supported model reaches the device check
    with pytest.raises(TypeError, match="feat must be float32"):
        H.anchor_heads(s.feat.double(), s.anchor, s.cam, bad, mc, mcol)
    with pytest.raises(ValueError, match="on the GPU"):
        H.anchor_heads(s.feat, s.anchor, s.cam, mo, mc, mcol, offset_mask=s.mask)
    with pytest.raises(ValueError, match="on the GPU"):
        H.AnchorHeads(mo, mc, mcol).evaluate(s.feat, s.anchor, s.cam)
    with pytest.raises(ValueError, match="on the GPU"):
        H.AnchorHeads(mo, mc, mcol, feat=s.feat, anchor=s.anchor, camera_center=s.cam, offset_mask=s.mask)(torch.tensor([0, 2]))
    with pytest.raises(ValueError, match="not bound"):
        H.AnchorHeads(mo, mc, mcol)(torch.tensor([0, 2]))
