"""CPU tests of the context head (include/bloomscene_context.h, bloomscene_amd/context.py): the restatements of
tests/context_reference.py against the literal reference lines run in torch, the tanh form's bound, the library's entry
points, and the python interface's checks -- all before the device is touched."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import context_reference as CR
from bloomscene_amd import _capi
from bloomscene_amd import context as Cx

SHAPES = ((48, 100, 50, 10), (1, 1, 1, 1), (7, 9, 3, 2))


def _np(ts):
    return [t.numpy() for t in ts]


@pytest.mark.parametrize("D,H,F,K", SHAPES)
def test_restatement_has_the_reference_lines_columns_and_formulas(D, H, F, K):
    """numpy's chains, step sizes and training tail against GR:76-97 in fp32 torch: the columns of the split, the order of
    Q's columns, and the formulas -- within the roundings of two chains and of tanh."""
    s = CR.scene(33, D, H, F, K, seed=1)
    a = CR.forward_np(s.enc.numpy(), _np(s.weights), F, K, s.q)
    ref = CR.autograd64(s, gate=a.gate)
    context, Q, feat, gs, go = CR.restatement(s.enc, s.weights, F, K, s.feat, s.grid_scaling, s.grid_offsets, s.noise, s.q)
    assert a.pre2.shape == (33, CR.outputs(F, K)) and a.pre1.shape == (33, H) and tuple(context.shape) == a.pre2.shape
    # a chain of D and one of H roundings on values of order max |context|
    bound = (D + H + 4) * 2.0 ** -24 * max(1.0, float(np.abs(ref.outs[0]).max()))
    assert np.abs(a.pre2 - ref.outs[0]).max() <= bound
    assert np.abs(context.numpy() - ref.outs[0]).max() <= bound
    assert (a.adj.view(np.uint32) == a.pre2[:, -3:].view(np.uint32)).all()
    # Q: the adjustment's error through q (1 + tanh), |d/dadj| <= q, plus 4 ulp of tanh and the two roundings
    q = np.asarray(s.q)[None, :]
    assert (np.abs(a.Q - ref.outs[1]) <= q * (bound + 6 * 2.0 ** -24) + 2.0 ** -24 * np.abs(ref.outs[1])).all()
    assert (np.abs(Q.numpy() - ref.outs[1]) <= q * (bound + 6 * 2.0 ** -24) + 2.0 ** -24 * np.abs(ref.outs[1])).all()
    # the training tail from the SAME Q is the reference line bit for bit (three IEEE operations each)
    for c, (x, noise, got) in enumerate(zip((s.feat, s.grid_scaling, s.grid_offsets), s.noise, (feat, gs, go))):
        mine = CR.noised_np(x.numpy(), noise.numpy(), Q.numpy()[:, c])
        assert mine.shape == tuple(got.shape)
        assert (mine.view(np.uint32) == got.numpy().view(np.uint32)).all(), CR.GRAD_NAMES[1 + c]


@pytest.mark.parametrize("D,H,F,K", SHAPES)
def test_quantiser_restatement_is_ste_multistep(D, H, F, K):
    """quantise_np from the eager lines' own Q: lo, hi, the clamp, x / Q, rint, Qq and d are IEEE operations and agree
    with torch exactly, so the outputs differ by the tanh form alone."""
    s = CR.scene(65, D, H, F, K, seed=2)
    Q, feat, gs, go = CR.restatement_quantise(s.enc, s.weights, F, K, s.feat, s.grid_scaling, s.grid_offsets, s.means, s.q)
    binds = 0
    for c, (x, got) in enumerate(zip((s.feat, s.grid_scaling, s.grid_offsets), (feat, gs, go))):
        z = CR.quantise_np(x.numpy(), Q.numpy()[:, c], s.means[c].numpy())
        Qc = Q[:, c].reshape(-1, *([1] * (x.dim() - 1)))
        clamped = torch.clamp(x, min=s.means[c] - 15_000 * Qc, max=s.means[c] + 15_000 * Qc)
        assert (z.clamped.view(np.uint32) == clamped.numpy().view(np.uint32)).all()
        assert (z.r == torch.round(clamped / Qc).numpy()).all()
        assert (z.Qq.view(np.uint32) == (torch.round(clamped / Qc) * Qc).numpy().view(np.uint32)).all()
        assert z.out.shape == tuple(got.shape)
        tol = 6 * 2.0 ** -24 * np.abs(z.Q) + 2.0 ** -24 * np.abs(z.out64)
        assert (np.abs(z.out - z.out64) <= tol).all()
        assert (np.abs(got.numpy() - z.out64) <= tol).all()
        binds += int(z.bound.sum())
        if c == 1 and D > 1:
            assert np.abs(z.ratio).max() > 1000.0        # thousands of steps in the scaling column
    assert binds > 0 or D == 1


def test_tanh_form_holds_its_bound():
    x = np.concatenate([np.linspace(-12, 12, 40001), np.linspace(-0.3, 0.3, 20001), np.float64(10.0) ** np.linspace(-30, -1, 500)])
    x = x.astype(np.float32)
    t = CR.tanh_form(x)
    t64 = np.tanh(x.astype(np.float64))
    assert (np.abs(t - t64) <= 4 * np.spacing(np.abs(t64).astype(np.float32))).all()
    assert (np.sign(t) == np.sign(x)).all()


def test_entry_points_exist_and_size_their_scratch():
    lib = _capi.lib()
    for name in ("bsr_context_head_forward", "bsr_context_head_backward", "bsr_context_quantise_forward",
                 "bsr_context_scratch_bytes"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES
    size = lib.bsr_context_scratch_bytes
    assert size(1000, 48, 100, 50, 10) > 0 and size(1000, 48, 100, 50, 10) % 256 == 0
    assert size(0, 48, 100, 50, 10) > 0
    assert size(1000, 48, 100, 50, 10) < size(2000, 48, 100, 50, 10)
    for args in ((-1, 48, 100, 50, 10), (10, 0, 100, 50, 10), (10, 129, 100, 50, 10), (10, 48, 0, 50, 10), (10, 48, 129, 50, 10),
                 (10, 48, 100, 0, 10), (10, 48, 100, 65, 10), (10, 48, 100, 50, 0), (10, 48, 100, 50, 17),
                 (2 ** 31 // 175 + 1, 48, 100, 50, 10), (2 ** 31 // 128 + 1, 128, 1, 1, 1)):
        assert size(*args) == 0, args
    # the per-row operands (enc, hid, dpre1, dpre2) and one partial per range of 256 rows and element
    tot = 100 * 48 + 100 + 175 * 100 + 175
    assert size(1000, 48, 100, 50, 10) >= 4 * (1000 * (48 + 100 + 100 + 175) + 4 * tot)


def test_c_entry_points_name_the_argument_they_refuse():
    import threading
    lib = _capi.lib()
    seen = []
    q = (0.25, 2.5e-4, 5e-2)

    def forward(n, D, H, F, K, w, es=128, feat=None, noise=None, out=None):
        return lib.bsr_context_head_forward(n, D, H, F, K, None, es, w, *q, feat, 64, None, 6, None, 48, noise, None, None,
                                            None, None, out, None, None, None, None)

    def calls():             # (the error string belongs to the calling thread: this one's dies with it)
        none = _capi.ContextPointers(*([None] * 4))
        for n, D, H, F, K, word in ((-1, 4, 4, 1, 1, "n must"), (1, 0, 4, 1, 1, "D must"), (1, 129, 4, 1, 1, "D must"),
                                    (1, 4, 0, 1, 1, "H must"), (1, 4, 129, 1, 1, "H must"), (1, 4, 4, 0, 1, "F must"),
                                    (1, 4, 4, 65, 1, "F must"), (1, 4, 4, 1, 0, "K must"), (1, 4, 4, 1, 17, "K must"),
                                    (2 ** 31 // 23 + 1, 4, 4, 1, 1, "2^31")):
            seen.append((forward(n, D, H, F, K, none), word in _capi.last_error()))
        seen.append((forward(1, 4, 4, 1, 1, none, es=3), "enc_stride" in _capi.last_error()))
        seen.append((forward(0, 4, 4, 1, 1, none), "NULL weight tensor" in _capi.last_error()))
        buf = (ctypes.c_float * 64)()
        addr = ctypes.addressof(buf)
        w = _capi.ContextPointers(*([addr] * 4))
        seen.append((1 - forward(0, 4, 4, 1, 1, w), True))                                  # n == 0 launches nothing
        seen.append((forward(1, 4, 4, 1, 1, w), "NULL enc" in _capi.last_error()))
        seen.append((forward(0, 4, 4, 1, 1, w, feat=addr), "feat without its noise" in _capi.last_error()))
        seen.append((forward(0, 4, 4, 1, 1, w, feat=addr, noise=addr), "feat without its output" in _capi.last_error()))
        seen.append((forward(0, 4, 4, 1, 1, w, noise=addr), "feat is NULL" in _capi.last_error()))
        seen.append((lib.bsr_context_head_backward(0, 4, 4, 1, 1, None, 4, w, *q, None, None, None, None, None, addr, None, None,
                                                   None, None, None, None), "needs the forward's noise_feat" in _capi.last_error()))
        seen.append((lib.bsr_context_quantise_forward(0, 4, 4, 1, 1, None, 4, w, *q, addr, 1, None, 6, None, 3, None, None, None,
                                                      None, addr, None, None, None), "feat without its mean" in _capi.last_error()))

    t = threading.Thread(target=calls)
    t.start()
    t.join()
    assert seen == [(1, True)] * len(seen), seen


def test_python_checks_come_before_the_device_in_the_siblings_order():
    D, H, F, K, n = 7, 9, 3, 2, 5
    s = CR.scene(n, D, H, F, K)
    ok = dict(enc=s.enc, weights=s.weights, F=F, K=K, feat=s.feat, grid_scaling=s.grid_scaling, grid_offsets=s.grid_offsets,
              noise=s.noise)

    def call(**kw):
        return Cx.context_head_tensors(**{**ok, **kw})

    wanting = s.noise[0].clone().requires_grad_(True)
    # a wrong dtype first, even with a wrong shape and a noise that wants a gradient beside it
    with pytest.raises(TypeError, match="enc must be float32"):
        call(enc=s.enc.double()[:, :3], noise=(wanting,) + s.noise[1:])
    with pytest.raises(TypeError, match="mlp_grid.W2 must be float32"):
        call(weights=s.weights[:2] + [s.weights[2].half()] + s.weights[3:])
    with pytest.raises(TypeError, match="grid_scaling must be a torch.Tensor"):
        call(grid_scaling=s.grid_scaling.numpy())
    with pytest.raises(TypeError, match=r"noise\[2\] \(grid_offsets\) must be float32"):
        call(noise=s.noise[:2] + (s.noise[2].double(),))
    # then what is not implemented, before any shape
    with pytest.raises(NotImplementedError, match=r"noise\[0\] \(feat\) requires a gradient"):
        call(noise=(wanting,) + s.noise[1:], feat=s.feat[:, :2])
    # then shapes
    with pytest.raises(ValueError, match=r"feat must be \[5, 3\]"):
        call(feat=s.feat[:, :2])
    with pytest.raises(ValueError, match=r"grid_offsets must be \[5, 2, 3\] or \[5, 6\]"):
        call(grid_offsets=s.grid_offsets[:, :1])
    with pytest.raises(ValueError, match="mlp_grid.b2 must be"):
        call(weights=s.weights[:3] + [s.weights[3][:-1]])
    with pytest.raises(ValueError, match="four"):
        call(weights=s.weights[:3])
    with pytest.raises(ValueError, match="without noise"):
        call(noise=(s.noise[0], None, s.noise[2]))
    with pytest.raises(ValueError, match=r"noise\[1\] is given but grid_scaling is not"):
        call(grid_scaling=None)
    with pytest.raises(ValueError, match=r"noise\[0\] must be shaped like feat"):
        call(noise=(s.noise[0][:, :2],) + s.noise[1:])
    with pytest.raises(ValueError, match="3-tuple"):
        call(noise=s.noise[:2])
    with pytest.raises(ValueError, match="q must be three numbers"):
        call(q=(0.25, 0.1))
    with pytest.raises(ValueError, match="K must be an int"):
        call(K=2.0)
    # and the device last: everything else is right, there is no CPU path
    with pytest.raises(ValueError, match="enc must be on the GPU"):
        call()
    with pytest.raises(ValueError, match="on the GPU"):
        call(grid_offsets=s.grid_offsets.reshape(n, 3 * K), noise=s.noise[:2] + (s.noise[2].reshape(n, 3 * K),))
    with pytest.raises(ValueError, match="on the GPU"):
        call(feat=None, grid_scaling=None, grid_offsets=None, noise=None)
    with pytest.raises(ValueError, match="on the GPU"):
        Cx.context_head_maps(**ok)
    # the quantiser: the same order, the means among the operands
    okq = dict(enc=s.enc, weights=s.weights, F=F, K=K, feat=s.feat, grid_scaling=s.grid_scaling, grid_offsets=s.grid_offsets,
               feat_mean=s.means[0], scaling_mean=s.means[1], offsets_mean=s.means[2])
    with pytest.raises(TypeError, match="scaling_mean must be a torch.Tensor"):
        Cx.context_quantise_tensors(**{**okq, "scaling_mean": 0.5, "feat": s.feat[:, :2]})
    with pytest.raises(ValueError, match="offsets_mean must hold one value"):
        Cx.context_quantise_tensors(**{**okq, "offsets_mean": torch.zeros(2)})
    with pytest.raises(ValueError, match="enc must be on the GPU"):
        Cx.context_quantise_tensors(**okq)


@pytest.mark.parametrize("D,H,F,K,word", ((0, 9, 3, 2, "D = enc"), (129, 9, 3, 2, "D = enc"), (7, 0, 3, 2, "H = mlp_grid.W1"),
                                          (7, 129, 3, 2, "H = mlp_grid.W1"), (7, 9, 65, 2, "F must be in"),
                                          (7, 9, 3, 17, "K must be in"), (7, 9, 0, 2, "F must be in"), (7, 9, 3, 0, "K must be in")))
def test_limits_are_refused_naming_the_argument(D, H, F, K, word):
    n, O = 4, CR.outputs(F, K)
    weights = [torch.zeros(H, D), torch.zeros(H), torch.zeros(O, H), torch.zeros(O)]
    with pytest.raises(ValueError, match=word):
        Cx.context_head_tensors(torch.zeros(n, D), weights, F, K)
    with pytest.raises(ValueError, match=word):
        Cx.context_quantise_tensors(torch.zeros(n, D), weights, F, K, None, None, None, None, None, None)
    with pytest.raises(ValueError, match="2\\^31"):
        Cx.context_head_tensors(torch.zeros(1, 1).expand(2 ** 31 // 23 + 1, 1), [torch.zeros(1, 1), torch.zeros(1), torch.zeros(23, 1),
                                                                                 torch.zeros(23)], 1, 1)


def test_module_checker_refuses_a_wrong_layer_and_names_it():
    D, H, F, K = 7, 9, 3, 2
    s = CR.scene(3, D, H, F, K)
    O = CR.outputs(F, K)
    good = nn.Sequential(nn.Linear(D, H), nn.ReLU(True), nn.Linear(H, O))
    w = Cx.grid_weights(good)
    assert len(w) == 4 and w[0] is good[0].weight and w[3] is good[2].bias                  # live parameters
    assert [tuple(t.shape) for t in w] == [(H, D), (H,), (O, H), (O,)]
    with pytest.raises(NotImplementedError, match=r"mlp_grid\[1\] is a LeakyReLU"):
        Cx.context_head(s.enc, nn.Sequential(nn.Linear(D, H), nn.LeakyReLU(), nn.Linear(H, O)), F, K)
    with pytest.raises(NotImplementedError, match=r"mlp_grid\[3\] is a Tanh"):
        Cx.context_head(s.enc, nn.Sequential(*good, nn.Tanh()), F, K)
    with pytest.raises(NotImplementedError, match=r"mlp_grid\[2\] is missing"):
        Cx.ContextHead(nn.Sequential(*list(good)[:2]), F, K)
    with pytest.raises(NotImplementedError, match=r"mlp_grid\[2\] has no bias"):
        Cx.context_quantise(s.enc, nn.Sequential(nn.Linear(D, H), nn.ReLU(), nn.Linear(H, O, bias=False)), F, K, s.feat,
                            s.grid_scaling, s.grid_offsets, *s.means)
    with pytest.raises(NotImplementedError, match="must be an nn.Sequential"):
        Cx.context_head(s.enc, good[0], F, K)
    # dtypes still come first, and a supported model reaches the device check
    with pytest.raises(TypeError, match="enc must be float32"):
        Cx.context_head(s.enc.double(), good[0], F, K)
    with pytest.raises(ValueError, match="on the GPU"):
        Cx.context_head(s.enc, good, F, K, s.feat, s.grid_scaling, s.grid_offsets, s.noise)
    head = Cx.ContextHead(good, F, K)
    assert list(head.parameters())[0] is good[0].weight
    with pytest.raises(ValueError, match="on the GPU"):
        head(s.enc, s.feat, s.grid_scaling, s.grid_offsets, s.noise)
    with pytest.raises(ValueError, match="on the GPU"):
        head.quantise(s.enc, s.feat, s.grid_scaling, s.grid_offsets, *s.means)
