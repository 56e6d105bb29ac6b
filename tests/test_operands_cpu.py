"""bloomscene_amd/_operands.py and _capi.call: the binding idioms every wrapper shares, checked once (no GPU, no library load;
torch.nn modules are only constructed, never run)."""
import pytest
import torch
from torch import nn

from bloomscene_amd import _capi
from bloomscene_amd import _operands as ops


# ---- 1. rows_in_place / row_stride ----

def _rows_cases():
    split = torch.split(torch.arange(16.0).reshape(2, 8), [3, 5], dim=1)[1]
    return {  # name: (tensor, n, width, returned as it is, the row stride reported)
        "n0": (torch.empty(0, 3), 0, 3, True, 3),
        "n1_any_row_stride": (torch.arange(5.0).as_strided((1, 3), (0, 1), 1), 1, 3, True, 3),
        "n2_expanded_rows": (torch.arange(3.0).expand(2, 3), 2, 3, False, 3),
        "n2_column_stride_2": (torch.arange(12.0).reshape(2, 6)[:, ::2], 2, 3, False, 3),
        "width1_column_stride_2": (torch.arange(8.0).reshape(2, 4)[:, ::2][:, :1], 2, 1, True, 4),
        "split_view": (split, 2, 5, True, 8),
    }


@pytest.mark.parametrize("case", sorted(_rows_cases()))
def test_rows_in_place_and_row_stride(case):
    t, n, width, in_place, stride = _rows_cases()[case]
    assert tuple(t.shape) == (n, width)
    out = ops.rows_in_place(t, n, width)
    if in_place:
        assert out is t and out.data_ptr() == t.data_ptr()
    else:
        assert out.is_contiguous() and out.data_ptr() != t.data_ptr()
    assert ops.row_stride(out, n, width) == stride
    assert torch.equal(out, t)
    # what a kernel reads: element (i, j) at i * row_stride + j from the result's first element
    assert torch.equal(out.as_strided((n, width), (stride, 1), out.storage_offset()), t)


def test_split_view_keeps_its_place():
    base = torch.arange(16.0).reshape(2, 8)
    view = torch.split(base, [3, 5], dim=1)[1]
    assert ops.rows_in_place(view, 2, 5).data_ptr() == base.data_ptr() + 3 * base.element_size()


def test_ptr_and_upstream_gradient():
    t = torch.zeros(2)
    assert ops.ptr(None) is None and ops.ptr(t) == t.data_ptr()
    assert ops.as_f32_contiguous(None) is None
    g = torch.arange(6.0).reshape(2, 3)
    assert ops.as_f32_contiguous(g) is g
    for other in (g.t(), g.half(), g.double().t()):
        out = ops.as_f32_contiguous(other)
        assert out.dtype == torch.float32 and out.is_contiguous() and torch.equal(out, other.float())


# ---- 2. the texts of the checks (the literal strings of heads.py, densify.py and anchor_state.py) ----

def test_check_tensors_texts():
    half = torch.zeros(2, dtype=torch.float16)
    with pytest.raises(TypeError) as e:
        ops.check_tensors("anchor_heads", [("feat", torch.zeros(2)), ("anchor", 3)])
    assert str(e.value) == "anchor_heads: anchor must be a torch.Tensor (got int)"
    with pytest.raises(TypeError) as e:
        ops.check_tensors("anchor_heads", [("feat", half)])
    assert str(e.value) == "anchor_heads: feat must be float32 (got torch.float16); half precision is not supported"
    with pytest.raises(TypeError) as e:
        ops.check_tensors("scatter_max", [("src", half)], half_note=False)
    assert str(e.value) == "scatter_max: src must be float32 (got torch.float16)"
    with pytest.raises(TypeError) as e:
        ops.check_tensors("scatter_max", [("index", torch.zeros(2, dtype=torch.int32))], torch.int64)
    assert str(e.value) == "scatter_max: index must be int64 (got torch.int32)"
    with pytest.raises(TypeError) as e:
        ops.check_tensors("accumulate", [("idx", torch.zeros(2, dtype=torch.int64), torch.int64),
                                         ("radii", torch.zeros(2), (torch.int32, torch.bool))], half_note=False)
    assert str(e.value) == "accumulate: radii must be int32 or bool (got torch.float32)"
    # the first finding in list order; a dtype of None asks for a tensor of any dtype
    with pytest.raises(TypeError, match="^who: a must be a torch.Tensor"):
        ops.check_tensors("who", [("a", None), ("b", half)])
    ops.check_tensors("who", [("a", half)], None)
    ops.check_tensors("who", [("a", torch.zeros(1)), ("b", torch.zeros(1, dtype=torch.bool), torch.bool)])


def test_device_check_texts():
    cpu, meta = torch.zeros(2), torch.zeros(2, device="meta")
    with pytest.raises(ValueError) as e:
        ops.check_on_gpu("anchor_heads", [("feat", cpu)])
    assert str(e.value) == "anchor_heads: feat must be on the GPU (there is no CPU path)"
    with pytest.raises(ValueError) as e:
        ops.check_same_device("anchor_heads", [("feat", cpu), ("anchor", meta, torch.float32)], cpu.device)
    assert str(e.value) == "anchor_heads: every operand must be on cpu (anchor is on meta)"
    ops.check_same_device("anchor_heads", [("feat", cpu)], cpu.device)


# ---- 3. the order of complaints: a float16 operand on the CPU is a TypeError in every wrapper, never a device complaint ----

def _f(*shape):
    return torch.zeros(*shape)


def _heads():
    from bloomscene_amd.heads import anchor_heads_tensors
    F, K = 4, 2
    weights = [w for O in (K, 7 * K, 3 * K) for w in (_f(F, F + 4), _f(F), _f(O, F), _f(O))]
    return anchor_heads_tensors(_f(3, F).half(), _f(3, 3), _f(3), weights, K)


def _context():
    from bloomscene_amd.context import context_head_tensors, outputs
    D, H, F, K = 4, 8, 4, 2
    return context_head_tensors(_f(3, D).half(), (_f(H, D), _f(H), _f(outputs(F, K), H), _f(outputs(F, K))), F, K)


def _entropy():
    from bloomscene_amd.entropy import gaussian_bits
    return gaussian_bits(_f(3, 2), _f(3, 2).half(), _f(3, 2), 0.5)


def _codec():
    from bloomscene_amd.codec import encode_gaussian
    return encode_gaussian(_f(3, 2), _f(3, 2), _f(3, 2).half(), 0.5)


def _mix_encoding():
    from bloomscene_amd.mix_encoding import mix_encode
    table = (_f(8, 2), torch.tensor([0, 8], dtype=torch.int32), torch.tensor([2], dtype=torch.int32))
    return mix_encode(_f(3, 3).half(), [table], [(0, 1, 2)])


def _anchor_state():
    from bloomscene_amd.anchor_state import visible
    N, F, K = 3, 4, 2
    return visible(torch.arange(2), _f(N, 3), _f(3), _f(3), _f(N, F).half(), _f(N, K, 3), _f(N, 6), _f(N, K, 1))


def _densify():
    from bloomscene_amd.densify import scatter_max
    return scatter_max(_f(3, 2).half(), torch.zeros(3, dtype=torch.int64), 2)


def _voxelize():
    from bloomscene_amd.voxelize import grow_level
    N, K = 3, 2
    return grow_level(_f(N, 3), _f(N, K, 3).half(), _f(N, 6), torch.zeros(N * K, dtype=torch.bool), _f(N, 4), 0.1)


def _adjust():
    from bloomscene_amd.adjust import decide
    N, K = 3, 2
    return decide(_f(N).half(), _f(N), _f(N * K), _f(N * K), K, [0.1])


def _loss():
    from bloomscene_amd.loss import photometric_loss
    return photometric_loss(_f(3, 4, 4).half(), _f(3, 4, 4))


def _depth_loss():
    from bloomscene_amd.depth_loss import depth_prior_loss
    return depth_prior_loss(_f(4, 4), _f(4, 4).half(), _f(4, 4, 3), value=1.0)


def _knn():
    from bloomscene_amd.knn import mean_dist3
    return mean_dist3(_f(4, 3).half())


@pytest.mark.parametrize("call", [_heads, _context, _entropy, _codec, _mix_encoding, _anchor_state, _densify, _voxelize,
                                  _adjust, _loss, _depth_loss, _knn], ids=lambda f: f.__name__.lstrip("_"))
def test_dtype_complaint_wins_over_device_complaint(call):
    with pytest.raises(TypeError, match=r"must be float32 \(got torch\.float16\)"):
        call()


# ---- 4. sequential_weights ----

def _mlp(*layers):
    return nn.Sequential(*layers)


def test_sequential_weights_texts():
    lin = lambda bias=True: nn.Linear(2, 2, bias=bias)
    good = _mlp(lin(), nn.ReLU(), lin(), nn.Tanh())
    w = ops.sequential_weights("w", "m", good, nn.Tanh)
    assert [id(t) for t in w] == [id(t) for t in (good[0].weight, good[0].bias, good[2].weight, good[2].bias)]
    cases = (
        (_mlp(lin(), nn.Tanh(), lin()), None, "w: m[1] is a Tanh (a ReLU is expected)"),
        (_mlp(lin(), nn.ReLU()), None, "w: m[2] is missing (a Linear is expected)"),
        (_mlp(lin(), nn.ReLU(), lin()), nn.Sigmoid, "w: m[3] is missing (a Sigmoid is expected)"),
        (_mlp(lin(), nn.ReLU(), lin(), nn.Sigmoid()), None, "w: m[3] is a Sigmoid: no layer is supported there"),
        (_mlp(lin(False), nn.ReLU(), lin()), None, "w: m[0] has no bias"),
        (_mlp(lin(), nn.ReLU(), lin(False)), None, "w: m[2] has no bias"),
        (lin(), None, "w: m must be an nn.Sequential (got Linear)"),
    )
    for mlp, last, text in cases:
        with pytest.raises(NotImplementedError) as e:
            ops.sequential_weights("w", "m", mlp, last)
        assert str(e.value) == text


def test_head_and_grid_weights_speak_through_sequential_weights():
    """The texts tests/test_heads_cpu.py and tests/test_context_cpu.py expect, with who / name substituted."""
    from bloomscene_amd.context import grid_weights
    from bloomscene_amd.heads import head_weights
    lin = lambda: nn.Linear(2, 2)
    ok = (_mlp(lin(), nn.ReLU(), lin(), nn.Tanh()), _mlp(lin(), nn.ReLU(), lin()))
    short_color = _mlp(lin(), nn.ReLU(), lin())
    with pytest.raises(NotImplementedError) as e:
        head_weights(*ok, short_color)
    with pytest.raises(NotImplementedError, match=r"mlp_color\[3\] is missing") as want:
        ops.sequential_weights("anchor_heads", "mlp_color", short_color, nn.Sigmoid)
    assert str(e.value) == str(want.value)
    short_grid = _mlp(lin(), nn.ReLU())
    with pytest.raises(NotImplementedError) as e:
        grid_weights(short_grid)
    with pytest.raises(NotImplementedError, match=r"mlp_grid\[2\] is missing") as want:
        ops.sequential_weights("context_head", "mlp_grid", short_grid)
    assert str(e.value) == str(want.value)


# ---- 5. _capi.call ----

class _StubLibrary:
    def __init__(self):
        self.seen = []

    def bsr_fine(self, *args):
        self.seen.append(args)
        return 0

    def bsr_broken(self, *args):
        self.seen.append(args)
        return 7

    def bsr_last_error(self):
        return b"the stub's reason"


def test_capi_call(monkeypatch):
    stub = _StubLibrary()
    monkeypatch.setattr(_capi, "lib", lambda: stub)
    assert _capi.call("bsr_fine", 1, None, 2.5) is None
    assert stub.seen == [(1, None, 2.5)]
    with pytest.raises(RuntimeError) as e:
        _capi.call("bsr_broken", 3)
    assert str(e.value).startswith("bsr_broken") and "the stub's reason" in str(e.value)
    assert stub.seen[-1] == (3,)
    with pytest.raises(AttributeError):
        _capi.call("bsr_absent")
