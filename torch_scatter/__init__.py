"""Import shim: BloomScene's ``scene/gaussian_model.py:22`` does ``from torch_scatter import scatter_max`` (the
``pytorch_scatter`` CUDA extension) and calls it once, in ``GaussianModel.anchor_growing`` (``:862``).  With this repository
on ``sys.path`` that import resolves here, to the MI355X-native reduction of ``bloomscene_amd.densify`` (C ABI
``include/bloomscene_densify.h``).  Importing needs no GPU.

``scatter_max(src, index, dim=-1, out=None, dim_size=None) -> (out, argmax)`` with the extension's signature.
Supported: float32 ``src`` of one or two dimensions reduced along dimension 0 (``dim`` 0, or -1 for a 1-D ``src``, or -2
for a 2-D one); int64 ``index``, 1-D or of ``src``'s shape (a stride-0 ``.expand`` view is read without a copy);
``dim_size=None`` derives ``index.max() + 1`` with one host read, as the extension does.  Empty groups give ``0`` and
``argmax == src.size(0)``.  Where the extension leaves a tied argmax to a race, the first row wins here, and NaN is above
everything (``include/bloomscene_densify.h``).  Differentiable in ``src``: the gradient of ``out`` goes to the winning
rows.  ``out=``, other dtypes and other dims raise; every other function of the package exists and raises
NotImplementedError.
"""
import torch

from bloomscene_amd import densify as _densify


class _ScatterMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, index, dim_size):
        out, arg = _densify.scatter_max(src, index, dim_size)
        ctx.mark_non_differentiable(arg)
        ctx.save_for_backward(arg)
        ctx.rows = src.shape[0]
        return out, arg

    @staticmethod
    def backward(ctx, grad_out, _grad_arg):
        (arg,) = ctx.saved_tensors
        # one spare row takes what the empty groups (arg == rows) would route: nowhere
        grad = torch.zeros((ctx.rows + 1,) + tuple(arg.shape[1:]), dtype=grad_out.dtype, device=grad_out.device)
        grad.scatter_(0, arg, grad_out.contiguous())
        return grad[:ctx.rows], None, None


def scatter_max(src, index, dim=-1, out=None, dim_size=None):
    who = "torch_scatter.scatter_max"
    if out is not None:
        raise NotImplementedError(f"{who}: out= is not supported on this backend")
    if not isinstance(src, torch.Tensor) or not isinstance(index, torch.Tensor):
        raise TypeError(f"{who}: src and index must be tensors")
    if src.dtype != torch.float32:
        raise TypeError(f"{who}: src must be float32 (got {src.dtype})")
    if index.dtype != torch.int64:
        raise TypeError(f"{who}: index must be int64 (got {index.dtype})")
    if src.dim() not in (1, 2):
        raise NotImplementedError(f"{who}: src of {src.dim()} dimensions is not supported (one or two)")
    if dim not in (0, -src.dim()):
        raise NotImplementedError(f"{who}: dim={dim} is not supported for a {src.dim()}-D src (only dimension 0)")
    if index.dim() != 1 and tuple(index.shape) != tuple(src.shape):
        raise NotImplementedError(f"{who}: index must be 1-D or of src's shape {list(src.shape)} "
                                  f"(got {list(index.shape)})")
    if index.shape[0] != src.shape[0]:
        raise ValueError(f"{who}: index has {index.shape[0]} rows, src {src.shape[0]}")
    if dim_size is None:
        dim_size = int(index.max()) + 1 if index.numel() > 0 else 0
    return _ScatterMax.apply(src, index, int(dim_size))


def _unsupported(name):
    def fn(*args, **kwargs):
        raise NotImplementedError(f"torch_scatter.{name} is not implemented on this backend (BloomScene does not call it)")
    fn.__name__ = name
    return fn


scatter_sum = _unsupported("scatter_sum")
scatter_add = _unsupported("scatter_add")
scatter_mul = _unsupported("scatter_mul")
scatter_mean = _unsupported("scatter_mean")
scatter_min = _unsupported("scatter_min")
scatter = _unsupported("scatter")
segment_sum_csr = _unsupported("segment_sum_csr")
segment_add_csr = _unsupported("segment_add_csr")
segment_mean_csr = _unsupported("segment_mean_csr")
segment_min_csr = _unsupported("segment_min_csr")
segment_max_csr = _unsupported("segment_max_csr")
segment_csr = _unsupported("segment_csr")
gather_csr = _unsupported("gather_csr")
segment_sum_coo = _unsupported("segment_sum_coo")
segment_add_coo = _unsupported("segment_add_coo")
segment_mean_coo = _unsupported("segment_mean_coo")
segment_min_coo = _unsupported("segment_min_coo")
segment_max_coo = _unsupported("segment_max_coo")
segment_coo = _unsupported("segment_coo")
gather_coo = _unsupported("gather_coo")
scatter_std = _unsupported("scatter_std")
scatter_logsumexp = _unsupported("scatter_logsumexp")
scatter_softmax = _unsupported("scatter_softmax")
scatter_log_softmax = _unsupported("scatter_log_softmax")
