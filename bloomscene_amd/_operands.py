"""What every Python wrapper of the C ABI does with its operands before and around a native call, written once.
Importing this module needs neither a GPU nor the shared library.

THE ORDER OF COMPLAINTS.  A wrapper's entry point examines its arguments in this order and raises the first finding:

  1. every dtype: a non-tensor or a tensor of the wrong dtype is a TypeError (``check_tensors``);
  2. what is not implemented: NotImplementedError (an operand that requires a gradient the kernels do not give, an
     unsupported option or layer);
  3. shapes and values: ValueError (op-specific, written in the wrapper);
  4. the device, last: ValueError, first "must be on the GPU" for every operand (``check_on_gpu``: there is no CPU
     path), then "every operand must be on ..." (``check_same_device``).

So a float16 tensor on the CPU is a TypeError, never a device complaint: that much holds in every wrapper.  Two older
orders are kept as they were and say so themselves.  ``grid_encoder.check_call`` takes options, then shapes, then dtypes,
then the device; the entry points built on it (``grid_encode``, ``knn.mean_dist3``, ``densify.scatter_max`` and
``densify.voxel_isin``) check their own shapes before they call it.  ``entropy._Operands`` checks "on the GPU" after the
dtypes and before the shapes.  Nothing here reads a tensor's contents: no host synchronisation, capturable into a CUDA
graph.
"""
from __future__ import annotations

import torch
from torch import nn

HALF_NOTE = "; half precision is not supported"


# ---- what a native call is given ----

def ptr(t):
    """The device pointer of a tensor; None (a null pointer) for None."""
    return None if t is None else t.data_ptr()


def rows_in_place(t, n, width):
    """``t [n, width]`` itself if the kernels can read it where it is, else a dense copy.

    The rule, which ``row_stride`` shares: a kernel reads element ``(i, j)`` at ``i * row_stride + j``.  That needs a
    unit column stride (any, where ``width`` is 1: ``j`` is always 0) and, where there is more than one row, a row stride
    of at least ``width`` (an expanded row, stride 0, would alias in a gradient and is copied).  With ``n <= 1`` only row
    0 is read, so ``stride(0)`` is never looked at and ``row_stride`` reports ``width``: torch gives a one-row view an
    arbitrary ``stride(0)``."""
    if (width == 1 or t.stride(1) == 1) and (n <= 1 or t.stride(0) >= width):
        return t
    return t.contiguous()


def row_stride(t, n, width):
    """The row stride, in elements, of what ``rows_in_place(t, n, width)`` returned."""
    return t.stride(0) if n > 1 else width


def stream(dev):
    """The raw handle of the current torch stream of ``dev``: every native call is queued there."""
    return torch.cuda.current_stream(dev).cuda_stream


def scratch(nbytes, dev):
    """``nbytes`` of scratch from torch's allocator (stream-ordered: it may be dropped once the call is queued)."""
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def as_f32_contiguous(g):
    """An upstream gradient as a backward kernel reads it: None stays None, else float32 and contiguous."""
    if g is None:
        return None
    return g.contiguous() if g.dtype == torch.float32 else g.float().contiguous()


# ---- the checks: a finding is the complaint's text without its "who: " prefix, or None ----

def dtype_complaint(name, t, dtypes=torch.float32, half_note=True):
    """The text for a tensor whose dtype is not (one of) ``dtypes``; float32 alone carries ``HALF_NOTE`` unless
    ``half_note`` is False.  (Whether the dtype is wrong is the caller's test: ``wrong_tensor`` makes it.)"""
    dtypes = dtypes if isinstance(dtypes, tuple) else (dtypes,)
    names = " or ".join(str(d).replace("torch.", "") for d in dtypes)
    return f"{name} must be {names} (got {t.dtype})" + (HALF_NOTE if half_note and dtypes == (torch.float32,) else "")


def wrong_tensor(named, dtypes=torch.float32, half_note=True):
    """The first finding of step 1 among ``[(name, tensor)]`` or ``[(name, tensor, dtypes)]``: a non-tensor, or a dtype
    that is not (one of) the entry's own ``dtypes``, else the call's.  ``dtypes`` None: any dtype."""
    for entry in named:
        t = entry[1]
        if not isinstance(t, torch.Tensor):
            return f"{entry[0]} must be a torch.Tensor (got {type(t).__name__})"
        want = entry[2] if len(entry) > 2 else dtypes
        if want is not None and t.dtype not in (want if isinstance(want, tuple) else (want,)):
            return dtype_complaint(entry[0], t, want, half_note)
    return None


def off_gpu(named):
    """The first finding of step 4's first pass: an operand that is not on a GPU."""
    for entry in named:
        if entry[1].device.type != "cuda":
            return f"{entry[0]} must be on the GPU (there is no CPU path)"
    return None


def check_tensors(who, named, dtypes=torch.float32, half_note=True):
    """Step 1: raise TypeError ``"{who}: ..."`` for the first entry of ``named`` that is not a tensor of its dtype
    (``wrong_tensor`` has the arguments)."""
    finding = wrong_tensor(named, dtypes, half_note)
    if finding:
        raise TypeError(f"{who}: {finding}")


def check_on_gpu(who, named):
    """Step 4, first pass: raise ValueError for the first tensor of ``named`` that is not on a GPU."""
    finding = off_gpu(named)
    if finding:
        raise ValueError(f"{who}: {finding}")


def check_same_device(who, named, dev):
    """Step 4, second pass: raise ValueError for the first tensor of ``named`` that is not on ``dev``."""
    for entry in named:
        if entry[1].device != dev:
            raise ValueError(f"{who}: every operand must be on {dev} ({entry[0]} is on {entry[1].device})")


def sequential_weights(who, name, mlp, last=None):
    """``[W1, b1, W2, b2]`` of an ``nn.Sequential`` that is ``Linear, ReLU, Linear`` and then ``last`` (a layer type, or
    None for nothing), as they are (live); anything else raises NotImplementedError naming the layer."""
    if not isinstance(mlp, nn.Sequential):
        raise NotImplementedError(f"{who}: {name} must be an nn.Sequential (got {type(mlp).__name__})")
    want = [nn.Linear, nn.ReLU, nn.Linear] + ([last] if last is not None else [])
    layers = list(mlp)
    for i in range(max(len(want), len(layers))):
        if i >= len(want):
            raise NotImplementedError(f"{who}: {name}[{i}] is a {type(layers[i]).__name__}: no layer is supported "
                                      "there")
        if i >= len(layers):
            raise NotImplementedError(f"{who}: {name}[{i}] is missing (a {want[i].__name__} is expected)")
        if type(layers[i]) is not want[i]:
            raise NotImplementedError(f"{who}: {name}[{i}] is a {type(layers[i]).__name__} "
                                      f"(a {want[i].__name__} is expected)")
    for i in (0, 2):
        if layers[i].bias is None:
            raise NotImplementedError(f"{who}: {name}[{i}] has no bias")
    return [layers[0].weight, layers[0].bias, layers[2].weight, layers[2].bias]
