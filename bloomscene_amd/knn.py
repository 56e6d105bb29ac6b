"""Mean squared distance to the three nearest neighbours on the MI355X: BloomScene's ``simple_knn._C.distCUDA2``
(``submodules/simple-knn``, called by ``GaussianModel.create_from_pcd``, ``scene/gaussian_model.py:447,464``) restated
in HIP behind ``include/bloomscene_knn.h``.

    dist2 = mean_dist3(points)    # points float32 [P, 3] on the GPU -> float32 [P]

``dist2[i]`` is the mean of the three smallest squared distances from point ``i`` to the other points, a pure function
of the input written out in the header (fp32, no contraction; duplicates count as 0; NaN / inf points get inf and are
nobody's neighbour; fewer than three neighbours pad with FLT_MAX).  The search is exact, so the result is bit-identical
on every run.  It runs on the current torch stream without a host synchronisation (capturable into a CUDA graph) and
takes its scratch from torch's allocator.  There is no CPU path.
"""
from __future__ import annotations

import torch

from . import _capi
from . import _operands as _ops
from .grid_encoder import check_call


def mean_dist3(points: torch.Tensor) -> torch.Tensor:
    """``points`` float32 ``[P, 3]`` on the GPU (any strides: copied to contiguous if needed) -> new float32 ``[P]``
    (``bsr_knn_mean_dist``)."""
    who = "mean_dist3"
    _ops.check_tensors(who, [("points", points)], None)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: points must be [P, 3] (got {list(points.shape)})")
    points = points.contiguous()
    check_call(who, 3, 1, float_tensors=(("points", points),))   # dtype TypeError, off the GPU ValueError
    P = points.shape[0]
    out = torch.empty(P, dtype=torch.float32, device=points.device)
    if P == 0:
        return out
    scratch = _ops.scratch(_capi.lib().bsr_knn_scratch_bytes(P), points.device)
    _capi.call("bsr_knn_mean_dist", P, points.data_ptr(), out.data_ptr(), scratch.data_ptr(),
               _ops.stream(points.device))
    return out
