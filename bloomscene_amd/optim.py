"""BloomScene's optimizer on the MI355X: ``torch.optim.Adam(l, lr=0.0, eps=1e-15)`` as ``scene/gaussian_model.py:531``
constructs it over thirteen parameter groups and ``bloomscene.py:358`` steps it, as ONE HIP launch over all tensors behind
``include/bloomscene_adam.h`` (which states the function per element, bit for bit).

    self.optimizer = bloomscene_amd.optim.Adam(l, lr=0.0, eps=1e-15)        # the one-line replacement

``Adam`` is a ``torch.optim.Optimizer``: ``param_groups`` keep their extra keys (the reference's ``"name"``), and the state is
torch's own layout, created lazily -- ``state[p] = {"step", "exp_avg", "exp_avg_sq"}`` with ``step`` a 0-dim float32
tensor -- so ``state_dict()`` / ``load_state_dict()`` interchange with ``torch.optim.Adam`` in both directions and the
reference's optimizer surgery (``replace_tensor_to_optimizer``, ``cat_tensors_to_optimizer``, ``_prune_anchor_optimizer``:
a group's ``nn.Parameter`` swapped, its state moved with sliced or extended moments and the inherited ``step``) runs on it
unmodified: the descriptors are built from the live tensors at every step and nothing about a tensor is cached.

A parameter whose ``grad`` is ``None`` is skipped and gets no state.  A non-contiguous ``grad`` is made contiguous.
``weight_decay != 0``, ``amsgrad``, ``maximize``, ``differentiable``, sparse gradients and a closure raise
``NotImplementedError``; there is no CPU path and no half precision.

``capturable=False`` (default): ``step`` lives on the CPU, ``group["lr"]`` is a python float (``param_group['lr'] = lr`` of
``update_learning_rate`` keeps working; ``set_lrs`` assigns the same way), one launch, no device allocation after the first
step and no host wait.

``capturable=True``: ``step`` lives on the device, the learning rates of all groups are 0-dim views of ONE device tensor
(each ``group["lr"]`` is such a view) that ``set_lrs({name_or_index: value})`` updates with one non-blocking copy from pinned
memory, outside a capture; a python float found in ``group["lr"]`` at ``step()`` raises ``ValueError``.  ``step()`` is then two
launches with no host read and can be captured with ``torch.cuda.graph`` and replayed.  For learning rates that are fp32
values the two forms give the same bits.

Importing this module needs no GPU.
"""
from __future__ import annotations

import torch

from . import _capi
from . import _operands as _ops
from ._capi import AdamTensor

__all__ = ["Adam"]


class Adam(torch.optim.Optimizer):
    """See the module docstring.  The argument list is ``torch.optim.Adam``'s as far as the reference uses it."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, capturable=False):
        if isinstance(lr, torch.Tensor):
            lr = float(lr)
        if not lr >= 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not eps >= 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        self._capturable = bool(capturable)
        self._lr_dev = self._lr_host = self._lr_copied = None
        self._descriptors = {}    # length -> a ctypes array, rewritten at every step (the buffer only: no tensor is cached)
        # the keys of torch.optim.Adam's groups, so that a state dict moves between the two in both directions
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=False, foreach=None,
                        capturable=self._capturable, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        if self._capturable:
            self._install_device_lrs()

    # ---- learning rates ----
    def _device_of_params(self):
        for group in self.param_groups:
            for p in group["params"]:
                return p.device
        raise ValueError("Adam(capturable=True) needs at least one parameter")

    def _install_device_lrs(self):
        """(capturable) one device tensor [groups], one pinned mirror; every group["lr"] becomes a 0-dim view of the former."""
        dev = self._device_of_params()
        if dev.type != "cuda":
            raise ValueError(f"bloomscene_amd.optim.Adam has no CPU path: the parameters are on {dev}")
        values = [float(g["lr"]) for g in self.param_groups]
        self._lr_host = torch.tensor(values, dtype=torch.float32).pin_memory()
        self._lr_dev = torch.empty(len(values), dtype=torch.float32, device=dev)
        self._push_lrs()
        for i, g in enumerate(self.param_groups):
            g["lr"] = self._lr_dev[i]

    def _push_lrs(self):
        self._lr_dev.copy_(self._lr_host, non_blocking=True)
        self._lr_copied = torch.cuda.Event()
        self._lr_copied.record(torch.cuda.current_stream(self._lr_dev.device))

    def _group_index(self, key):
        if isinstance(key, str):
            hits = [i for i, g in enumerate(self.param_groups) if g.get("name") == key]
            if len(hits) != 1:
                raise KeyError(f"{len(hits)} parameter groups are named {key!r}")
            return hits[0]
        if not 0 <= int(key) < len(self.param_groups):
            raise KeyError(f"no parameter group {key}")
        return int(key)

    def set_lrs(self, lrs):
        """``{group name or index: learning rate}``.  Default form: assigns ``group["lr"]``.  Capturable form: ONE non-blocking
        copy of all rates from pinned memory into the device tensor the groups view; call it outside a capture."""
        items = [(self._group_index(k), float(v)) for k, v in lrs.items()]
        if not self._capturable:
            for i, v in items:
                self.param_groups[i]["lr"] = v
            return
        if self._lr_copied is not None:
            self._lr_copied.synchronize()    # the previous copy has read the pinned mirror (it has long finished)
        for i, v in items:
            self._lr_host[i] = v
        self._push_lrs()

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if getattr(self, "_capturable", False) and self._lr_dev is not None:
            self._install_device_lrs()    # the tensor grows: every view is re-seated (reads the rates back; not in a capture)

    def load_state_dict(self, state_dict):
        """torch's, then the loaded ``step`` and ``lr`` values brought to this form's places (``step`` on the CPU or on the
        device, the rates back into the one device tensor).  Not inside a capture."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            group["capturable"] = self._capturable
            for p in group["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    step = torch.as_tensor(st["step"], dtype=torch.float32)
                    st["step"] = step.to(p.device) if self._capturable else step.cpu()
        if self._capturable:
            self._install_device_lrs()
        else:
            for group in self.param_groups:
                if isinstance(group["lr"], torch.Tensor):
                    group["lr"] = float(group["lr"])

    # ---- the step ----
    def _gather(self):
        """-> [(group, p, grad, state or None)] of the parameters that have a gradient.  ONE pass over the live tensors (the
        host's cost of a step is this loop and the next: tools/bench_adam.py prints it); the first finding of each kind is
        kept and the kinds are raised in ``_operands``' order of complaints before any state is created."""
        f32, cap, state = torch.float32, self._capturable, self.state
        work, dev = [], None
        wrong_type = unsupported = wrong_layout = wrong_device = None
        betas = eps = None
        for group in self.param_groups:
            if unsupported is None:
                if group["weight_decay"] != 0:
                    unsupported = "weight_decay != 0 is not implemented"
                else:
                    for key in ("amsgrad", "maximize", "differentiable"):
                        if group.get(key):
                            unsupported = f"{key} is not implemented"
            lr = group["lr"]
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                st = state.get(p) or None
                work.append((group, p, g, st))
                if betas is None:
                    betas, eps, dev = group["betas"], group["eps"], p.device
                elif unsupported is None and (group["betas"] != betas or group["eps"] != eps):
                    unsupported = "betas and eps that differ between groups are not implemented"
                if p.dtype != f32 or g.dtype != f32:
                    wrong_type = wrong_type or f"takes float32 parameters and gradients (got {p.dtype}, {g.dtype})"
                if g.is_sparse:
                    unsupported = unsupported or "sparse gradients are not implemented"
                    continue
                if not p.is_contiguous():
                    wrong_layout = wrong_layout or "a parameter must be contiguous"
                if g.shape != p.shape:
                    wrong_layout = wrong_layout or (f"gradient of shape {tuple(g.shape)} for a parameter of shape "
                                                    f"{tuple(p.shape)}")
                if cap and (not isinstance(lr, torch.Tensor) or lr.dtype != f32 or lr.device != dev):
                    wrong_layout = wrong_layout or ("(capturable=True): group['lr'] is a python number or a foreign tensor; set "
                                                    "learning rates with set_lrs({name_or_index: value}), which updates the "
                                                    "device tensor the step reads")
                if p.device != dev or g.device != dev or dev.type != "cuda":
                    wrong_device = wrong_device or (f"has no CPU path and steps one device per call: parameter on {p.device}, "
                                                    f"gradient on {g.device}")
                if st is not None:
                    for key in ("exp_avg", "exp_avg_sq"):
                        t = st[key]
                        if t.dtype != f32:
                            wrong_type = wrong_type or f"state {key} must be float32 (got {t.dtype})"
                        if t.shape != p.shape or not t.is_contiguous() or t.device != p.device:
                            wrong_layout = wrong_layout or (f"state {key} of shape {tuple(t.shape)} (contiguous: {t.is_contiguous()}) "
                                                            f"on {t.device} for a parameter of shape {tuple(p.shape)} on {p.device}")
                    step = st["step"]
                    if step.dtype != f32 or step.device.type != ("cuda" if cap else "cpu"):
                        wrong_layout = wrong_layout or (f"state step must be a float32 tensor on the {'device' if cap else 'CPU'} "
                                                        f"in this form (got {step.dtype} on {step.device}; load_state_dict moves it)")
        for kind, finding in ((TypeError, wrong_type), (NotImplementedError, unsupported), (ValueError, wrong_layout),
                              (ValueError, wrong_device)):
            if finding is not None:
                raise kind(f"bloomscene_amd.optim.Adam: {finding}")
        return work

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("bloomscene_amd.optim.Adam: a closure is not implemented")
        work = self._gather()
        if not work:
            return None
        n = len(work)
        arr = self._descriptors.get(n)
        if arr is None:
            arr = self._descriptors[n] = (AdamTensor * n)()
        group, p = work[0][:2]
        dev, betas, eps, cap = p.device, group["betas"], group["eps"], self._capturable
        keep, steps = [], []
        for d, (group, p, g, st) in zip(arr, work):
            if st is None:
                st = self.state[p]
                st["step"] = torch.zeros((), dtype=torch.float32, device=dev if cap else "cpu")
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)                 # (alive until the launch is queued: torch's allocator is stream-ordered)
            step = st["step"]
            d.p, d.g, d.m, d.v = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            d.numel = p.numel()
            if cap:
                d.lr_dev, d.step_dev = group["lr"].data_ptr(), step.data_ptr()
            else:
                d.lr, d.step = float(group["lr"]), int(step.item()) + 1
                d.lr_dev = d.step_dev = None
                steps.append(step)
        _capi.call("bsr_adam_step", n, arr, betas[0], betas[1], eps, _ops.stream(dev))
        if steps:
            torch._foreach_add_(steps, 1.0)
        return None
