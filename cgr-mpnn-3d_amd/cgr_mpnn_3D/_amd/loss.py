"""``MSELoss`` on the native kernels (``cgr_mse_loss_forward`` / ``_backward``): a drop-in for the
``torch.nn.MSELoss(reduction="sum")`` that train.py:120 hands the trainer (trainer.py:142-143),
``reduction="mean"`` too.  Forward and backward are one launch each (torch: four kernels), so the
captured training step carries two launches for its loss instead of five.  Same values as torch up
to the summation order; deterministic.

``L1Loss`` and ``HuberLoss`` stand beside it for targets with outliers (``cgr_l1_loss_*``,
``cgr_huber_loss_*``): drop-ins for ``torch.nn.L1Loss`` / ``torch.nn.HuberLoss``, the same two
launches, the same input checks."""

from __future__ import annotations

import torch
from torch import nn

from . import native


class _LossFunction(torch.autograd.Function):
    """``kind`` names the native pair (``cgr_<kind>_loss_forward`` / ``_backward``); ``extra`` are
    the arguments a loss takes between ``reduction_mean`` and the outputs (Huber's delta)."""

    @staticmethod
    def forward(ctx, input, target, mean, kind, extra):
        lib = native.load()
        x = input.contiguous()
        t = target.contiguous()
        out = torch.empty((), dtype=torch.float32, device=x.device)
        with native.device_guard(x.device):
            native.check(getattr(lib, f"cgr_{kind}_loss_forward")(
                native.ptr(x), native.ptr(t), x.numel(), int(mean), *extra, native.ptr(out),
                native.stream_ptr(x.device)))
        ctx.save_for_backward(x, t)
        ctx.mean, ctx.kind, ctx.extra = mean, kind, extra
        return out

    @staticmethod
    def backward(ctx, grad):
        lib = native.load()
        x, t = ctx.saved_tensors
        g = grad.contiguous().float()
        gi = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        with native.device_guard(x.device):
            native.check(getattr(lib, f"cgr_{ctx.kind}_loss_backward")(
                native.ptr(x), native.ptr(t), native.ptr(g), x.numel(), int(ctx.mean), *ctx.extra,
                native.ptr(gi) if gi is not None else None,
                native.ptr(gt) if gt is not None else None, native.stream_ptr(x.device)))
        return gi, gt, None, None, None


class _NativeLoss(nn.Module):
    _kind = None

    def __init__(self, reduction: str = "mean"):
        super().__init__()
        if reduction not in ("sum", "mean"):
            raise NotImplementedError(
                f"cgr_mpnn_3D {type(self).__name__}: reduction={reduction!r} "
                f"(native: 'sum', 'mean')")
        self.reduction = reduction

    def _extra(self):
        return ()

    def forward(self, input, target):
        name = type(self).__name__
        if not (input.is_cuda and target.is_cuda):
            raise RuntimeError(f"cgr_mpnn_3D {name} runs on the GPU only (no CPU fallback)")
        if input.shape != target.shape:
            raise ValueError(f"{name}: input {tuple(input.shape)} and target "
                             f"{tuple(target.shape)} must have the same shape (no broadcasting)")
        if input.dtype != torch.float32 or target.dtype != torch.float32:
            raise TypeError(f"cgr_mpnn_3D {name}: fp32 tensors required")
        if input.device != target.device:
            raise RuntimeError(f"{name}: input and target on different devices")
        return _LossFunction.apply(input, target, self.reduction == "mean", self._kind,
                                   self._extra())


class MSELoss(_NativeLoss):
    """``torch.nn.MSELoss`` for fp32 CUDA tensors of one shape; reduction "sum" or "mean"."""

    _kind = "mse"


class L1Loss(_NativeLoss):
    """``torch.nn.L1Loss`` for fp32 CUDA tensors of one shape; reduction "sum" or "mean".  The
    gradient is ``sign(input - target)``, 0 where they are equal."""

    _kind = "l1"


class HuberLoss(_NativeLoss):
    """``torch.nn.HuberLoss`` for fp32 CUDA tensors of one shape; reduction "sum" or "mean";
    quadratic inside ``|input - target| < delta``, linear outside."""

    _kind = "huber"

    def __init__(self, reduction: str = "mean", delta: float = 1.0):
        super().__init__(reduction)
        delta = float(delta)
        if not 0.0 < delta < float("inf"):  # also NaN
            raise ValueError(f"HuberLoss: delta must be a finite value > 0, got {delta}")
        self.delta = delta

    def _extra(self):
        return (self.delta,)
