"""``MSELoss`` on the native kernels (``cgr_mse_loss_forward`` / ``_backward``): a drop-in for the
``torch.nn.MSELoss(reduction="sum")`` that train.py:120 hands the trainer (trainer.py:142-143),
``reduction="mean"`` too.  Forward and backward are one launch each (torch: four kernels), so the
captured training step carries two launches for its loss instead of five.  Same values as torch up
to the summation order; deterministic.

``L1Loss`` and ``HuberLoss`` stand beside it for targets with outliers (``cgr_l1_loss_*``,
``cgr_huber_loss_*``): drop-ins for ``torch.nn.L1Loss`` / ``torch.nn.HuberLoss``, the same two
launches, the same input checks.  All three take an optional per-element ``weight``
(``cgr_weighted_loss_*``), and ``GaussianNLLLoss`` (``cgr_gaussian_nll_loss_*``) is the loss of a
mean-variance head (``_amd/heads.py``): the same two launches again."""

from __future__ import annotations

import torch
from torch import nn

from . import config as _config
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


_WEIGHTED_KINDS = {"mse": 0, "l1": 1, "huber": 2}  # enum cgr_weighted_loss


class _WeightedLossFunction(torch.autograd.Function):
    """``_LossFunction`` with a per-element weight (``cgr_weighted_loss_forward`` /
    ``_backward``); the weight is not differentiable."""

    @staticmethod
    def forward(ctx, input, target, weight, mean, kind, delta):
        lib = native.load()
        x, t, w = input.contiguous(), target.contiguous(), weight.contiguous()
        out = torch.empty((), dtype=torch.float32, device=x.device)
        with native.device_guard(x.device):
            native.check(lib.cgr_weighted_loss_forward(
                _WEIGHTED_KINDS[kind], native.ptr(x), native.ptr(t), native.ptr(w), x.numel(),
                int(mean), delta, native.ptr(out), native.stream_ptr(x.device)))
        ctx.save_for_backward(x, t, w)
        ctx.mean, ctx.kind, ctx.delta = mean, kind, delta
        return out

    @staticmethod
    def backward(ctx, grad):
        lib = native.load()
        x, t, w = ctx.saved_tensors
        g = grad.contiguous().float()
        gi = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        with native.device_guard(x.device):
            native.check(lib.cgr_weighted_loss_backward(
                _WEIGHTED_KINDS[ctx.kind], native.ptr(x), native.ptr(t), native.ptr(w),
                native.ptr(g), x.numel(), int(ctx.mean), ctx.delta, native.ptr(gi),
                native.ptr(gt), native.stream_ptr(x.device)))
        return gi, gt, None, None, None, None


def _check_pair(name, input, target):
    if not (input.is_cuda and target.is_cuda):
        raise RuntimeError(f"cgr_mpnn_3D {name} runs on the GPU only (no CPU fallback)")
    if input.shape != target.shape:
        raise ValueError(f"{name}: input {tuple(input.shape)} and target "
                         f"{tuple(target.shape)} must have the same shape (no broadcasting)")
    if input.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(f"cgr_mpnn_3D {name}: fp32 tensors required")
    if input.device != target.device:
        raise RuntimeError(f"{name}: input and target on different devices")


def _check_weight(name, weight, target):
    """A per-element weight: fp32, on the target's device, one per element."""
    if not weight.is_cuda:
        raise RuntimeError(f"cgr_mpnn_3D {name} runs on the GPU only (no CPU fallback)")
    if weight.dtype != torch.float32:
        raise TypeError(f"cgr_mpnn_3D {name}: fp32 weight required")
    if weight.device != target.device:
        raise RuntimeError(f"{name}: weight and target on different devices")
    if weight.numel() != target.numel():
        raise ValueError(f"{name}: weight {tuple(weight.shape)} must have one element per "
                         f"element of target {tuple(target.shape)}")


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

    def forward(self, input, target, weight=None):
        """``weight`` [n] (optional, not differentiable): the loss is ``sum(weight * term)``
        (``/ n`` for the mean, as torch's weighted losses divide); an element of weight 0 is
        skipped, so whatever it holds (NaN, inf) reaches neither the loss nor a gradient.
        Without a weight: the unweighted kernels, as before."""
        name = type(self).__name__
        _check_pair(name, input, target)
        if weight is None:
            return _LossFunction.apply(input, target, self.reduction == "mean", self._kind,
                                       self._extra())
        _check_weight(name, weight, target)
        return _WeightedLossFunction.apply(input, target, weight, self.reduction == "mean",
                                           self._kind, getattr(self, "delta", 0.0))


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


class _GaussianNLLFunction(torch.autograd.Function):
    """``loss = f(mu, var, target, weight, ...)`` on ``cgr_gaussian_nll_loss_forward`` /
    ``_backward``.  ``pair``: ``mu`` is the head's ``[n, 2]`` output, read in place (``var`` is
    None), and its gradient is one ``[n, 2]`` tensor."""

    @staticmethod
    def forward(ctx, mu, var, target, weight, pair, mean, full, eps):
        lib = native.load()
        mu, t = mu.contiguous(), target.contiguous()
        w = None if weight is None else weight.contiguous()
        if pair:
            args = (native.ptr(mu), 2, native.ptr(mu) + 4, 2)
        else:
            var = var.contiguous()
            args = (native.ptr(mu), 1, native.ptr(var), 1)
        out = torch.empty((), dtype=torch.float32, device=mu.device)
        with native.device_guard(mu.device):
            native.check(lib.cgr_gaussian_nll_loss_forward(
                *args, native.ptr(t), native.ptr(w), t.numel(), int(mean), int(full), eps,
                native.ptr(out), native.stream_ptr(mu.device)))
        ctx.save_for_backward(mu, var, t, w)
        ctx.pair, ctx.mean, ctx.eps = pair, mean, eps
        return out

    @staticmethod
    def backward(ctx, grad):
        lib = native.load()
        mu, var, t, w = ctx.saved_tensors
        g = grad.contiguous().float()
        need_mu, need_var, need_t = ctx.needs_input_grad[:3]
        gt = torch.empty_like(t) if need_t else None
        if ctx.pair:
            gm = torch.empty_like(mu) if need_mu else None  # [n, 2]: both columns, one launch
            gv = None
            args = (native.ptr(mu), 2, native.ptr(mu) + 4, 2)
            grads = (native.ptr(gm), native.ptr(gm) + 4 if need_mu else None, 2)
        else:
            gm = torch.empty_like(mu) if need_mu else None
            gv = torch.empty_like(var) if need_var else None
            args = (native.ptr(mu), 1, native.ptr(var), 1)
            grads = (native.ptr(gm), native.ptr(gv), 1)
        with native.device_guard(t.device):
            native.check(lib.cgr_gaussian_nll_loss_backward(
                *args, native.ptr(t), native.ptr(w), native.ptr(g), t.numel(), int(ctx.mean),
                ctx.eps, *grads, native.ptr(gt), native.stream_ptr(t.device)))
        return gm, gv, gt, None, None, None, None, None


class GaussianNLLLoss(nn.Module):
    """``torch.nn.GaussianNLLLoss`` for fp32 CUDA tensors; reduction "sum" or "mean".  Two call
    forms::

        loss(input, target, var, weight=None)    # torch's signature: [n] tensors of one shape
        loss(out2, target, weight=None)          # out2 [n, 2] = (mean, variance) per row, as
                                                 # MeanVarianceHead returns it; read in place

    The term is ``0.5 (log v + (input - target)^2 / v)`` with ``v = max(var, eps)`` (+ ``0.5 log
    2 pi`` when ``full``); gradients are torch's, the clamp is not differentiated.  ``weight``
    [n] as in the other native losses: ``sum(weight * term)``, an element of weight 0 is skipped
    whatever it holds -- how ``CapturedTrainer`` removes padded slots (``pads_by_weight``), since
    ``nll(0, 0, var)`` is not 0.  Unlike torch a negative ``var`` is not refused (the check is a
    host sync and would break a captured step); ``CGR_STRICT=1`` checks it, one sync."""

    pads_by_weight = True  # CapturedTrainer: loss(pred, y, weight=mask), not loss(pred * mask, ..)

    def __init__(self, full: bool = False, eps: float = 1e-6, reduction: str = "mean"):
        super().__init__()
        if reduction not in ("sum", "mean"):
            raise NotImplementedError(
                f"cgr_mpnn_3D GaussianNLLLoss: reduction={reduction!r} (native: 'sum', 'mean')")
        eps = float(eps)
        if not 0.0 < eps < float("inf"):  # also NaN
            raise ValueError(f"GaussianNLLLoss: eps must be a finite value > 0, got {eps}")
        self.full, self.eps, self.reduction = bool(full), eps, reduction

    def forward(self, input, target, var=None, weight=None):
        name = "GaussianNLLLoss"
        if var is not None and weight is None and input.dim() == target.dim() + 1:
            var, weight = None, var  # loss(out2, target, weight), positionally
        pair = var is None
        if pair:
            if not (input.is_cuda and target.is_cuda):
                raise RuntimeError(f"cgr_mpnn_3D {name} runs on the GPU only (no CPU fallback)")
            if input.dim() != 2 or input.shape[1] != 2 or target.shape != input.shape[:1]:
                raise ValueError(
                    f"{name}: without var, input must be [n, 2] (mean, variance) and target [n]; "
                    f"got {tuple(input.shape)} and {tuple(target.shape)}")
            if input.dtype != torch.float32 or target.dtype != torch.float32:
                raise TypeError(f"cgr_mpnn_3D {name}: fp32 tensors required")
            if input.device != target.device:
                raise RuntimeError(f"{name}: input and target on different devices")
        else:
            _check_pair(name, input, target)
            _check_pair(name, var, target)
        if weight is not None:
            _check_weight(name, weight, target)
        if _config.strict:
            v = input[:, 1] if pair else var
            bad = v < 0 if weight is None else (v < 0) & (weight.reshape(v.shape) != 0)
            if bool(bad.any()):
                raise ValueError(f"{name}: var has negative entry/entries (CGR_STRICT=1)")
        return _GaussianNLLFunction.apply(input, var, target, weight, pair,
                                          self.reduction == "mean", self.full, self.eps)
