"""Heads that replace ``GNN.ffn`` on native kernels.

``MeanVarianceHead`` predicts a mean and a variance per reaction from the pooled fingerprint
(``GNN.encode``), the head of a heteroscedastic regression trained with ``GaussianNLLLoss``
(``_amd/loss.py``)::

    model.ffn = MeanVarianceHead(H)
    out = model(batch)                     # [B, 2]: out[:, 0] the mean, out[:, 1] the variance
    loss = GaussianNLLLoss("sum")(out, batch.y)

One launch each way (``cgr_meanvar_head_forward`` / ``_backward``); deterministic, and a graph's
row is the same bits alone or in any batch.
"""

from __future__ import annotations

import math

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import native


class _MeanVarFunction(torch.autograd.Function):
    """``out [B, 2] = f(g, w_mu, b_mu, w_var, b_var, min_var)``; not differentiable twice."""

    @staticmethod
    def forward(ctx, g, w_mu, b_mu, w_var, b_var, min_var):
        lib = native.load()
        B, H = g.shape
        out = torch.empty((B, 2), dtype=torch.float32, device=g.device)
        raw = torch.empty((B,), dtype=torch.float32, device=g.device)
        with native.device_guard(g.device):
            native.check(lib.cgr_meanvar_head_forward(
                native.ptr(g), g.stride(0), B, H, native.ptr(w_mu), native.ptr(b_mu),
                native.ptr(w_var), native.ptr(b_var), min_var, native.ptr(out), native.ptr(raw),
                native.stream_ptr(g.device)))
        ctx.save_for_backward(g, w_mu, w_var, raw)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lib = native.load()
        g, w_mu, w_var, raw = ctx.saved_tensors
        B, H = g.shape
        dout = dout.contiguous()
        if dout.dtype != torch.float32:
            dout = dout.float()
        need = ctx.needs_input_grad
        dg = torch.empty((B, H), dtype=torch.float32, device=g.device) if need[0] else None
        dW = torch.empty((2, H), dtype=torch.float32, device=g.device) \
            if need[1] or need[3] else None
        db = torch.empty((2,), dtype=torch.float32, device=g.device) \
            if need[2] or need[4] else None
        with native.device_guard(g.device):
            native.check(lib.cgr_meanvar_head_backward(
                native.ptr(g), g.stride(0), B, H, native.ptr(w_mu), native.ptr(w_var),
                native.ptr(raw), native.ptr(dout), native.ptr(dg), native.ptr(dW), native.ptr(db),
                native.stream_ptr(g.device)))
        return (dg,
                dW[0].view(w_mu.shape) if need[1] else None, db[0:1] if need[2] else None,
                dW[1].view(w_var.shape) if need[3] else None, db[1:2] if need[4] else None,
                None)


class MeanVarianceHead(nn.Module):
    """``forward(g [B, H]) -> [B, 2]``: column 0 the mean ``mean(g)``, column 1 the variance
    ``softplus(var(g)) + min_var`` (> 0; torch's softplus, beta 1, threshold 20).  Parameters
    ``mean = nn.Linear(hidden, 1)`` and ``var = nn.Linear(hidden, 1)``.  Use as
    ``model.ffn = MeanVarianceHead(H)``: ``GNN.forward`` then returns ``[B, 2]``.  fp32 tensors on
    the GPU only (no CPU fallback)."""

    def __init__(self, hidden: int, min_var: float = 1e-6):
        super().__init__()
        min_var = float(min_var)
        if not 0.0 <= min_var < math.inf:  # also NaN
            raise ValueError(f"MeanVarianceHead: min_var must be finite and >= 0, got {min_var}")
        self.min_var = min_var
        self.mean = nn.Linear(hidden, 1)
        self.var = nn.Linear(hidden, 1)

    def forward(self, g):
        ps = (self.mean.weight, self.mean.bias, self.var.weight, self.var.bias)
        if not (g.is_cuda and all(p.is_cuda for p in ps)):
            raise RuntimeError(
                "cgr_mpnn_3D MeanVarianceHead runs on the GPU only (no CPU fallback)")
        if g.dtype != torch.float32 or any(p.dtype != torch.float32 for p in ps):
            raise TypeError("cgr_mpnn_3D MeanVarianceHead: fp32 tensors required")
        H = self.mean.in_features
        if g.dim() != 2 or g.shape[1] != H:
            raise ValueError(f"MeanVarianceHead: g must be [B, {H}], got {tuple(g.shape)}")
        if any(p.device != g.device for p in ps):
            raise RuntimeError(f"MeanVarianceHead: parameters and g ({g.device}) on different "
                               "devices")
        if g.stride(1) != 1 or g.stride(0) < H:
            g = g.contiguous()
        ps = [p if p.is_contiguous() else p.contiguous() for p in ps]
        return _MeanVarFunction.apply(g, *ps, self.min_var)
