"""Pooling functions accepted as ``GNN(pooling_fn=...)`` (the reference default is PyG's
``global_add_pool``, ``GNN.py:5,23,110``; PyG's ``global_mean_pool`` and ``global_max_pool`` are
the others the native head implements).  The native path fuses pooling with the ffn head, so ``pooling_fn`` is only
inspected to select that fused head; these functions also work standalone.

``AttentionPool`` / ``attention_pool`` is the one readout here with parameters of its own: a gated
softmax over each graph's atoms on native kernels (``cgr_attention_pool_forward`` /
``_backward``), applied to the per-atom embedding of ``GNN.encode_nodes``.
"""

from __future__ import annotations

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import config as _config
from . import native


def global_add_pool(x: torch.Tensor, batch: torch.Tensor | None, size: int | None = None):
    """Sum node rows per graph id (PyG semantics: ``batch=None`` -> ``x.sum(-2, keepdim)``)."""
    if batch is None:
        return x.sum(dim=-2, keepdim=x.dim() == 2)
    if size is None:
        size = int(batch.max()) + 1 if batch.numel() else 0
    out = x.new_zeros((size,) + tuple(x.shape[1:]))
    return out.index_add_(0, batch, x)


def global_mean_pool(x: torch.Tensor, batch: torch.Tensor | None, size: int | None = None):
    """Mean of node rows per graph id (PyG semantics: sum / max(count, 1); ``batch=None`` ->
    ``x.mean(-2, keepdim)``)."""
    if batch is None:
        return x.mean(dim=-2, keepdim=x.dim() == 2)
    if size is None:
        size = int(batch.max()) + 1 if batch.numel() else 0
    out = global_add_pool(x, batch, size)
    cnt = torch.bincount(batch, minlength=size).clamp(min=1).to(x.dtype)
    return out / cnt.view(-1, *([1] * (x.dim() - 1)))


def global_max_pool(x: torch.Tensor, batch: torch.Tensor | None, size: int | None = None):
    """Column-wise max of node rows per graph id (PyG semantics: ``scatter_reduce("amax",
    include_self=False)``, 0 for a graph without nodes; ``batch=None`` -> ``x.max(-2, keepdim)``)."""
    if batch is None:
        return x.max(dim=-2, keepdim=x.dim() == 2)[0]
    if size is None:
        size = int(batch.max()) + 1 if batch.numel() else 0
    idx = batch.view(-1, *([1] * (x.dim() - 1))).expand_as(x)
    out = x.new_zeros((size,) + tuple(x.shape[1:]))
    return out.scatter_reduce(0, idx, x, reduce="amax", include_self=False)


class _AttentionPoolFunction(torch.autograd.Function):
    """``g, alpha = f(x, weight, bias, batch, ptr, mask, B)``; ``alpha`` is not differentiable,
    the backward is not differentiable again."""

    @staticmethod
    def forward(ctx, x, weight, bias, batch, ptr, mask, B):
        lib = native.load()
        N, H = x.shape
        g = torch.empty((B, H), dtype=torch.float32, device=x.device)
        alpha = torch.empty((N,), dtype=torch.float32, device=x.device)
        with native.device_guard(x.device):
            native.check(lib.cgr_attention_pool_forward(
                native.ptr(x), x.stride(0), N, H, native.ptr(batch), native.ptr(ptr), B,
                native.ptr(weight), native.ptr(bias), native.ptr(mask), native.ptr(g),
                native.ptr(alpha), native.stream_ptr(x.device)))
        ctx.save_for_backward(x, weight, batch, ptr, alpha)
        ctx.B, ctx.bias_shape = B, None if bias is None else bias.shape
        ctx.mark_non_differentiable(alpha)
        return g, alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, dg, _dalpha):
        lib = native.load()
        x, weight, batch, ptr, alpha = ctx.saved_tensors
        N, H = x.shape
        B = ctx.B
        dg = dg.contiguous()
        if dg.dtype != torch.float32:
            dg = dg.float()
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dx = torch.empty((N, H), dtype=torch.float32, device=x.device) if need_x else None
        dw = torch.empty_like(weight) if need_w else None
        ws = None
        if need_w:
            ws = torch.empty(max(int(lib.cgr_attention_pool_workspace_bytes(B, H)), 16),
                             dtype=torch.uint8, device=x.device)
        if need_x or need_w:
            with native.device_guard(x.device):
                native.check(lib.cgr_attention_pool_backward(
                    native.ptr(x), x.stride(0), N, H, native.ptr(batch), native.ptr(ptr), B,
                    native.ptr(weight), native.ptr(alpha), native.ptr(dg), native.ptr(dx),
                    native.ptr(dw), native.ptr(ws), native.stream_ptr(x.device)))
        # the softmax is invariant to a shift of every score: d/d bias is exactly 0
        db = x.new_zeros(ctx.bias_shape) if need_b and ctx.bias_shape is not None else None
        return dx, dw, db, None, None, None, None


def attention_pool(x: torch.Tensor, batch: torch.Tensor | None, weight: torch.Tensor,
                   bias: torch.Tensor | None = None, size: int | None = None, *,
                   ptr: torch.Tensor | None = None, mask: torch.Tensor | None = None):
    """Gated-softmax readout ``(g [B, H], alpha [N])`` over each graph's atoms on the native
    kernels::

        s_v     = x[v] . weight + bias
        alpha_v = softmax of s over the unmasked atoms of v's graph   (0 for a masked atom)
        g[b]    = sum over graph b's atoms of alpha_v x[v]

    ``x`` [N, H] fp32 on the GPU; ``batch`` [N] graph ids, **sorted ascending** (the contract of
    ``GNN.forward``; ``None`` = one graph); ``weight`` [H] or [1, H]; ``bias`` [1] or None;
    ``mask`` [N] bool / uint8, true = the atom takes part.  ``size`` is the number of graphs; with
    neither ``size`` nor ``ptr`` [B + 1] it is read from ``batch.max()`` (one device sync, as in
    ``global_add_pool``); with ``ptr`` or ``size`` there is none.  Sortedness of ``batch`` is the
    caller's contract (the kernel finds a graph's atoms by binary search); under ``CGR_STRICT=1``
    an unsorted ``batch`` raises (one sync).  A graph without (unmasked) atoms gives a zero row,
    never NaN.  Differentiable in ``x`` and ``weight``; the gradient of ``bias`` is exactly zero
    (a shift of every score cancels in the softmax); ``alpha`` is returned detached from the
    graph.  Deterministic, no CPU fallback."""
    if not (x.is_cuda and weight.is_cuda):
        raise RuntimeError("cgr_mpnn_3D attention_pool runs on the GPU only (no CPU fallback)")
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or \
            (bias is not None and bias.dtype != torch.float32):
        raise TypeError("cgr_mpnn_3D attention_pool: fp32 tensors required")
    if x.dim() != 2:
        raise ValueError(f"attention_pool: x must be [N, H], got {tuple(x.shape)}")
    N, H = x.shape
    if weight.numel() != H or H == 0:
        raise ValueError(f"attention_pool: x has width {H}, the gate weight "
                         f"{tuple(weight.shape)}")
    if bias is not None and bias.numel() != 1:
        raise ValueError(f"attention_pool: bias must have one element, got {tuple(bias.shape)}")
    dev = x.device
    for name, t in (("bias", bias), ("batch", batch), ("ptr", ptr), ("mask", mask)):
        if t is not None and t.device != dev:
            raise RuntimeError(f"attention_pool: {name} is on {t.device}, x on {dev}")
    if x.stride(1) != 1 or x.stride(0) < H:
        x = x.contiguous()
    if not weight.is_contiguous():
        weight = weight.contiguous()
    if batch is not None:
        if batch.shape != (N,):
            raise ValueError(f"attention_pool: batch must be [{N}], got {tuple(batch.shape)}")
        if batch.dtype != torch.int64 or not batch.is_contiguous():
            batch = batch.to(torch.int64).contiguous()
        if _config.strict and N > 1 and bool((batch[1:] < batch[:-1]).any()):
            raise RuntimeError("attention_pool: batch is not sorted (CGR_STRICT=1)")
    if ptr is not None:
        if ptr.dim() != 1 or ptr.numel() < 1:
            raise ValueError(f"attention_pool: ptr must be [B + 1], got {tuple(ptr.shape)}")
        if ptr.dtype != torch.int64 or not ptr.is_contiguous():
            ptr = ptr.to(torch.int64).contiguous()
        B = ptr.numel() - 1
        if size is not None and int(size) != B:
            raise ValueError(f"attention_pool: size {size} but ptr describes {B} graphs")
    elif size is not None:
        B = int(size)
    elif batch is None:
        B = 1
    else:
        B = int(batch.max()) + 1 if N else 0
    if batch is None and ptr is None and B != 1:
        raise ValueError(f"attention_pool: batch=None is one graph, size={B}")
    if mask is not None:
        if mask.shape != (N,) or mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError("attention_pool: mask must be a bool or uint8 tensor [N]")
        mask = mask.contiguous()
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
    return _AttentionPoolFunction.apply(x, weight, bias, batch, ptr, mask, B)


class AttentionPool(nn.Module):
    """``attention_pool`` as a module with its gate ``nn.Linear(hidden, 1)``: usable standalone on
    ``GNN.encode_nodes`` output and as ``GNN(pooling_fn=AttentionPool(H))``, where its parameters
    become the model's (``pooling_fn.gate.weight``, ``pooling_fn.gate.bias``)."""

    def __init__(self, hidden: int):
        super().__init__()
        self.gate = nn.Linear(hidden, 1)

    def forward(self, x, batch, size=None, *, ptr=None, mask=None, return_weights=False):
        g, alpha = attention_pool(x, batch, self.gate.weight, self.gate.bias, size, ptr=ptr,
                                  mask=mask)
        return (g, alpha) if return_weights else g


def is_add_pool(fn) -> bool:
    """True for this module's global_add_pool or PyG's (matched by name, PyG may be absent)."""
    return fn is global_add_pool or getattr(fn, "__name__", "") == "global_add_pool"


def is_mean_pool(fn) -> bool:
    """True for this module's global_mean_pool or PyG's (matched by name)."""
    return fn is global_mean_pool or getattr(fn, "__name__", "") == "global_mean_pool"


def is_max_pool(fn) -> bool:
    """True for this module's global_max_pool or PyG's (matched by name)."""
    return fn is global_max_pool or getattr(fn, "__name__", "") == "global_max_pool"


def pooling_code(fn) -> int:
    """The native head's pooling (include/cgr_mpnn3d.h enum cgr_pooling) for ``pooling_fn``."""
    if is_add_pool(fn):
        return 0
    if is_mean_pool(fn):
        return 1
    if is_max_pool(fn):
        return 2
    raise NotImplementedError(
        f"cgr_mpnn_3D (MI355X): pooling_fn {getattr(fn, '__name__', fn)!r} has no native head; "
        "supported are global_add_pool (the reference default), global_mean_pool and "
        "global_max_pool; any other readout composes in PyTorch on the per-atom embedding, "
        "ffn(pooling_fn(model.encode_nodes(data), data.batch))")


def aggregation_code(aggr) -> int:
    """PyG MessagePassing aggr -> include/cgr_mpnn3d.h enum cgr_aggregation."""
    if aggr in ("add", "sum"):
        return 0
    if aggr == "mean":
        return 1
    raise NotImplementedError(
        f"cgr_mpnn_3D (MI355X): aggr={aggr!r}; the native D-MPNN implements 'add' (= 'sum', the "
        "reference default) and 'mean'")
