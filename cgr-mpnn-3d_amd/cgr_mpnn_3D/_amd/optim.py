"""Fused Adam / AMSGrad on the MI355X path: ``torch.optim.Adam`` semantics, one native launch.

The reference trains with ``torch.optim.Adam(model.parameters(), lr=lr,
weight_decay=weight_decay, amsgrad=True)`` (train.py:117-119) plus ``ExponentialLR``
(train.py:121).  torch's foreach implementation runs ~11 multi-tensor kernels per step; this class
keeps the same constructor, ``param_groups`` / ``state`` layout (``step``, ``exp_avg``,
``exp_avg_sq``, ``max_exp_avg_sq``) and update rule, and performs the whole update in
``cgr_adam_step`` (csrc/optim.hip): one kernel over every tensor plus a tiny step-counter
kernel.  Each tensor's ``state["step"]`` lives on the device (like ``capturable=True``), so a training step that
includes ``optimizer.step()`` can be captured into a HIP graph and replayed.  A float ``lr`` is
read from ``param_groups`` at each call (a graph replays the lr it was captured with, as torch's
does); an ``lr`` given as a 0-dim fp32 CUDA tensor, as ``torch.optim.Adam(lr=tensor,
capturable=True)`` takes it, is read on the device by the kernel (``cgr_adam_step_lr_ptr``), so
a scheduler that updates the tensor in place (``ExponentialLR``) is followed by every replay.
Parameters must be fp32 CUDA tensors; there is no CPU fallback.

``max_grad_norm`` (``None``: off, and then the optimizer is exactly the above) adds global L2
gradient clipping with the semantics of ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)``
followed by ``step()``: one norm over every gradient of every param group, ``coef = min(1,
max_grad_norm / (norm + 1e-6))`` applied before ``maximize`` and ``weight_decay``, each group by
its own ``max_grad_norm`` (a group with ``None`` is not scaled; ``float("inf")`` measures and never
clips).  One more native launch per param group (``cgr_grad_sumsq``), no host read, capturable; a
captured step replays the float it was captured with.  Two deviations from torch: ``p.grad`` is
left unscaled (the scaling happens inside the Adam kernel), and a non-finite norm skips the whole
step -- parameters, moments and ``state["step"]`` stay, ``skipped_steps`` counts it.  The norm is
not finite in two cases, and torch differs in each.  With a NaN among the gradients torch's norm
and coefficient are NaN and it writes NaN into every parameter.  With an infinite norm -- an
``inf`` among the gradients, or finite gradients whose squares overflow in fp32 (``|g|`` above
~1.8e19) -- torch's coefficient is 0 and it steps with zeroed gradients (weight decay and the
decaying moments still move the parameters; an ``inf`` element itself becomes ``inf * 0`` = NaN).
``grad_norm`` is the last step's norm before clipping.
"""

from __future__ import annotations

import ctypes
import operator

import torch

from . import native


def _tensor_lr_ptr(lr, dev):
    """A tensor lr is read on the device, never on the host: no sync, and a captured step follows
    a scheduler's in-place updates."""
    if lr.device != dev or lr.dtype != torch.float32 or lr.numel() != 1:
        raise RuntimeError("FusedAdam: a tensor lr must be a 1-element float32 tensor on the "
                           "parameters' device")
    return lr.data_ptr()


def _check_max_grad_norm(v):
    if v is not None and not v > 0.0:  # also NaN
        raise ValueError(f"Invalid max_grad_norm: {v} (None, a float > 0, or inf)")


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 amsgrad=False, *, maximize=False, max_grad_norm=None):
        if isinstance(lr, torch.Tensor):
            if lr.numel() != 1:
                raise ValueError("Tensor lr must be 1-element")
        elif not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        _check_max_grad_norm(max_grad_norm)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                        maximize=maximize, max_grad_norm=max_grad_norm)
        super().__init__(params, defaults)
        self._lib = native.load()

    # -- clipping ----------------------------------------------------------------------------------
    def _clips(self):
        return any(g.get("max_grad_norm") is not None for g in self.param_groups)

    def _clip_scratch(self, dev, partials):
        """The device words of a clipped step, owned here and static across steps (a captured step
        replays on them): the block partials, the norm, the skip count and the gate word.  Grown
        only when a rebuilt pointer table needs more partials than it holds."""
        sc = self.__dict__.get("_cgr_clip")
        if sc is None or sc["norm"].device != dev:
            sc = self.__dict__["_cgr_clip"] = dict(
                norm=torch.zeros((), dtype=torch.float32, device=dev),
                skipped=torch.zeros((), dtype=torch.int64, device=dev),
                gate=torch.zeros(1, dtype=torch.int32, device=dev),
                partials=torch.empty(0, dtype=torch.float32, device=dev))
        if sc["partials"].numel() < partials:
            sc["partials"] = torch.empty(partials, dtype=torch.float32, device=dev)
        return sc

    def _clip_device(self):
        for g in self.param_groups:
            for p in g["params"]:
                if not p.is_cuda:
                    raise RuntimeError("FusedAdam: parameters must be float32 tensors on the GPU")
                return p.device
        return None

    @property
    def grad_norm(self):
        """The last clipped step's total gradient L2 norm before clipping: a 0-dim fp32 device
        tensor with static storage, overwritten by every step and every replay of a captured one
        (reading it is the caller's sync).  None while no param group sets ``max_grad_norm``."""
        if not self._clips():
            return None
        return self._clip_scratch(self._clip_device(), 0)["norm"]

    @property
    def skipped_steps(self):
        """How many clipped steps were skipped because their gradient norm was not finite: a
        0-dim int64 device tensor.  None while no param group sets ``max_grad_norm``."""
        if not self._clips():
            return None
        return self._clip_scratch(self._clip_device(), 0)["skipped"]

    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            if not p.is_cuda or p.dtype != torch.float32:
                raise RuntimeError("FusedAdam: parameters must be float32 tensors on the GPU")
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)  # device, like
            # torch's capturable=True: the native kernel advances it
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        else:  # e.g. after load_state_dict of a torch.optim.Adam state (CPU step tensors)
            for k in ("step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
                v = st.get(k)
                if v is None:
                    st[k] = (torch.zeros((), dtype=torch.float32, device=p.device) if k == "step"
                             else torch.zeros_like(p, memory_format=torch.preserve_format))
                elif v.device != p.device or v.dtype != torch.float32 or not v.is_contiguous():
                    st[k] = v.to(device=p.device, dtype=torch.float32).contiguous()
        return st

    _STATE_KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq", "step")

    def _table(self, gi, params, grads):
        """The group's CgrAdamTensor table.  Built once and kept while the group's parameters,
        their state tensors and the state dict itself are the same objects (load_state_dict
        replaces the dict, so it rebuilds); per step only the parameter and gradient pointers are
        rewritten.  Every gradient is still checked (fp32, contiguous) each step."""
        for g in grads:
            if g.dtype != torch.float32 or not g.is_contiguous():
                raise RuntimeError("FusedAdam: contiguous float32 params/grads required")
        cache = self.__dict__.setdefault("_cgr_tables", {})
        hit = cache.get(gi)
        if hit is not None:
            state, ps, sts, tab, _ = hit
            ok = state is self.state and len(ps) == len(params)
            if ok:
                for p, q, s in zip(params, ps, sts):
                    st = state.get(p)
                    if p is not q or st is None or \
                            not all(map(operator.is_, map(st.get, self._STATE_KEYS), s)):
                        ok = False
                        break
            if ok:
                for i, (p, g) in enumerate(zip(params, grads)):
                    e = tab[i]
                    if e.numel != p.numel():  # p.data was replaced by a tensor of another size
                        ok = False
                        break
                    e.param, e.grad = p.data_ptr(), g.data_ptr()
            if ok:
                return tab
        sts = []
        tab = (native.CgrAdamTensor * len(params))()
        for i, (p, g) in enumerate(zip(params, grads)):
            st = self._init_state(p)
            if not p.is_contiguous():
                raise RuntimeError("FusedAdam: contiguous float32 params/grads required")
            s = tuple(st[k] for k in self._STATE_KEYS)
            sts.append(s)
            tab[i] = native.CgrAdamTensor(p.data_ptr(), g.data_ptr(), s[0].data_ptr(),
                                          s[1].data_ptr(), s[2].data_ptr(), s[3].data_ptr(),
                                          p.numel())
        dev = params[0].device
        if any(p.device != dev for p in params):
            raise RuntimeError("FusedAdam: all parameters of a group must be on one device")
        # (the table's block count: the partials a clipped step's sum of squares writes for it)
        cache[gi] = (self.state, list(params), sts, tab,
                     int(self._lib.cgr_grad_sumsq_partials(tab, len(params))))
        return tab

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.pop("_cgr_tables", None)
        for group in self.param_groups:  # a state dict saved before max_grad_norm existed
            group.setdefault("max_grad_norm", None)

    def _step_clipped(self):
        """The step with global gradient-norm clipping: one sum-of-squares launch per table into
        the partials, then the clipped update of every group; the first update launch finalises
        the norm on the device.  Nothing is read back and, once warm, nothing is allocated."""
        work = []
        dev = None
        need = 0
        for gi, group in enumerate(self.param_groups):
            _check_max_grad_norm(group.get("max_grad_norm"))
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            tab = self._table(gi, ps, [p.grad for p in ps])
            if dev is None:
                dev = ps[0].device
            elif ps[0].device != dev:
                raise RuntimeError("FusedAdam: max_grad_norm needs every param group on one "
                                   "device (one global norm)")
            blocks = self._cgr_tables[gi][4]
            work.append((group, tab, len(ps), need, blocks))
            need += blocks
        if not work:
            return
        sc = self._clip_scratch(dev, need)
        partials = sc["partials"]
        base, cap = partials.data_ptr(), partials.numel()
        lib = self._lib
        with native.device_guard(dev):
            stream = native.stream_ptr(dev)
            for group, tab, n, off, blocks in work:
                native.check(lib.cgr_grad_sumsq(tab, n, base + 4 * off, cap - off, stream))
            first = True
            for group, tab, n, off, blocks in work:
                lr = group["lr"]
                if isinstance(lr, torch.Tensor):
                    lr_host, lr_dev = 0.0, _tensor_lr_ptr(lr, dev)
                else:
                    lr_host, lr_dev = float(lr), None
                mg = group.get("max_grad_norm")
                clip = native.CgrAdamClip(base, need if first else 0, sc["norm"].data_ptr(),
                                          sc["gate"].data_ptr(), sc["skipped"].data_ptr(),
                                          0.0 if mg is None else float(mg))
                first = False
                beta1, beta2 = group["betas"]
                native.check(lib.cgr_adam_step_clip(
                    tab, n, lr_host, lr_dev, float(beta1), float(beta2), float(group["eps"]),
                    float(group["weight_decay"]), int(bool(group["amsgrad"])),
                    int(bool(group["maximize"])), ctypes.byref(clip), stream))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._clips():
            self._step_clipped()
            return loss
        for gi, group in enumerate(self.param_groups):
            ps = group["params"]
            grads = [p.grad for p in ps]
            if any(g is None for g in grads):
                ps = [p for p, g in zip(ps, grads) if g is not None]
                grads = [g for g in grads if g is not None]
            if not ps:
                continue
            beta1, beta2 = group["betas"]
            tab = self._table(gi, ps, grads)
            dev = ps[0].device
            lr = group["lr"]
            if isinstance(lr, torch.Tensor):
                entry, lr_arg = self._lib.cgr_adam_step_lr_ptr, _tensor_lr_ptr(lr, dev)
            else:
                entry, lr_arg = self._lib.cgr_adam_step, float(lr)
            with native.device_guard(dev):
                native.check(entry(
                    tab, len(ps), lr_arg, float(beta1), float(beta2),
                    float(group["eps"]), float(group["weight_decay"]),
                    int(bool(group["amsgrad"])), int(bool(group["maximize"])),
                    native.stream_ptr(dev)))
        return loss
