"""ORACLE (test infrastructure only) - the fused Adam / AMSGrad step (csrc/optim.hip), one step
of one flat array of elements, stage by stage in float64.

Every intermediate of the update is an output of the kernel (``exp_avg``, ``exp_avg_sq``,
``max_exp_avg_sq``, ``param``, ``step``), so every stage is judged from the implementation's own
stored inputs to it, as ``oracle/stagewise.py`` judges the model's stages:
``rho = |got - ref| / (u S) <= max(8, 4 rho_ref)``, ``u = 2^-24``, ``rho_ref`` the same metric of
an honest fp32 evaluation (torch fp32 on the CPU, ``standin_*``) of the same stage from the same
inputs.  A result that is not finite is over any bar.

The constants are cast as the kernel and torch cast them -- ``w1 = float32(1 - b1)``,
``b2f = float32(b2)``, ``w2 = float32(1 - b2)``, ``eps`` and ``wd`` as float32 -- and everything
after that is float64 (``consts(h, cast=False)`` keeps the doubles, for the comparison with
torch's float64 Adam).

  gradient   g_c = coef g;  -g_c under maximize;  g_e = g_c + wd p;  S_g = |coef g| + wd |p|
             coef = min(max_norm / (norm + 1e-6), 1) from the float the implementation stored in
             grad_norm (1 when the group does not clip)
  m          m' = m + w1 (g_e - m)                    S_m = (1 + w1) |m| + w1 S_g
  v          v' = b2f v + w2 g_e^2                    S_v = b2f v + w2 S_g^2
  vmax       exact: max(vmax, v'_stored) under amsgrad, untouched otherwise
  p          bc1 = 1 - b1^(t+1), bc2 = 1 - b2^(t+1), den = sqrt(vv') / sqrt(bc2) + eps,
             upd = (lr / bc1) m' / den, p' = p - upd    S_p = |p| + |upd|
             from the stored m' and vv' (vmax' under amsgrad, v' otherwise)
  step       exact: t + 1

``t`` may be an array (one step count per element: a table whose tensors differ in it).

``VARIANTS`` names one-line deviations of the update and the stages that must flag each;
``replica_step`` is the kernel's ``adam_elem`` in numpy fp32 in the kernel's own operation order
(``fmaf`` where the kernel has one), and takes a variant.  ``norm64`` / ``norm_replica`` are the
global gradient norm in float64 and in the summation structure of ``k_grad_sumsq`` and the
finalising kernel; ``NORM_BAR`` is the relative bar derived from that structure.

numpy and torch (the stand-in) only.  ``tests/`` is the only importer.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from .stagewise import Stage, U, bar, rho

Hyper = namedtuple("Hyper", "b1 b2 eps wd amsgrad maximize",
                   defaults=(0.9, 0.999, 1e-8, 0.0, True, False))
Consts = namedtuple("Consts", "w1 b2f w2 eps wd")

BLOCK = 1024  # elements per block of k_adam / k_grad_sumsq: 256 threads, one float4 each
THREADS = 256

# name: the stages that tell the variant from the update (every other stage stays inside its bar)
VARIANTS = {
    "eps_omitted": ("p",),             # den = sqrt(vv) / sqrt(bc2)
    "eps_in_sqrt": ("p",),             # den = sqrt(vv / bc2 + eps)
    "eps_before_bc2": ("p",),          # den = (sqrt(vv) + eps) / sqrt(bc2)
    "v_for_vmax": ("p",),              # the denominator reads v' under amsgrad
    "bc_at_t": ("p",),                 # bias corrections at t instead of t + 1
    "wd_before_maximize": ("m", "v"),  # g_e = -(coef g + wd p)
    "clip_after_wd": ("m", "v"),       # g_e = coef (+-g + wd p)
    "decoupled_decay": ("m", "v", "p"),  # AdamW: g_e = g_c, p' = p (1 - lr wd) - upd
    "shared_step": ("p",),             # the table's first tensor's step word for every tensor
}


def consts(h, cast=True):
    f = np.float32 if cast else np.float64
    return Consts(*(float(f(x)) for x in (1.0 - h.b1, h.b2, 1.0 - h.b2, h.eps, h.wd)))


def _f8(a):
    return np.asarray(a, np.float64)


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient in float64 from the stored fp32 norm; 1 without a bound."""
    if max_norm is None or not max_norm > 0.0:
        return 1.0
    with np.errstate(all="ignore"):
        return float(np.minimum(np.float64(np.float32(max_norm)) / (np.float64(norm) + 1e-6), 1.0))


def _steps(t, variant):
    """The step count the bias corrections read, float64 (array or scalar)."""
    t = _f8(t)
    if variant == "shared_step" and t.ndim:
        t = np.full_like(t, t.reshape(-1)[0])
    return t if variant == "bc_at_t" else t + 1.0


# -------------------------------------------------------------------------------------------------
# the float64 stages
# -------------------------------------------------------------------------------------------------
def eff_grad(p, g, h, c, coef=1.0, variant=None):
    """(g_e, S_g)"""
    p, g = _f8(p), _f8(g)
    sign = -1.0 if h.maximize else 1.0
    wd = 0.0 if variant == "decoupled_decay" else c.wd
    if variant == "wd_before_maximize":
        ge = sign * (coef * g + wd * p)
    elif variant == "clip_after_wd":
        ge = coef * (sign * g + wd * p)
    else:
        ge = sign * (coef * g) + wd * p
    return ge, np.abs(coef * g) + wd * np.abs(p)


def m_stage(p, g, m, h, c, coef=1.0, variant=None):
    ge, Sg = eff_grad(p, g, h, c, coef, variant)
    m = _f8(m)
    return Stage(m + c.w1 * (ge - m), (1.0 + c.w1) * np.abs(m) + c.w1 * Sg, 0.0)


def v_stage(p, g, v, h, c, coef=1.0, variant=None):
    ge, Sg = eff_grad(p, g, h, c, coef, variant)
    v = _f8(v)
    return Stage(c.b2f * v + c.w2 * ge * ge, c.b2f * np.abs(v) + c.w2 * Sg * Sg, 0.0)


def vmax_stage(vmax, v1, h):
    """Exact: None without amsgrad (untouched: compare the bytes)."""
    return np.maximum(vmax, v1) if h.amsgrad else None


def p_stage(p, m1, v1, vmax1, t, h, c, lr, variant=None):
    """From the stored m' and v' / vmax'; lr a double (the host value, or the device float)."""
    p, m1 = _f8(p), _f8(m1)
    vv = _f8(vmax1 if h.amsgrad and variant != "v_for_vmax" else v1)
    step = _steps(t, variant)
    with np.errstate(all="ignore"):
        bc1 = 1.0 - np.power(h.b1, step)
        bc2 = 1.0 - np.power(h.b2, step)
        if variant == "eps_omitted":
            den = np.sqrt(vv) / np.sqrt(bc2)
        elif variant == "eps_in_sqrt":
            den = np.sqrt(vv / bc2 + c.eps)
        elif variant == "eps_before_bc2":
            den = (np.sqrt(vv) + c.eps) / np.sqrt(bc2)
        else:
            den = np.sqrt(vv) / np.sqrt(bc2) + c.eps
        upd = (lr / bc1) * m1 / den
        p0 = p * (1.0 - lr * c.wd) if variant == "decoupled_decay" else p
        return Stage(p0 - upd, np.abs(p) + np.abs(upd), 0.0)


def step64(p, g, m, v, vmax, t, h, lr, coef=1.0, variant=None, cast=True):
    """The chained float64 step (each stage from the previous stage's float64 result)
    -> dict(p, m, v, vmax)."""
    c = consts(h, cast)
    m1 = m_stage(p, g, m, h, c, coef, variant).ref
    v1 = v_stage(p, g, v, h, c, coef, variant).ref
    vm1 = np.maximum(_f8(vmax), v1) if h.amsgrad else _f8(vmax)
    p1 = p_stage(p, m1, v1, vm1, t, h, c, lr, variant).ref
    return dict(p=p1, m=m1, v=v1, vmax=vm1)


# -------------------------------------------------------------------------------------------------
# the fp32 stand-in that sets rho_ref: the same stages by torch fp32 on the CPU, in the operations
# torch.optim.Adam's single-tensor path applies (add alpha, lerp, mul + addcmul, sqrt / div / add,
# addcdiv), each from the stage's own inputs
# -------------------------------------------------------------------------------------------------
def _t32(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))


def standin_coef(norm, max_norm):
    """The coefficient in fp32: clamp(max_norm / (norm + 1e-6), max=1)."""
    if max_norm is None or not max_norm > 0.0:
        return None
    f = np.float32
    with np.errstate(all="ignore"):
        return np.minimum(f(max_norm) / (f(norm) + f(1e-6)), f(1.0))


def _standin_grad(p, g, h, coef):
    g = _t32(g)
    if coef is not None:
        g = g * float(coef)
    if h.maximize:
        g = -g
    if h.wd != 0.0:
        g = g.add(_t32(p), alpha=h.wd)
    return g


def standin_m(p, g, m, h, coef=None):
    return _t32(m).lerp(_standin_grad(p, g, h, coef), 1.0 - h.b1).numpy()


def standin_v(p, g, v, h, coef=None):
    ge = _standin_grad(p, g, h, coef)
    return _t32(v).mul(h.b2).addcmul_(ge, ge, value=1.0 - h.b2).numpy()


def standin_p(p, m1, v1, vmax1, t, h, lr):
    step = _f8(t) + 1.0
    bc1, bc2 = 1.0 - np.power(h.b1, step), 1.0 - np.power(h.b2, step)
    step_size, bc2_sqrt = lr / bc1, np.sqrt(bc2)
    den = _t32(vmax1 if h.amsgrad else v1).sqrt()
    if np.ndim(step):  # one scalar per element: the doubles rounded to fp32 as a scalar would be
        den = (den / _t32(bc2_sqrt)).add_(h.eps)
        return (_t32(p) - _t32(step_size) * (_t32(m1) / den)).numpy()
    den = (den / float(bc2_sqrt)).add_(h.eps)
    return _t32(p).addcdiv(_t32(m1), den, value=-float(step_size)).numpy()


# -------------------------------------------------------------------------------------------------
# the kernel's adam_elem in numpy fp32, operation by operation
# -------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf on fp32 operands: the product is exact in double, the sum rounds to 53 bits and then
    to 24 (a double rounding that differs from the fused result in about one element in 2^29)."""
    return (_f8(a) * _f8(b) + _f8(c)).astype(np.float32)


def replica_coef(norm, max_norm):
    """k_adam's sc[2] (None: the unclipped kernel, which never multiplies)."""
    return standin_coef(norm, max_norm)


def replica_step(p, g, m, v, vmax, t, h, lr, coef=None, variant=None):
    """adam_elem + the block's scalars (double pow, rounded to fp32) on fp32 arrays
    -> dict(p, m, v, vmax).  ``coef``: an fp32 scalar under cgr_adam_step_clip, else None."""
    f = np.float32
    c = Consts(*(f(x) for x in consts(h)))
    p, g, m, v, vmax = (np.asarray(a, f) for a in (p, g, m, v, vmax))
    with np.errstate(all="ignore"):
        wd = f(0.0) if variant == "decoupled_decay" else c.wd
        if variant == "wd_before_maximize":
            if coef is not None:
                g = g * f(coef)
            if wd != 0:
                g = _fma(p, wd, g)
            if h.maximize:
                g = -g
        elif variant == "clip_after_wd":
            if h.maximize:
                g = -g
            if wd != 0:
                g = _fma(p, wd, g)
            if coef is not None:
                g = g * f(coef)
        else:
            if coef is not None:
                g = g * f(coef)
            if h.maximize:
                g = -g
            if wd != 0:
                g = _fma(p, wd, g)
        m = _fma(c.w1, g - m, m)
        v = _fma(c.w2 * g, g, v * c.b2f)
        vv = v
        if h.amsgrad:
            vmax = np.maximum(vmax, v)
            vv = v if variant == "v_for_vmax" else vmax
        step = _steps(t, variant)
        bc1 = 1.0 - np.power(np.float64(h.b1), step)
        bc2 = 1.0 - np.power(np.float64(h.b2), step)
        nss = np.asarray(-(np.float64(lr) / bc1)).astype(f)
        bc2s = np.sqrt(bc2).astype(f)
        if variant == "eps_omitted":
            den = np.sqrt(vv) / bc2s
        elif variant == "eps_in_sqrt":
            den = np.sqrt(vv / (bc2s * bc2s) + c.eps)
        elif variant == "eps_before_bc2":
            den = (np.sqrt(vv) + c.eps) / bc2s
        else:
            den = np.sqrt(vv) / bc2s + c.eps
        if variant == "decoupled_decay":
            p = p * f(1.0 - np.float64(lr) * np.float64(c.wd))
        p = _fma(nss, m / den, p)
    assert all(a.dtype == f for a in (p, m, v, vmax, den)), "the replica left fp32"
    return dict(p=p, m=m, v=v, vmax=vmax)


# -------------------------------------------------------------------------------------------------
# judging one step
# -------------------------------------------------------------------------------------------------
def _row(stage, got, st, ref32):
    r, at = rho(got, st)
    rr, _ = rho(ref32, st)
    return dict(stage=stage, rho=r, rho_ref=rr, bar=bar(rr), argmax=list(at), rho_fp64=r)


def judge(before, after, t, h, lr, norm=None, max_norm=None):
    """-> ([rows of adam_m, adam_v, adam_p], [what an exact stage got wrong]).

    before: dict(p, g, m, v, vmax) fp32, the step's inputs; after: dict(p, m, v, vmax) fp32, what
    the implementation stored; t: the step count before the step (scalar or per element); lr: the
    double the kernel read.  Clipping: ``norm`` the implementation's stored fp32 grad_norm and
    ``max_norm`` the group's bound."""
    c = consts(h)
    coef = clip_coef(norm, max_norm)
    coef32 = standin_coef(norm, max_norm)
    b, a = before, after
    rows = [
        _row("adam_m", a["m"], m_stage(b["p"], b["g"], b["m"], h, c, coef),
             standin_m(b["p"], b["g"], b["m"], h, coef32)),
        _row("adam_v", a["v"], v_stage(b["p"], b["g"], b["v"], h, c, coef),
             standin_v(b["p"], b["g"], b["v"], h, coef32)),
        _row("adam_p", a["p"], p_stage(b["p"], a["m"], a["v"], a["vmax"], t, h, c, lr),
             standin_p(b["p"], a["m"], a["v"], a["vmax"], t, h, lr)),
    ]
    exact = []
    want = vmax_stage(np.asarray(b["vmax"], np.float32), np.asarray(a["v"], np.float32), h)
    if want is None:
        want = np.asarray(b["vmax"], np.float32)
    got = np.asarray(a["vmax"], np.float32)
    bad = np.flatnonzero(want.view(np.uint32) != got.view(np.uint32))
    if bad.size:
        k = int(bad[0])
        exact.append(f"adam_vmax: {bad.size} elements differ from "
                     f"{'max(vmax, v_stored)' if h.amsgrad else 'the untouched array'}, first at "
                     f"{k}: {got[k]!r} vs {want[k]!r}")
    return rows, exact


def flagged(rows):
    """The short stage names ("m", "v", "p") over their bar."""
    return {r["stage"][len("adam_"):] for r in rows if not r["rho"] <= r["bar"]}


# -------------------------------------------------------------------------------------------------
# the global gradient norm
# -------------------------------------------------------------------------------------------------
# The derived bar.  Every term is a square, so no sum cancels and an error bound by depth holds:
# the float4 path rounds the square, x^2 + y^2 and the sum of the two pairs (3 deep; a contracted
# fma only removes roundings), the scalar path is a chain of four fmaf (4 deep); six levels of the
# wave's butterfly and the two levels of (r0 + r1) + (r2 + r3) follow: 11 and 12 roundings, a
# relative error of the block partial of at most (1 + u)^12 - 1.  The partials are added in double
# (2^-53 per addition: nothing).  The square root halves the relative error, 6u + O(u^2); its own
# rounding in double is nothing, and the rounding of the result to float adds u: 7u + O(u^2), of
# which 50 u^2 + 300 * 2^-53 < 1e-12 bounds the rest.  This needs every square to be a normal
# fp32 number (no underflow), which the norm cases' inputs keep.
NORM_BAR = 7.0 * U + 1e-12


def norm64(grads):
    """float64 L2 norm over every array of ``grads`` (None entries skipped)."""
    return float(np.sqrt(sum(float(np.sum(_f8(g) ** 2)) for g in grads if g is not None)))


def block_partials(g, vec4):
    """k_grad_sumsq's partials of one tensor: fp32, one per block of 1,024 elements."""
    f = np.float32
    g = np.asarray(g, f).reshape(-1)
    n = g.size
    nb = -(-n // BLOCK)
    pad = np.zeros(nb * BLOCK, f)
    pad[:n] = g
    q = pad.reshape(nb, THREADS, 4)
    with np.errstate(over="ignore"):
        sq = q * q
        vec = (sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3])
        # the scalar path: s = fmaf(g, g, s) over the thread's elements that exist (a padded
        # element is 0 and fmaf(0, 0, s) = s, so the chain over all four is the same)
        s = np.zeros((nb, THREADS), f)
        for k in range(4):
            s = _fma(q[..., k], q[..., k], s)
        full = (np.arange(nb)[:, None] * BLOCK + 4 * np.arange(THREADS)[None, :] + 4) <= n
        s = np.where(full & bool(vec4), vec, s).reshape(nb, THREADS // 64, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):  # wave_sum: v += shfl_xor(v, o)
            s = s + s[..., lane ^ o]
        r = s[..., 0]
        return ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])).astype(f)


def finalise(partials):
    """k_adam_step_count_clip's norm from the partials: thread i adds partials i, i + 256, ... in
    double, a 256-wide LDS tree adds the threads, float(sqrt(total))."""
    red = np.zeros(THREADS, np.float64)
    with np.errstate(all="ignore"):
        for i in range(min(THREADS, len(partials))):
            s = 0.0
            for x in partials[i::THREADS]:
                s += float(x)
            red[i] = s
        o = THREADS // 2
        while o > 0:
            red[:o] = red[:o] + red[o:2 * o]
            o //= 2
        return np.float32(np.sqrt(red[0]))


def norm_replica(grads, vec4, variant=None):
    """The kernels' norm of a table's gradients (``vec4[i]``: gradient i is 16-byte aligned).
    variant "drop_last_partial": the last block's partial is never added; "double_tail": the last
    element of the last tensor whose length is no multiple of 4 is counted twice."""
    grads = [np.asarray(g, np.float32).reshape(-1) for g in grads]
    if variant == "double_tail":
        k = max(i for i, g in enumerate(grads) if g.size % 4)
        grads[k] = np.concatenate([grads[k], grads[k][-1:]])
    parts = [block_partials(g, a) for g, a in zip(grads, vec4) if g.size]
    parts = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    if variant == "drop_last_partial":
        parts = parts[:-1]
    return finalise(parts), parts


def norm_row(got, grads):
    """The adam_norm row: the relative error of the stored fp32 norm against float64 in units of
    u, held to NORM_BAR / u (exactly 0 for an exactly zero norm)."""
    ref = norm64(grads)
    got = float(got)
    if ref == 0.0:
        r = 0.0 if got == 0.0 else np.inf
    else:
        r = abs(got - ref) / (U * ref) if np.isfinite(got) else np.inf
    return dict(stage="adam_norm", rho=float(r), rho_ref=0.0, bar=NORM_BAR / U, argmax=[],
                rho_fp64=float(r))
