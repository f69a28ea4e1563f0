"""ORACLE (test infrastructure only) - one-step float64 references of every kernel stage.

``oracle/dmpnn_numpy.py`` restates the whole model; a test that compares only predictions and
gradients with it lets a one-element error of a single kernel hide behind the pooling and the
matrix products that follow.  Here every stage of the forward and the backward is a function of
*that stage's own inputs* (whatever ran upstream produced them, e.g. the arena buffers of a GPU
run, in the arena's dst-sorted edge order), so an implementation can be judged stage by stage.

Every stage function returns ``Stage(ref, S, T)``:

* ``ref``  the stage's output, evaluated by ``ops`` (float64 numpy by default);
* ``S``    the same expression with the absolute value of every term -- ``|A| @ |B|.T + |bias| +
           |sigma| |h0|`` -- pushed through later linear steps of a composite stage in absolute
           value and multiplied by ``|act'|`` where the stage applies one (always float64);
* ``T``    the absolute allowance of the activations the stage evaluates: ``tol_act(z)`` for
           ``act(z)``, ``tol_act(z) * |upstream gradient|`` for ``act'(z)``, pushed through later
           linear steps like ``S`` (0 where the stage evaluates none).

``rho(got, stage)`` is the error metric, ``max (|got - ref| - T)+ / (u S)`` with ``u = 2^-24``.
An implementation with fp32-class arithmetic obeys ``rho <= max(8, 4 rho_ref)``, ``rho_ref`` the
metric of an honest fp32 evaluation of the same stage from the same inputs (``ops=F32``, or any
object with the same methods, e.g. one built on torch): see ``bar`` and DESIGN.md §2.

numpy only (scipy, where present, speeds the segment sums up and provides erf through
``dmpnn_numpy``).  ``tests/`` is the only importer.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import dmpnn_numpy as on

U = 2.0 ** -24  # fp32 unit roundoff
Stage = namedtuple("Stage", "ref S T")


# ----------------------------------------------------------------------------------------------
# arithmetic back ends
# ----------------------------------------------------------------------------------------------
class Ops:
    """The arithmetic a stage is evaluated in.  ``Ops(np.float64)`` is the reference; ``Ops(
    np.float32)`` an honest fp32 evaluation (every operand rounded to fp32, BLAS sgemm products,
    sequential fp32 segment sums, blocked pairwise fp32 column and total sums)."""

    def __init__(self, dtype):
        self.dtype = np.dtype(dtype)

    def arr(self, a):
        return np.asarray(a, dtype=self.dtype, order="C")

    def mm(self, a, b):
        """a [m, k] @ b [k, n]"""
        return self.arr(a) @ self.arr(b)

    def segsum(self, vals, index, n):
        """out[index[j]] += vals[j]  (out has n rows)"""
        vals = self.arr(vals)
        index = np.asarray(index, np.int64)
        if on._sp is not None and vals.ndim == 2:
            data = np.ones(index.shape[0], dtype=self.dtype)
            m = on._sp.csr_matrix((data, (index, np.arange(index.shape[0]))),
                                  shape=(n, vals.shape[0]))
            return np.asarray(m @ vals, dtype=self.dtype)
        out = np.zeros((n,) + vals.shape[1:], dtype=self.dtype)
        np.add.at(out, index, vals)
        return out

    def total(self, a):
        return self.arr(a).sum(dtype=self.dtype)

    def colsum(self, a):
        # numpy sums a contiguous axis pairwise in blocks (as a parallel reduction does); down
        # the rows of a C-ordered matrix it would add one row after the other
        return np.ascontiguousarray(self.arr(a).T).sum(axis=1, dtype=self.dtype)

    def act(self, z, name):
        with np.errstate(over="ignore"):  # exp(-z) -> inf -> 1 / inf = 0: the right limit
            return on.act_fwd(self.arr(z), name).astype(self.dtype)

    def act_grad(self, z, name):
        with np.errstate(over="ignore"):
            return on.act_grad(self.arr(z), name).astype(self.dtype)


REF = Ops(np.float64)
F32 = Ops(np.float32)
_f8 = REF.arr


def _abs(a):
    return np.abs(_f8(a))


# ----------------------------------------------------------------------------------------------
# the metric and the bars
# ----------------------------------------------------------------------------------------------
def tol_act(z):
    """Absolute allowance of one activation (or activation derivative, per unit of upstream
    gradient) at pre-activation z: u (8 + |z|) (1 + |z|).  A fast exponent scales its argument
    (about |z| u relative on values up to about |z|), a handful of roundings surround it."""
    z = _abs(z)
    return U * (8.0 + z) * (1.0 + z)


def rho(got, stage, cols=None):
    """(rho, argmax index tuple) of ``got`` against a Stage over the logical columns."""
    ref, S, T = (_f8(stage.ref), np.broadcast_to(_f8(stage.S), np.shape(stage.ref)),
                 np.broadcast_to(_f8(stage.T), np.shape(stage.ref)))
    got = _f8(got)
    if cols is not None:
        got = got[..., :cols]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0, ()
    excess = np.maximum(np.abs(got - ref) - T, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(excess > 0, excess / (U * S), 0.0)  # S == 0: any excess is infinite
    r = np.where(np.isfinite(got), r, np.inf)
    k = int(np.argmax(r))
    return float(r.reshape(-1)[k]), tuple(int(i) for i in np.unravel_index(k, r.shape))


def bar(rho_ref):
    """max(8, 4 rho_ref): 2x for the matrix core's biased alignment rounding and another
    summation order, 2x for a maximum over ~1e6 elements against the reference's maximum over
    the same count; the floor covers stages where fp32's own error is near zero."""
    return max(8.0, 4.0 * float(rho_ref))


# ----------------------------------------------------------------------------------------------
# split-bf16 arithmetic (csrc/gemm_b3.hpp, DESIGN.md §2 "Precision choice")
# ----------------------------------------------------------------------------------------------
def _bf16_rne(x32):
    """fp32 -> nearest-even bf16, returned as fp32 (finite inputs)."""
    b = np.ascontiguousarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def split_pieces(x, n):
    """n bf16 pieces of x (rounded to fp32 first): piece i is the RNE bf16 of the fp32 remainder
    x - p0 - .. - p(i-1); every remainder is exact in fp32."""
    r = np.ascontiguousarray(np.asarray(x), np.float32).copy()
    out = []
    for _ in range(n):
        p = _bf16_rne(r)
        out.append(p)
        r = (r - p).astype(np.float32)  # exact
    return out


NT_TERMS = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))  # three pieces, six products
TN_TERMS = ((0, 0), (0, 1), (1, 0))  # two pieces: hi.hi, hi.lo, lo.hi


def split_matmul(a, b, n, terms):
    """a [m, k] @ b [k, n'] with both operands split into n bf16 pieces and only the piece
    products named in ``terms`` (pairs (piece of a, piece of b)), accumulated in float64."""
    pa = [p.astype(np.float64) for p in split_pieces(a, n)]
    pb = [p.astype(np.float64) for p in split_pieces(b, n)]
    out = 0.0
    for i, j in terms:
        out = out + pa[i] @ pb[j]
    return out


# ----------------------------------------------------------------------------------------------
# forward stages (dmpnn_numpy.forward, one step each; edge rows in dst-sorted order)
# ----------------------------------------------------------------------------------------------
def linear(a, w, bias=None, ops=REF):
    """a @ w.T (+ bias): P = x W0[:, :F]^T, Q = x Wn[:, :F]^T, y = g wf^T + bf."""
    ref = ops.mm(a, ops.arr(w).T)
    S = _abs(a) @ _abs(w).T
    if bias is not None:
        ref = ref + ops.arr(bias)
        S = S + _abs(bias)
    return Stage(ref, S, 0.0)


def edge_init_pre(P, src_s, e_s, w0e, b0, ops=REF):
    """pre0 = P[src] + e_s W0[:, F:]^T + b0."""
    ref = ops.arr(P)[src_s] + ops.arr(b0)
    S = _abs(P)[src_s] + _abs(b0)
    if np.shape(e_s)[1]:
        ref = ref + ops.mm(e_s, ops.arr(w0e).T)
        S = S + _abs(e_s) @ _abs(w0e).T
    return Stage(ref, S, 0.0)


def layer_pre(a, h, h0, src_s, rev_s, w, b, sigma, ops=REF):
    """pre_{l+1} = (a_l[src] - h_l[rev]) W_l^T + b_l + sigma_l h0."""
    a_, h_ = ops.arr(a), ops.arr(h)
    m = a_[src_s] - h_[rev_s]
    sg = ops.arr(sigma)
    ref = ops.mm(m, ops.arr(w).T) + ops.arr(b) + sg * ops.arr(h0)
    S = (_abs(a)[src_s] + _abs(h)[rev_s]) @ _abs(w).T + _abs(b) + abs(float(sigma)) * _abs(h0)
    return Stage(ref, S, 0.0)


def readout_pre(Q, aD, wns, bn, ops=REF):
    """zn = Q + a_D Wn[:, F:]^T + bn."""
    ref = ops.arr(Q) + ops.mm(aD, ops.arr(wns).T) + ops.arr(bn)
    S = _abs(Q) + _abs(aD) @ _abs(wns).T + _abs(bn)
    return Stage(ref, S, 0.0)


def activate(z, act, keep_scale=None, ops=REF):
    """act(z) of a *given* pre-activation (the stored one), times the dropout keep mask / (1 - p)
    where given: no sum, so S = 0 and the allowance is tol_act(z)."""
    ref = ops.act(z, act)
    T = tol_act(z)
    if keep_scale is not None:
        ref = ref * ops.arr(keep_scale)
        T = T * _abs(keep_scale) + U * np.abs(_f8(ref))  # the product's own rounding
    return Stage(ref, 0.0, T)


def relu_of(pre, keep_scale=None, ops=REF):
    """ReLU composed with the stage that forms its pre-activation (ReLU models store no
    pre-activation): 1-Lipschitz, so the pre-activation's S bounds the output's error."""
    ref = np.maximum(pre.ref, 0)
    S, T = _f8(pre.S), pre.T
    if keep_scale is not None:
        ref = ref * ops.arr(keep_scale)
        S = S * _abs(keep_scale)
    return Stage(ref, S, T)


def aggregate(h, dst_s, N, inv_deg=None, ops=REF):
    """a = segsum_dst(h) (* inv_deg under mean aggregation)."""
    ref = ops.segsum(h, dst_s, N)
    S = REF.segsum(_abs(h), dst_s, N)
    if inv_deg is not None:
        ref = ref * ops.arr(inv_deg)[:, None]
        S = S * _abs(inv_deg)[:, None]
    return Stage(ref, S, 0.0)


def pool(hn, node_graph, B, mode="add", inv_cnt=None, ops=REF):
    """g: global add / mean / max pooling of the node activations (max: an exact selection,
    0 for an empty graph)."""
    if mode == "max":
        v = ops.arr(hn)
        ref = np.zeros((B, v.shape[1]), dtype=ops.dtype)
        for b in range(B):
            rows = v[np.asarray(node_graph) == b]
            if rows.shape[0]:
                ref[b] = rows.max(axis=0)
        return Stage(ref, 0.0, 0.0)
    ref = ops.segsum(hn, node_graph, B)
    S = REF.segsum(_abs(hn), node_graph, B)
    if mode == "mean":
        ref = ref * ops.arr(inv_cnt)[:, None]
        S = S * _abs(inv_cnt)[:, None]
    return Stage(ref, S, 0.0)


# ----------------------------------------------------------------------------------------------
# backward stages (dmpnn_numpy.backward, one step each)
# ----------------------------------------------------------------------------------------------
def act_grad_of(z, h, act, ops=REF):
    """act'(z); for ReLU the decision of the implementation under test, h > 0 (z is None)."""
    if act == "relu":
        return (np.asarray(h) > 0).astype(ops.dtype), 0.0
    return ops.act_grad(z, act), tol_act(z)


def head_grads(dy, g, ops=REF):
    """ffn.weight = dy^T g, ffn.bias = sum dy."""
    dy2 = ops.arr(dy)[None, :]
    w = Stage(ops.mm(dy2, g), _abs(dy)[None, :] @ _abs(g), 0.0)
    b = Stage(np.asarray([ops.total(dy)]), np.asarray([_abs(dy).sum()]), 0.0)
    return w, b


def max_pool_share(hn, g, node_graph, batched=True, pool_arg=None):
    """Each node's share of its column's pooled gradient (dmpnn_numpy.forward, max pooling), from
    the implementation's own hn and g."""
    hn, g = _f8(hn), _f8(g)
    gid = np.asarray(node_graph, np.int64)
    if not batched:
        return (pool_arg[gid] == np.arange(hn.shape[0])[:, None]).astype(np.float64)
    eq = hn == g[gid]
    cnt = np.zeros_like(g)
    np.add.at(cnt, gid, eq.astype(np.float64))
    cnt = cnt + (g == 0.0)
    return np.where(eq, 1.0 / np.maximum(cnt[gid], 1.0), 0.0)


def readout_dzn(dy, node_graph, wf, zn, hn, act, inv_cnt=None, share=None, ops=REF):
    """dzn = dy[graph] inv_cnt wf (share) act'(zn): the one stage no implementation has to
    store, so it is always formed here and fed to the stages that consume it."""
    up = ops.arr(dy)[np.asarray(node_graph, np.int64)][:, None]
    if inv_cnt is not None:
        up = up * ops.arr(inv_cnt)[np.asarray(node_graph, np.int64)][:, None]
    up = up * ops.arr(wf).reshape(1, -1)
    if share is not None:
        up = up * ops.arr(share)
    d, t = act_grad_of(zn, hn, act, ops)
    ref = up * d
    return Stage(ref, np.abs(_f8(ref)), t * np.abs(_f8(up)))


def tn(a, b, ops=REF, a_T=0.0):
    """a^T b, a weight gradient: a [R, n] the gradient rows (allowance a_T), b [R, k]."""
    ref = ops.mm(ops.arr(a).T, b)
    S = _abs(a).T @ _abs(b)
    T = (np.broadcast_to(_f8(a_T), np.shape(a)).T @ _abs(b)) if np.any(a_T) else 0.0
    return Stage(ref, S, T)


def tn_emulated(a, b):
    """The split-bf16 weight-gradient arithmetic with exact accumulation: both operands rounded to
    fp32, two bf16 pieces each, the products hi.hi, hi.lo, lo.hi (csrc/gemm_b3.hpp "TN")."""
    return split_matmul(np.asarray(a, np.float32).T, np.asarray(b, np.float32), 2, TN_TERMS)


def colsum(a, ops=REF, a_T=0.0):
    """bias gradients: column sums of the gradient rows."""
    T = np.broadcast_to(_f8(a_T), np.shape(a)).sum(axis=0) if np.any(a_T) else 0.0
    return Stage(ops.colsum(a), _abs(a).sum(axis=0), T)


def skip_grad(dpre, h0, ops=REF):
    """dsigma_l = sum dpre_l * h0 (one scalar)."""
    t = ops.arr(dpre) * ops.arr(h0)
    return Stage(np.asarray(ops.total(t)), np.asarray(np.abs(_f8(dpre) * _f8(h0)).sum()), 0.0)


def message(a, h, src_s, rev_s, ops=REF):
    """m_l = a_l[src] - h_l[rev] (the weight gradients' second operand, recomputed)."""
    return ops.arr(a)[src_s] - ops.arr(h)[rev_s]


def readout_ds(dzn, wns, inv_deg=None, ops=REF):
    """ds = dzn Wn[:, F:] (* inv_deg under mean aggregation: what the top layer gathers)."""
    ref = ops.mm(dzn.ref, wns)
    S = _f8(dzn.S) @ _abs(wns)
    T = np.broadcast_to(_f8(dzn.T), np.shape(dzn.ref)) @ _abs(wns)
    if inv_deg is not None:
        ref = ref * ops.arr(inv_deg)[:, None]
        S, T = S * _abs(inv_deg)[:, None], T * _abs(inv_deg)[:, None]
    return Stage(ref, S, T)


def act_bwd(dh, z, h, act, keep_scale=None, ops=REF):
    """dpre = dh * keep / (1 - p) * act'(z), dh a Stage (or an array: S = |dh|)."""
    if not isinstance(dh, Stage):
        dh = Stage(ops.arr(dh), _abs(dh), 0.0)
    d, t = act_grad_of(z, h, act, ops)
    up = dh.ref if keep_scale is None else dh.ref * ops.arr(keep_scale)
    ks = 1.0 if keep_scale is None else _abs(keep_scale)
    f = np.abs(_f8(d)) * ks
    return Stage(up * d, _f8(dh.S) * f, _f8(dh.T) * f + t * np.abs(_f8(up)))


def layer_dh(dpre, w, src_s, dst_s, rev_s, N, inv_deg=None, ops=REF):
    """dm = dpre_l W_l, da = segsum_src(dm), dh = da[dst] * inv_deg - dm[rev]."""
    dm = ops.mm(dpre, w)
    Sm = _abs(dpre) @ _abs(w)
    da = ops.segsum(dm, src_s, N)
    Sa = REF.segsum(Sm, src_s, N)
    if inv_deg is not None:
        da = da * ops.arr(inv_deg)[:, None]
        Sa = Sa * _abs(inv_deg)[:, None]
    return Stage(da[dst_s] - dm[rev_s], Sa[dst_s] + Sm[rev_s], 0.0)


def edge_init_dh(dpres, sigmas, dh, ops=REF):
    """dh0 + dh_0 = sum_l sigma_l dpre_l + dh (dh: layer_dh of layer 0)."""
    ref, S = dh.ref, _f8(dh.S)
    for dp, sg in zip(dpres, sigmas):
        ref = ref + ops.arr(sg) * ops.arr(dp)
        S = S + abs(float(sg)) * _abs(dp)
    return Stage(ref, S, dh.T)


def input_grads(dpre0, dzn, w0, wn, src_s, perm, N, F, ops=REF):
    """dx = segsum_src(dpre0) W0[:, :F] + dzn Wn[:, :F]; dedge_attr = dpre0 W0[:, F:] in the
    caller's edge order (row perm[i] <- sorted row i)."""
    w0, wn = ops.arr(w0), ops.arr(wn)
    Gs = ops.segsum(dpre0, src_s, N)
    SG = REF.segsum(_abs(dpre0), src_s, N)
    dx = Stage(ops.mm(Gs, w0[:, :F]) + ops.mm(dzn.ref, wn[:, :F]),
               SG @ _abs(w0[:, :F]) + _f8(dzn.S) @ _abs(wn[:, :F]),
               np.broadcast_to(_f8(dzn.T), np.shape(dzn.ref)) @ _abs(wn[:, :F]))
    de_s = ops.mm(dpre0, w0[:, F:])
    Se_s = _abs(dpre0) @ _abs(w0[:, F:])
    de, Se = np.empty_like(de_s), np.empty_like(Se_s)
    de[perm], Se[perm] = de_s, Se_s
    return dx, Stage(de, Se, 0.0)


# ----------------------------------------------------------------------------------------------
# a whole run as a record, and the walk over its stages
# ----------------------------------------------------------------------------------------------
# A record holds what an implementation produced, edge rows in dst-sorted order, logical columns:
#   x, e_s, perm, src_s, dst_s, rev_s, node_graph, B, inv_deg / inv_cnt (None: add), pool_arg,
#   P, Q, pre[0..D] (None entries for ReLU), h[0..D], a[0..D], zn (None for ReLU), hn, g, y,
#   keep[l] (None, or keep mask / (1 - p) of layer l's output h[l+1]), dy, ds, dpre[0..D-1],
#   dpre0, grads {state_dict name: array}, dx / de (None: not computed),
#   tn {"readout" | "layer" | "node": "b3" (split-bf16 two-piece) | "f32"}
# cfg: dict(F, Fe, H, D, act, skip, aggr, pool, batched)
def _weights(params, cfg):
    F, D = cfg["F"], cfg["D"]
    w0, wn = _f8(params["edge_init.weight"]), _f8(params["edge_to_node.weight"])
    sig = [float(np.asarray(params[f"skip_weights.{l}"])) if cfg["skip"] else 1.0
           for l in range(D)]
    return dict(w0x=w0[:, :F], w0e=w0[:, F:], b0=_f8(params["edge_init.bias"]), wnx=wn[:, :F],
                wns=wn[:, F:], bn=_f8(params["edge_to_node.bias"]), w0=w0, wn=wn,
                wl=[_f8(params[f"convs.{l}.lin.weight"]) for l in range(D)],
                bl=[_f8(params[f"convs.{l}.lin.bias"]) for l in range(D)], sig=sig,
                wf=_f8(params["ffn.weight"]), bf=_f8(params["ffn.bias"]))


# bf16 keeps 8 significand bits: |x - bf16(x)| <= 2^-8 |x|.  A two-piece operand x = hi + lo + r
# therefore has |lo| <= 2^-8 |x| and |r| <= 2^-16 |x|.  The three kept products hi.hi + hi.lo +
# lo.hi = (a - ra)(b - rb) - lo_a lo_b, so one product's error is at most (2^-16 + 2^-16 + 2^-16)
# |ab| = 3 * 256 u |ab|: 768 u S for the sum, whatever the signs (reached when one term dominates
# the sum, e.g. a node with a single edge).
TN_SPLIT_WORST = 768.0


# The split-bf16 TN forms its bias rider (the column sums of the gradient-side operand) from the
# operand's two pieces, hi + lo per element (csrc/gemm_b3.hpp): each term is short of x by the
# residual |r| <= 2^-16 |x| = 256 u |x|.
TN_BIAS_WORST = 256.0


def two_piece(a):
    """hi + lo of a's two-piece split (exact in float64)."""
    hi, lo = split_pieces(a, 2)
    return hi.astype(np.float64) + lo.astype(np.float64)


def _tn_bias_stage(a, family, ops, a_T=0.0, a_observed=True):
    """The bias gradient that rides a weight-gradient TN: column sums of fp32 rows on an fp32
    family; of the two-piece rows on a split-bf16 family (judged as _tn_stage judges)."""
    st = colsum(a, ops, a_T)
    if family != "b3":
        return st, None, 0.0
    if not a_observed:
        return st, None, TN_BIAS_WORST
    return st, Stage(colsum(two_piece(a)).ref if ops is REF else st.ref, st.S, st.T), 0.0


def _tn_stage(a, b, family, ops, a_T=0.0, a_observed=True):
    """(stage against fp64, stage against the emulation or None, additive bar term).  An fp32
    family is judged against fp64.  A split-bf16 family is judged against the two-piece emulation
    of the same operands when both are read bit for bit from the record.  Where the gradient-side
    operand is formed inside the kernel (dzn, Gs: stored as split images only) its last bit is
    not observable, and one flipped last bit moves the low piece's rounding by 2^-16 |x|, not by
    2^-24 |x|: no emulation from a re-formed operand reproduces the pieces, so that stage is
    judged against fp64 with the split's worst case added to the bar."""
    st = tn(a, b, ops, a_T)
    if family != "b3":
        return st, None, 0.0
    if not a_observed:
        return st, None, TN_SPLIT_WORST
    return st, Stage(tn_emulated(a, b) if ops is REF else st.ref, st.S, st.T), 0.0


def stages(rec, params, cfg, ops=REF):
    """Yield (name, got, stage, stage_emulated, bar_extra) for every stage of a record, each stage evaluated
    by ``ops`` from the record's own inputs to that stage.  ``stage_emulated`` is not None for the
    weight gradients of a split-bf16 family whose operands the record holds bit for bit: the bar
    applies to it, ``stage`` is reported; ``bar_extra`` is added to the bar (_tn_stage)."""
    W = _weights(params, cfg)
    D, F, act = cfg["D"], cfg["F"], cfg["act"]
    relu = act == "relu"
    N = rec["x"].shape[0]
    src, dst, rev, gid = rec["src_s"], rec["dst_s"], rec["rev_s"], rec["node_graph"]
    inv_deg, inv_cnt = rec.get("inv_deg"), rec.get("inv_cnt")
    h, a, pre, keep = rec["h"], rec["a"], rec["pre"], rec["keep"]

    # ---- forward
    yield "P", rec["P"], linear(rec["x"], W["w0x"], ops=ops), None, 0.0
    yield "Q", rec["Q"], linear(rec["x"], W["wnx"], ops=ops), None, 0.0
    st = edge_init_pre(rec["P"], src, rec["e_s"], W["w0e"], W["b0"], ops)
    if relu:
        yield "h0", h[0], relu_of(st, ops=ops), None, 0.0
    else:
        yield "pre0", pre[0], st, None, 0.0
        yield "h0", h[0], activate(pre[0], act, ops=ops), None, 0.0
    yield "a0", a[0], aggregate(h[0], dst, N, inv_deg, ops), None, 0.0
    for l in range(D):
        st = layer_pre(a[l], h[l], h[0], src, rev, W["wl"][l], W["bl"][l], W["sig"][l], ops)
        if relu:
            yield f"h{l + 1}", h[l + 1], relu_of(st, keep[l], ops), None, 0.0
        else:
            yield f"pre{l + 1}", pre[l + 1], st, None, 0.0
            yield f"h{l + 1}", h[l + 1], activate(pre[l + 1], act, keep[l], ops), None, 0.0
        yield f"a{l + 1}", a[l + 1], aggregate(h[l + 1], dst, N, inv_deg, ops), None, 0.0
    st = readout_pre(rec["Q"], a[D], W["wns"], W["bn"], ops)
    if relu:
        yield "hn", rec["hn"], relu_of(st, ops=ops), None, 0.0
    else:
        yield "zn", rec["zn"], st, None, 0.0
        yield "hn", rec["hn"], activate(rec["zn"], act, ops=ops), None, 0.0
    yield "g", rec["g"], pool(rec["hn"], gid, rec["B"], cfg["pool"], inv_cnt, ops), None, 0.0
    sy = linear(rec["g"], W["wf"], W["bf"], ops)
    yield "y", rec["y"], Stage(sy.ref[:, 0], sy.S[:, 0], 0.0), None, 0.0

    # ---- backward
    if rec.get("dy") is None:
        return
    dy, G = rec["dy"], rec["grads"]
    fw, fb = head_grads(dy, rec["g"], ops)
    yield "ffn.weight", G["ffn.weight"], fw, None, 0.0
    yield "ffn.bias", G["ffn.bias"], fb, None, 0.0
    share = None
    if cfg["pool"] == "max":
        share = max_pool_share(rec["hn"], rec["g"], gid, cfg["batched"], rec.get("pool_arg"))
    dzn = readout_dzn(dy, gid, W["wf"], rec["zn"], rec["hn"], act, inv_cnt, share, ops)
    qn = np.concatenate([_f8(rec["x"]), _f8(a[D])], axis=1)
    st, emu, extra = _tn_stage(dzn.ref, qn, rec["tn"]["readout"], ops, dzn.T, a_observed=False)
    yield "edge_to_node.weight", G["edge_to_node.weight"], st, emu, extra
    st, emu, extra = _tn_bias_stage(dzn.ref, rec["tn"]["readout"], ops, dzn.T, a_observed=False)
    yield "edge_to_node.bias", G["edge_to_node.bias"], st, emu, extra
    yield "ds", rec["ds"], readout_ds(dzn, W["wns"], inv_deg, ops), None, 0.0
    if D > 0:
        yield (f"dpre.{D - 1}", rec["dpre"][D - 1],
               act_bwd(ops.arr(rec["ds"])[dst], pre[D], h[D], act, keep[D - 1], ops), None, 0.0)
    for l in range(D - 1, -1, -1):
        dp = rec["dpre"][l]
        m = message(a[l], h[l], src, rev, ops)
        st, emu, extra = _tn_stage(dp, m, rec["tn"]["layer"], ops)
        yield f"convs.{l}.lin.weight", G[f"convs.{l}.lin.weight"], st, emu, extra
        st, emu, extra = _tn_bias_stage(dp, rec["tn"]["layer"], ops)
        yield f"convs.{l}.lin.bias", G[f"convs.{l}.lin.bias"], st, emu, extra
        if cfg["skip"]:
            yield f"skip_weights.{l}", G[f"skip_weights.{l}"], skip_grad(dp, h[0], ops), None, 0.0
        dh = layer_dh(dp, W["wl"][l], src, dst, rev, N, inv_deg, ops)
        if l > 0:
            yield (f"dpre.{l - 1}", rec["dpre"][l - 1],
                   act_bwd(dh, pre[l], h[l], act, keep[l - 1], ops), None, 0.0)
        else:
            tot = edge_init_dh(rec["dpre"], W["sig"], dh, ops)
            yield "dpre0", rec["dpre0"], act_bwd(tot, pre[0], h[0], act, None, ops), None, 0.0
    dp0 = rec["dpre0"]
    gw0 = _f8(G["edge_init.weight"])
    if cfg["Fe"]:
        yield "edge_init.weight[:, F:]", gw0[:, F:], tn(dp0, rec["e_s"], ops), None, 0.0
    if F:
        Gs = ops.segsum(dp0, src, N)
        st, emu, extra = _tn_stage(Gs, rec["x"], rec["tn"]["node"], ops, a_observed=False)
        st = Stage(st.ref, REF.segsum(_abs(dp0), src, N).T @ _abs(rec["x"]), 0.0)
        yield "edge_init.weight[:, :F]", gw0[:, :F], st, emu, extra
    # db0 rides the edge-feature TN (an fp32 family); without edge features the node TN, whose
    # operand Gs has the same column sums
    st, emu, extra = _tn_bias_stage(dp0, "f32" if cfg["Fe"] else rec["tn"]["node"], ops,
                                    a_observed=False)
    yield "edge_init.bias", G["edge_init.bias"], st, emu, extra
    if rec.get("dx") is not None:
        dx, de = input_grads(dp0, dzn, W["w0"], W["wn"], src, rec["perm"], N, F, ops)
        yield "input:x", rec["dx"], dx, None, 0.0
        if cfg["Fe"]:
            yield "input:edge_attr", rec["de"], de, None, 0.0


def run_chain(params, cfg, x, edge_index, edge_attr, batch, num_graphs, dy=None, ops=REF,
              keep=None, tn_family="f32", inputs=False, hooks=None):
    """A record produced by chaining the stage functions, each fed the previous ones' outputs as
    evaluated by ``ops``: with REF the oracle itself stage by stage, with F32 a stand-in kernel
    (its split-bf16 weight gradients: the two-piece emulation rounded to fp32).  ``keep[l]``: the
    [E, H] keep mask / (1 - p) of layer l in the caller's edge order (or None).  ``hooks``
    {stage name: f(value, record so far) -> value} replace a stage's output before anything
    reads it (the tests' mutations)."""
    hooks = hooks or {}
    D, F, act = cfg["D"], cfg["F"], cfg["act"]
    relu = act == "relu"
    W = _weights(params, cfg)
    N = np.shape(x)[0]
    gp = on.graph_prep(edge_index, N, batch, num_graphs)
    perm, src, dst, rev = gp["perm"], gp["src_s"], gp["dst_s"], gp["rev_s"]
    gid = np.zeros(N, np.int64) if batch is None else np.asarray(batch, np.int64)
    B = int(num_graphs)
    rec = dict(x=ops.arr(x), e_s=ops.arr(edge_attr)[perm], perm=perm, src_s=src, dst_s=dst,
               rev_s=rev, node_graph=gid, B=B, inv_deg=None, inv_cnt=None, pool_arg=None,
               pre=[None] * (D + 1), h=[None] * (D + 1), a=[None] * (D + 1), zn=None,
               keep=[None if keep is None or keep[l] is None else _f8(keep[l])[perm]
                     for l in range(D)],
               dy=None, grads={}, dx=None, de=None,
               tn=dict(readout=tn_family, layer=tn_family, node=tn_family))
    if cfg["aggr"] == "mean":
        rec["inv_deg"] = ops.arr(1.0 / np.maximum(np.bincount(dst, minlength=N)[:N], 1))
    if cfg["pool"] == "mean":
        rec["inv_cnt"] = ops.arr(1.0 / np.maximum(np.bincount(gid, minlength=B)[:B], 1))
    inv_deg, inv_cnt = rec["inv_deg"], rec["inv_cnt"]

    def put(name, value):
        return hooks[name](value, rec) if name in hooks else value

    def act_of(st, name_pre, name_h, keep_l=None):
        if relu:
            return None, put(name_h, relu_of(st, keep_l, ops).ref)
        z = put(name_pre, st.ref)
        return z, put(name_h, activate(z, act, keep_l, ops).ref)

    rec["P"] = put("P", linear(rec["x"], W["w0x"], ops=ops).ref)
    rec["Q"] = put("Q", linear(rec["x"], W["wnx"], ops=ops).ref)
    h, a, pre = rec["h"], rec["a"], rec["pre"]
    pre[0], h[0] = act_of(edge_init_pre(rec["P"], src, rec["e_s"], W["w0e"], W["b0"], ops),
                          "pre0", "h0")
    a[0] = put("a0", aggregate(h[0], dst, N, inv_deg, ops).ref)
    for l in range(D):
        st = layer_pre(a[l], h[l], h[0], src, rev, W["wl"][l], W["bl"][l], W["sig"][l], ops)
        pre[l + 1], h[l + 1] = act_of(st, f"pre{l + 1}", f"h{l + 1}", rec["keep"][l])
        a[l + 1] = put(f"a{l + 1}", aggregate(h[l + 1], dst, N, inv_deg, ops).ref)
    rec["zn"], rec["hn"] = act_of(readout_pre(rec["Q"], a[D], W["wns"], W["bn"], ops), "zn", "hn")
    rec["g"] = put("g", pool(rec["hn"], gid, B, cfg["pool"], inv_cnt, ops).ref)
    if cfg["pool"] == "max" and not cfg["batched"]:
        rec["pool_arg"] = np.argmax(_f8(rec["hn"]), axis=0)[None, :]
    rec["y"] = put("y", linear(rec["g"], W["wf"], W["bf"], ops).ref[:, 0])
    if dy is None:
        return rec

    def tn_of(a_, b_, family):
        if family == "b3" and ops is not REF:
            return tn_emulated(a_, b_).astype(ops.dtype)
        return tn(a_, b_, ops).ref

    def bias_of(a_, family):
        if family == "b3" and ops is not REF:
            return colsum(two_piece(a_)).ref.astype(ops.dtype)
        return colsum(a_, ops).ref

    rec["dy"] = ops.arr(dy)
    G = rec["grads"]
    fw, fb = head_grads(rec["dy"], rec["g"], ops)
    G["ffn.weight"], G["ffn.bias"] = put("ffn.weight", fw.ref), put("ffn.bias", fb.ref)
    share = None
    if cfg["pool"] == "max":
        share = max_pool_share(rec["hn"], rec["g"], gid, cfg["batched"], rec["pool_arg"])
    dzn = readout_dzn(rec["dy"], gid, W["wf"], rec["zn"], rec["hn"], act, inv_cnt, share, ops)
    qn = np.concatenate([rec["x"], a[D]], axis=1)
    G["edge_to_node.weight"] = put("edge_to_node.weight", tn_of(dzn.ref, qn, tn_family))
    G["edge_to_node.bias"] = put("edge_to_node.bias", bias_of(dzn.ref, tn_family))
    rec["ds"] = put("ds", readout_ds(dzn, W["wns"], inv_deg, ops).ref)
    dpre = rec["dpre"] = [None] * D
    if D > 0:
        dpre[D - 1] = put(f"dpre.{D - 1}", act_bwd(rec["ds"][dst], pre[D], h[D], act,
                                                  rec["keep"][D - 1], ops).ref)
    for l in range(D - 1, -1, -1):
        m = message(a[l], h[l], src, rev, ops)
        k = f"convs.{l}.lin."
        G[k + "weight"] = put(k + "weight", tn_of(dpre[l], m, tn_family))
        G[k + "bias"] = put(k + "bias", bias_of(dpre[l], tn_family))
        if cfg["skip"]:
            G[f"skip_weights.{l}"] = put(f"skip_weights.{l}", skip_grad(dpre[l], h[0], ops).ref)
        dh = layer_dh(dpre[l], W["wl"][l], src, dst, rev, N, inv_deg, ops)
        if l > 0:
            dpre[l - 1] = put(f"dpre.{l - 1}", act_bwd(dh, pre[l], h[l], act, rec["keep"][l - 1],
                                                      ops).ref)
        else:
            rec["dpre0"] = put("dpre0", act_bwd(edge_init_dh(dpre, W["sig"], dh, ops), pre[0],
                                                h[0], act, None, ops).ref)
    dp0 = rec["dpre0"]
    gw0 = np.zeros(W["w0"].shape, ops.dtype)
    if cfg["Fe"]:
        gw0[:, F:] = tn(dp0, rec["e_s"], ops).ref
    if F:
        gw0[:, :F] = tn_of(ops.segsum(dp0, src, N), rec["x"], tn_family)
    G["edge_init.weight"] = put("edge_init.weight", gw0)
    G["edge_init.bias"] = put("edge_init.bias", bias_of(dp0, "f32" if cfg["Fe"] else tn_family))
    if inputs:
        dx, de = input_grads(dp0, dzn, W["w0"], W["wn"], src, perm, N, F, ops)
        rec["dx"], rec["de"] = put("input:x", dx.ref), put("input:edge_attr", de.ref)
    return rec


def judge(rec, params, cfg, ops_ref=F32):
    """[{stage, rho, rho_ref, bar, argmax, rho_fp64}] for every stage of a record.  ``rho`` is
    what the bar applies to (against the two-piece emulation for a split-bf16 weight gradient,
    whose error against float64 is reported as ``rho_fp64``); ``rho_ref`` the fp32 evaluation by
    ``ops_ref`` of the same stage from the same inputs."""
    out = []
    for (name, got, st, emu, extra), (_, _, st32, _, _) in zip(stages(rec, params, cfg, REF),
                                                     stages(rec, params, cfg, ops_ref)):
        r64, at = rho(got, st)
        r, at = rho(got, emu) if emu is not None else (r64, at)
        rr, _ = rho(st32.ref, st)
        out.append(dict(stage=name, rho=r, rho_ref=rr, bar=bar(rr) + extra, argmax=list(at),
                        rho_fp64=r64))
    return out


# ----------------------------------------------------------------------------------------------
# the standalone DMPNNConv (csrc/conv.hip), in the caller's edge order
# ----------------------------------------------------------------------------------------------
# A conv record: edge_index [2, E] (reverse-edge pairs 2k, 2k + 1), N, h [E, H], weight [H, H],
# bias [H], inv_deg (None: add; 1 / max(in-degree, 1) under mean), grad_a [N, H] / grad_out [E, H]
# (None: the ABI's NULL), and what the implementation produced: a, out, grad_h, grad_weight,
# grad_bias.
def conv_dh(grad_out, grad_a, w, src, dst, rev, N, inv_deg=None, ops=REF):
    """grad_h = (segsum_src(grad_out W) + grad_a)[dst] * inv_deg - (grad_out W)[rev]: layer_dh
    extended by the grad_a term; a None gradient drops its terms."""
    E = np.shape(dst)[0]
    if grad_out is None:
        z = np.zeros((E, np.shape(w)[1]))
        st = Stage(ops.arr(z), z, 0.0)
    else:
        st = layer_dh(grad_out, w, src, dst, rev, N, inv_deg, ops)
    if grad_a is None:
        return st
    t, St = ops.arr(grad_a)[dst], _abs(grad_a)[dst]
    if inv_deg is not None:
        t = t * ops.arr(inv_deg)[dst][:, None]
        St = St * _abs(inv_deg)[dst][:, None]
    return Stage(st.ref + t, _f8(st.S) + St, 0.0)


def conv_stages(rec, ops=REF):
    """Yield (name, got, stage) for the five stages of a conv record, each evaluated by ``ops``
    from the record's own inputs to it (``out`` and ``grad_weight`` from the record's ``a``)."""
    ei = np.asarray(rec["edge_index"], np.int64)
    src, dst = ei[0], ei[1]
    E, N = src.shape[0], int(rec["N"])
    rev = np.arange(E) ^ 1
    h, w, inv_deg = rec["h"], rec["weight"], rec.get("inv_deg")
    H = np.shape(w)[0]
    yield "a", rec["a"], aggregate(h, dst, N, inv_deg, ops)
    yield "out", rec["out"], layer_pre(rec["a"], h, h, src, rev, w, rec["bias"], 0.0, ops)
    go, ga = rec.get("grad_out"), rec.get("grad_a")
    if go is None:  # exactly zero: any non-zero element is an infinite rho
        yield "grad_weight", rec["grad_weight"], Stage(np.zeros((H, H), ops.dtype), 0.0, 0.0)
        yield "grad_bias", rec["grad_bias"], Stage(np.zeros(H, ops.dtype), 0.0, 0.0)
    else:
        yield "grad_weight", rec["grad_weight"], tn(go, message(rec["a"], h, src, rev, ops), ops)
        yield "grad_bias", rec["grad_bias"], colsum(go, ops)
    yield "grad_h", rec["grad_h"], conv_dh(go, ga, w, src, dst, rev, N, inv_deg, ops)


def conv_chain(edge_index, N, h, weight, bias, grad_a=None, grad_out=None, mean=False, ops=REF,
               hooks=None):
    """A conv record produced by the stage functions evaluated by ``ops`` (REF: the oracle itself;
    F32: a stand-in kernel).  ``hooks`` {stage name: f(value, record so far) -> value} replace a
    stage's output before anything reads it."""
    hooks = hooks or {}
    ei = np.asarray(edge_index, np.int64)
    rec = dict(edge_index=ei, N=int(N), h=ops.arr(h), weight=ops.arr(weight), bias=ops.arr(bias),
               inv_deg=None, grad_a=None if grad_a is None else ops.arr(grad_a),
               grad_out=None if grad_out is None else ops.arr(grad_out),
               a=None, out=None, grad_h=None, grad_weight=None, grad_bias=None)
    if mean:
        rec["inv_deg"] = ops.arr(1.0 / np.maximum(np.bincount(ei[1], minlength=N)[:N], 1))
    gen = conv_stages(rec, ops)
    for name, _, st in gen:  # each stage is evaluated only after its inputs are in the record
        rec[name] = hooks[name](st.ref, rec) if name in hooks else st.ref
    return rec


def conv_judge(rec, ops_ref=F32):
    """judge() for a conv record: [{stage, rho, rho_ref, bar, argmax, rho_fp64}]."""
    out = []
    for (name, got, st), (_, _, st32) in zip(conv_stages(rec, REF), conv_stages(rec, ops_ref)):
        r, at = rho(got, st)
        rr, _ = rho(st32.ref, st)
        out.append(dict(stage=name, rho=r, rho_ref=rr, bar=bar(rr), argmax=list(at), rho_fp64=r))
    return out


def segsum_judge(got, vals, index, nseg, ops_ref=F32):
    """One row for a bare segment sum (cgr_segment_sum): out[index[j]] += vals[j]."""
    st = aggregate(vals, index, nseg)
    r, at = rho(got, st)
    rr, _ = rho(aggregate(vals, index, nseg, ops=ops_ref).ref, st)
    return dict(stage="segment_sum", rho=r, rho_ref=rr, bar=bar(rr), argmax=list(at), rho_fp64=r)
