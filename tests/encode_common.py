"""Shared by tests/test_encode_surface.py (CPU) and tests/test_gpu_encode.py: the float64 reference
of GNN.encode -- the pooled fingerprint g and the reverse mode from a general cotangent dg [B, H]
-- built from oracle/dmpnn_numpy.py as it is, and the small batches the encode tests run on."""

from dataclasses import replace

import numpy as np

from cgr_mpnn_3D._amd.synth import RxnBatch, make_batch
from oracle import dmpnn_numpy as on


def with_dummy_head(sd, H):
    """`sd` with a zero Linear(H, 1) head: oracle.forward reads ffn.weight / ffn.bias for its y,
    which the encode reference ignores (the model's own ffn may be any module)."""
    p = {k: v for k, v in sd.items() if not k.startswith("ffn.")}
    p["ffn.weight"] = np.zeros((1, H))
    p["ffn.bias"] = np.zeros(1)
    return p


def encode_forward(sd, b, D, act, skip, aggr="add", pool="add", batch_none=False, relu_masks=None):
    """(g [B, H] float64, cache) of oracle.forward on batch `b`."""
    H = np.asarray(sd["edge_to_node.bias"]).shape[0]
    _, cache = on.forward(with_dummy_head(sd, H), b.x, b.edge_index, b.edge_attr,
                          None if batch_none else b.batch, D, act, skip,
                          None if batch_none else b.num_graphs, relu_masks=relu_masks, aggr=aggr,
                          pool=pool)
    return cache["g"], cache


def encode_backward(sd, cache, dg):
    """Reverse mode of the fingerprint from a general cotangent dg [B, H] (float64).

    oracle.backward starts from dy [B] and reads wf = params["ffn.weight"] at call time; it is
    linear in dg = dy (x) wf.  So: one call per graph b with ffn.weight = dg[b:b+1] and dy = e_b,
    results summed, ffn entries dropped.  Returns (grads by state_dict name, {"x", "edge_attr"},
    skip_abs by name).  skip_abs: sum |terms| of each learnable-skip scalar -- graphs share no
    edge, so graph b's terms live on its own edges and the per-call values add up exactly."""
    dg = np.asarray(dg, np.float64)
    B, H = dg.shape
    assert B == cache["B"]
    base = with_dummy_head(sd, H)
    grads, inputs, skip_abs = {}, {}, {}
    for bi in range(B):
        p = dict(base)
        p["ffn.weight"] = dg[bi:bi + 1]
        e = np.zeros(B)
        e[bi] = 1.0
        io = {}
        cache.pop("skip_abs", None)
        g = on.backward(p, cache, e, io)
        for k, v in g.items():
            if k.startswith("ffn."):
                continue
            grads[k] = grads.get(k, 0.0) + v
        for k, v in io.items():
            inputs[k] = inputs.get(k, 0.0) + v
        for k, v in cache.get("skip_abs", {}).items():
            skip_abs[k] = skip_abs.get(k, 0.0) + v
    return grads, inputs, skip_abs


def general_dg(B, H, seed=20262):
    """A general cotangent: standard normal times magnitudes over three decades, per element
    (stagewise_common.mixed_dy's recipe on [B, H])."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, H)) * 10.0 ** rng.uniform(-2.0, 1.0, (B, H))).astype(
        np.float32)


def _concat(parts):
    """Collate (x, edge_index, edge_attr) graphs into one RxnBatch."""
    xs, eis, eas, bs, ptr, off = [], [], [], [], [0], 0
    for g, (x, ei, ea) in enumerate(parts):
        xs.append(x)
        eis.append(ei + off)
        eas.append(ea)
        bs.append(np.full(x.shape[0], g, np.int64))
        off += x.shape[0]
        ptr.append(off)
    rng = np.random.default_rng(len(parts))
    return RxnBatch(x=np.ascontiguousarray(np.concatenate(xs, 0)),
                    edge_index=np.ascontiguousarray(np.concatenate(eis, 1)),
                    edge_attr=np.ascontiguousarray(np.concatenate(eas, 0)),
                    batch=np.concatenate(bs, 0), ptr=np.asarray(ptr, np.int64),
                    y=rng.normal(80.0, 20.0, len(parts)).astype(np.float32))


def ragged_batch(seed=7, atoms=(20, 1, 27, 9, 16), n_mace=None, fe0=False):
    """B = 5 ragged reactions, one of them a single atom without bonds (not the last: the
    reference's scatter size needs the batch's last node to have an in-edge).  N = 73: three
    32-row slabs of the dzn kernel, the last partial.  F odd, Fe = 14 (fe0: no edge features)."""
    base_f = make_batch(1, n_atoms=2, n_bonds=1, n_mace=0, seed=0).x.shape[1]
    if n_mace is None:
        n_mace = 3 if base_f % 2 == 0 else 2
    parts = []
    for g, A in enumerate(atoms):
        if A == 1:
            rng = np.random.default_rng(seed + 100)
            parts.append((rng.standard_normal((1, base_f + n_mace)).astype(np.float32),
                          np.zeros((2, 0), np.int64), np.zeros((0, 14), np.float32)))
            continue
        o = make_batch(1, n_atoms=A, n_bonds=A + 2, n_mace=n_mace, seed=seed + g)
        parts.append((o.x, o.edge_index, o.edge_attr))
    b = _concat(parts)
    assert b.x.shape[1] % 2 == 1
    if fe0:
        b = replace(b, edge_attr=np.zeros((b.edge_index.shape[1], 0), np.float32))
    return b
