"""Shared by tests/test_encode_nodes_surface.py (CPU) and tests/test_gpu_encode_nodes.py: the
float64 reference of GNN.encode_nodes -- the per-atom embedding hn [N, H] and the reverse mode from
a general cotangent dn [N, H] -- built from oracle/dmpnn_numpy.py as it is, through
tests/encode_common.py: with every atom its own graph (batch = arange(N)) and add pooling, the
pooled fingerprint IS hn and encode_backward(dn) its reverse mode (N oracle.backward calls)."""

from dataclasses import replace

import numpy as np

from encode_common import encode_backward, encode_forward, with_dummy_head
from oracle import dmpnn_numpy as on


def atoms_as_graphs(b):
    """`b` with every atom its own graph: batch = arange(N), ptr = arange(N + 1)."""
    N = b.x.shape[0]
    return replace(b, batch=np.arange(N, dtype=np.int64), ptr=np.arange(N + 1, dtype=np.int64),
                   y=np.zeros(N, np.float32))


def nodes_forward(sd, b, D, act, skip, aggr="add", relu_masks=None):
    """(hn [N, H] float64, cache) of oracle.forward on `b`; the batch's own graphs play no part."""
    g, cache = encode_forward(sd, atoms_as_graphs(b), D, act, skip, aggr, "add", False,
                              relu_masks)
    assert g.shape[0] == b.x.shape[0]
    return g, cache


def nodes_backward(sd, cache, dn):
    """Reverse mode of hn from a general cotangent dn [N, H] (float64): (grads by state_dict
    name, {"x", "edge_attr"}, skip_abs by name), on a cache of nodes_forward.

    Gradients: encode_common.encode_backward, one oracle.backward call per atom.  skip_abs, the
    sum |terms| of each learnable-skip scalar (the conditioning test_gpu_parity.SKIP_COND_U
    scales), cannot be summed over those calls: atoms of one molecule share edges, so the calls'
    terms meet -- and partly cancel -- on the same elements, and the sum of the per-call values
    would overstate it (a wider bar).  It is taken from one more oracle.backward call that sees
    the whole cotangent: oracle.backward forms dg = dy[:, None] * ffn.weight, which numpy
    broadcasting makes exactly dn for dy = ones(N) and ffn.weight = dn [N, H]; whole_backward
    returns that call's gradients too and test_encode_nodes_surface.py holds them equal to the
    per-atom sum."""
    grads, inputs, _ = encode_backward(sd, cache, dn)
    _, _, skip_abs = whole_backward(sd, cache, dn)
    return grads, inputs, skip_abs


def whole_backward(sd, cache, dn):
    """One oracle.backward call with dg = ones(N)[:, None] * dn (see nodes_backward)."""
    dn = np.asarray(dn, np.float64)
    N, H = dn.shape
    assert N == cache["B"] == cache["N"]
    p = with_dummy_head(sd, H)
    p["ffn.weight"] = dn
    io = {}
    cache.pop("skip_abs", None)
    g = on.backward(p, cache, np.ones(N), io)
    return ({k: v for k, v in g.items() if not k.startswith("ffn.")}, io,
            dict(cache.get("skip_abs", {})))
