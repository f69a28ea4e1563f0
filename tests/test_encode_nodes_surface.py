"""CPU: the surface of GNN.encode_nodes, and the pin of its tests' float64 reference
(tests/nodes_common.py: every atom its own graph) to the encode reference (tests/encode_common.py,
itself pinned against finite differences by tests/test_encode_surface.py)."""

import re
from pathlib import Path

import numpy as np
import pytest
import torch

from encode_common import encode_backward, encode_forward, general_dg, ragged_batch
from nodes_common import nodes_backward, nodes_forward, whole_backward
from stagewise_common import random_params
from test_gpu_parity import _sparse_batch

from cgr_mpnn_3D._amd import native
from cgr_mpnn_3D._amd.pool import pooling_code
from cgr_mpnn_3D.models.GNN import GNN

ENTRY_POINTS = ("cgr_gnn_encode_nodes", "cgr_gnn_encode_nodes_backward",
                "cgr_gnn_encode_nodes_input_grads", "cgr_gnn_encode_nodes_predict")

# float64 rounding of two evaluation orders of the same sums (a few hundred terms each)
PIN_BAR = 1e-12

BATCHES = {"ragged": lambda: ragged_batch(),
           "ragged_fe0": lambda: ragged_batch(seed=8, fe0=True),
           "sparse": lambda: _sparse_batch(5, 15, seed=33)}


def _rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-300))


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("kind", list(BATCHES))
def test_nodes_reference_is_pinned_to_the_encode_reference(kind, aggr):
    """H 12, D 2, SiLU, learnable skip.  (1) the atoms-as-graphs fingerprint is the ordinary
    cache's node embedding, exactly; (2) with dn = (dg inv_cnt)[batch] -- what pooling's reverse
    mode hands each atom -- its reverse mode is encode_backward(dg), for add and mean pooling;
    (3) the single whole-cotangent call that supplies skip_abs gives the per-atom sum's
    gradients."""
    H, D = 12, 2
    b = BATCHES[kind]()
    F_, Fe = b.x.shape[1], b.edge_attr.shape[1]
    rng = np.random.default_rng(5)
    sd = {k: np.asarray(v, np.float64) for k, v in random_params(rng, F_, Fe, H, D).items()}
    hn, ncache = nodes_forward(sd, b, D, "silu", True, aggr)
    worst = 0.0
    for pool in ("add", "mean"):
        _, cache = encode_forward(sd, b, D, "silu", True, aggr, pool)
        assert np.array_equal(hn, cache["hnode"])
        dg = general_dg(b.num_graphs, H).astype(np.float64)
        inv_cnt = 1.0 / np.maximum(np.bincount(b.batch, minlength=b.num_graphs), 1) \
            if pool == "mean" else np.ones(b.num_graphs)
        dn = (dg * inv_cnt[:, None])[b.batch]
        g_ref, in_ref, _ = encode_backward(sd, cache, dg)
        g, gin, skip_abs = nodes_backward(sd, ncache, dn)
        gw, ginw, _ = whole_backward(sd, ncache, dn)
        assert set(g) == set(g_ref) == set(gw) and not any(k.startswith("ffn.") for k in g)
        assert set(skip_abs) == {f"skip_weights.{l}" for l in range(D)}
        for k in g_ref:
            worst = max(worst, _rel(g[k], g_ref[k]), _rel(gw[k], g[k]))
        for k in ("x", "edge_attr"):
            if np.size(in_ref[k]):
                worst = max(worst, _rel(gin[k], in_ref[k]), _rel(ginw[k], gin[k]))
    print(f"{kind} aggr={aggr}: worst relative mismatch {worst:.2e}")
    assert worst <= PIN_BAR


def test_whole_cotangent_skip_abs_is_no_larger_than_the_per_atom_sum():
    """sum |sum_v t_v| <= sum_v sum |t_v|: the skip_abs nodes_backward returns is the tighter
    one."""
    H, D = 12, 2
    b = ragged_batch()
    rng = np.random.default_rng(5)
    sd = {k: np.asarray(v, np.float64)
          for k, v in random_params(rng, b.x.shape[1], b.edge_attr.shape[1], H, D).items()}
    _, ncache = nodes_forward(sd, b, D, "silu", True)
    dn = general_dg(b.x.shape[0], H).astype(np.float64)
    _, _, per_atom = encode_backward(sd, ncache, dn)
    _, _, whole = nodes_backward(sd, ncache, dn)
    for k, v in whole.items():
        assert 0.0 < v <= per_atom[k] * (1 + 1e-12), k


def test_the_four_nodes_entry_points_are_declared_and_bound():
    header = (Path(__file__).resolve().parents[1] / "include" / "cgr_mpnn3d.h").read_text()
    lib = native.load()
    bound = {s[0]: s for s in native.SIGNATURES}
    for name in ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name) and name in bound
        # the encode forms, argument for argument
        twin = bound[name.replace("_encode_nodes", "_encode")]
        assert bound[name][1] is twin[1] and bound[name][2] == twin[2], name
    assert lib.cgr_abi_version() == 9


def test_encode_nodes_refuses_cpu_tensors():
    b = ragged_batch(seed=3, atoms=(6, 1, 9, 4, 7))
    m = GNN(b.x.shape[1], 14, depth=2, hidden_sizes=[12, 12])
    with pytest.raises(RuntimeError, match="GPU only"):
        m.encode_nodes(b.to_torch())


def test_a_custom_pooling_fn_keeps_raising_where_the_native_pool_is_chosen():
    """pooling_code is what forward and encode reach (tests/test_gpu_parity.py pins forward's
    NotImplementedError on the GPU); encode_nodes does not call it.  The message now names the
    way out."""
    m = GNN(9, 4, depth=2, hidden_sizes=[12, 12], pooling_fn=lambda h, batch: h.max(0)[0])
    with pytest.raises(NotImplementedError, match="encode_nodes"):
        pooling_code(m.pooling_fn)
    assert callable(m.encode_nodes)
    # the table of the nodes level: None in the ffn slots, as for encode
    assert [i for i, p in enumerate(m.native_parameters(head=False)) if p is None] == [8, 9]


def test_level_tables_agree_between_python_layers():
    from cgr_mpnn_3D._amd import functional as fn

    assert (fn.LEVEL_FUSED, fn.LEVEL_POOLED, fn.LEVEL_NODES) == (0, 1, 2)
    assert fn._LEVEL_CALLS[fn.LEVEL_NODES] == ENTRY_POINTS  # forward, backward, inputs, predict
    assert fn._out_shape(fn.LEVEL_NODES, 7, 2, 5) == (7, 5)
    assert fn._out_shape(fn.LEVEL_POOLED, 7, 2, 5) == (2, 5)
    assert fn._out_shape(fn.LEVEL_FUSED, 7, 2, 5) == 2
    assert torch.empty(fn._out_shape(fn.LEVEL_FUSED, 7, 2, 5)).shape == (2,)
