"""CPU: the surface of GNN.encode / the routed GNN.forward, and the pin of the encode tests'
float64 reference (tests/encode_common.py) against central finite differences."""

import io
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from encode_common import encode_backward, encode_forward, general_dg, ragged_batch
from stagewise_common import random_params

from cgr_mpnn_3D._amd import native
from cgr_mpnn_3D.models.GNN import GNN, global_max_pool

# Central differences of L = sum(dg * g) in float64 with step h * max(1, |p|): truncation error
# ~ h^2 |L'''| / 6 and rounding error ~ 2^-52 |L| / h.  With h = 1e-5 and |L| / max|grad| up to
# ~1e3 here both stay below 1e-7 of a tensor's largest gradient entry; the bar leaves a decade.
FD_STEP = 1e-5
FD_BAR = 1e-6
FD_SAMPLES = 12  # entries checked per tensor: the largest-gradient one and random ones


@pytest.mark.parametrize("pool", ["add", "mean", "max"])
@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_encode_reference_matches_finite_differences(pool, aggr):
    """5 ragged graphs (one a single atom), H 13, D 2, SiLU, learnable skip: every encoder
    gradient, dx and dedge_attr of the per-graph decomposition against central differences of
    cache["g"] contracted with a general dg."""
    H, D = 13, 2
    b = ragged_batch(seed=3, atoms=(6, 1, 9, 4, 7))
    F_, Fe = b.x.shape[1], b.edge_attr.shape[1]
    rng = np.random.default_rng(5)
    sd = {k: np.asarray(v, np.float64) for k, v in random_params(rng, F_, Fe, H, D).items()}
    dg = general_dg(b.num_graphs, H).astype(np.float64)

    def loss(p, x, ea):
        bb = type(b)(x=x, edge_index=b.edge_index, edge_attr=ea, batch=b.batch, ptr=b.ptr, y=b.y)
        g, _ = encode_forward(p, bb, D, "silu", True, aggr, pool)
        return float((dg * g).sum())

    x0, ea0 = b.x.astype(np.float64), b.edge_attr.astype(np.float64)
    bb = type(b)(x=x0, edge_index=b.edge_index, edge_attr=ea0, batch=b.batch, ptr=b.ptr, y=b.y)
    _, cache = encode_forward(sd, bb, D, "silu", True, aggr, pool)
    grads, gin, skip_abs = encode_backward(sd, cache, dg)
    assert set(skip_abs) == {f"skip_weights.{l}" for l in range(D)}
    assert not any(k.startswith("ffn.") for k in grads)
    tensors = {k: (sd[k], grads[k]) for k in grads}
    tensors["input:x"] = (x0, gin["x"])
    tensors["input:edge_attr"] = (ea0, gin["edge_attr"])
    worst = 0.0
    for name, (val, grad) in tensors.items():
        grad = np.asarray(grad, np.float64).reshape(np.shape(val))
        flat = np.asarray(val, np.float64).reshape(-1)
        picks = {int(np.argmax(np.abs(grad)))} | set(
            rng.integers(0, flat.size, min(FD_SAMPLES, flat.size)).tolist())
        for i in picks:
            h = FD_STEP * max(1.0, abs(flat[i]))
            vals = []
            for s in (+h, -h):
                pert = flat.copy()
                pert[i] += s
                pert = pert.reshape(np.shape(val))
                if name == "input:x":
                    vals.append(loss(sd, pert, ea0))
                elif name == "input:edge_attr":
                    vals.append(loss(sd, x0, pert))
                else:
                    vals.append(loss(dict(sd, **{name: pert}), x0, ea0))
            fd = (vals[0] - vals[1]) / (2 * h)
            err = abs(fd - grad.reshape(-1)[i]) / (np.abs(grad).max() + 1e-300)
            worst = max(worst, err)
            assert err <= FD_BAR, f"{name}[{i}]: fd {fd:.9e} vs {grad.reshape(-1)[i]:.9e}"
    print(f"pool={pool} aggr={aggr}: worst relative mismatch {worst:.2e}")


def _model(**kw):
    torch.manual_seed(11)
    return GNN(9, 4, depth=2, hidden_sizes=[12, 12], **kw)


def test_the_four_entry_points_are_bound():
    lib = native.load()
    for name in ("cgr_gnn_encode", "cgr_gnn_encode_backward", "cgr_gnn_encode_input_grads",
                 "cgr_gnn_encode_predict"):
        assert hasattr(lib, name) and name in {s[0] for s in native.SIGNATURES}
    assert lib.cgr_abi_version() == 9


def test_encode_and_custom_heads_refuse_cpu_tensors():
    b = ragged_batch(seed=3, atoms=(6, 1, 9, 4, 7))
    m = GNN(b.x.shape[1], 14, depth=2, hidden_sizes=[12, 12])
    with pytest.raises(RuntimeError, match="GPU only"):
        m.encode(b.to_torch())
    m.ffn = nn.Linear(12, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(b.to_torch())


def test_head_routing_predicate():
    m = _model()
    assert m._fused_head()
    for head in (nn.Linear(12, 3), nn.Linear(12, 1, bias=False), nn.Linear(11, 1),
                 nn.Sequential(nn.Linear(12, 16), nn.SiLU(), nn.Linear(16, 1))):
        m.ffn = head
        assert not m._fused_head()

    class MyLinear(nn.Linear):
        pass

    m.ffn = MyLinear(12, 1)
    assert not m._fused_head()  # type(...) is nn.Linear, not isinstance
    m.ffn = nn.Linear(12, 1)
    m.ffn.register_forward_hook(lambda *a: None)
    assert m._fused_head()  # hooks do not change the routing


def test_state_dict_keys_and_seeded_init_unchanged():
    m = _model(use_learnable_skip=True)
    keys = ["edge_init.weight", "edge_init.bias", "convs.0.lin.weight", "convs.0.lin.bias",
            "convs.1.lin.weight", "convs.1.lin.bias", "edge_to_node.weight", "edge_to_node.bias",
            "ffn.weight", "ffn.bias", "skip_weights.0", "skip_weights.1"]
    assert list(m.state_dict().keys()) == keys
    # the reference's construction order under the same seed (GNN.py:53-74)
    torch.manual_seed(11)
    ref = [nn.Linear(13, 12), nn.Linear(12, 12), nn.Linear(12, 12), nn.Linear(9 + 12, 12),
           nn.Linear(12, 1)]
    got = [m.edge_init, m.convs[0].lin, m.convs[1].lin, m.edge_to_node, m.ffn]
    for a, r in zip(got, ref):
        assert torch.equal(a.weight, r.weight) and torch.equal(a.bias, r.bias)
    # the table: the fused order, and None in the ffn slots for encode
    full, enc = m.native_parameters(), m.native_parameters(head=False)
    assert len(full) == len(enc) == 12
    assert [i for i, p in enumerate(enc) if p is None] == [8, 9]
    assert all(a is c for a, c in zip(full, enc) if c is not None)


def test_pickled_module_round_trips_with_encode():
    m = _model(activation_fn=F.silu, pooling_fn=global_max_pool)
    m.ffn = nn.Linear(12, 3)
    buf = io.BytesIO()
    pickle.dump(m, buf)
    m2 = pickle.loads(buf.getvalue())
    assert callable(m2.encode) and not m2._fused_head()
    for (k, a), (k2, c) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2 and torch.equal(a, c)
    assert len(m2.native_parameters(head=False)) == 10
