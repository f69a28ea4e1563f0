"""CPU: the surface of the attention-pooling readout -- the module's parameters, the model's
state dict with it as ``pooling_fn``, the GPU-only refusals, and the C entries' argument checks
(ctypes, nothing is launched: every refusal comes before the first launch)."""

import ctypes
import io
import pickle

import pytest
import torch

from cgr_mpnn_3D._amd import native
from cgr_mpnn_3D._amd.pool import AttentionPool, attention_pool
from cgr_mpnn_3D.models import GNN as gnn_module
from cgr_mpnn_3D.models.GNN import GNN

H = 39


def _model(pool=None):
    torch.manual_seed(5)
    kw = {} if pool is None else {"pooling_fn": pool}
    return GNN(7, 3, depth=2, hidden_sizes=[H] * 2, dropout_ps=[0.0] * 2, **kw)


def test_module_parameters():
    p = AttentionPool(H)
    assert {k: tuple(v.shape) for k, v in p.named_parameters()} == \
        {"gate.weight": (1, H), "gate.bias": (1,)}
    assert "AttentionPool" in gnn_module.__all__ and gnn_module.AttentionPool is AttentionPool


def test_model_state_dict_gains_the_gate_and_round_trips():
    plain = _model()
    m = _model(AttentionPool(H))
    keys = list(m.state_dict())
    assert set(keys) == set(plain.state_dict()) | {"pooling_fn.gate.weight",
                                                   "pooling_fn.gate.bias"}
    assert list(_model().state_dict()) == list(plain.state_dict())  # the default: unchanged
    names = {k for k, _ in m.named_parameters()}
    assert {"pooling_fn.gate.weight", "pooling_fn.gate.bias"} <= names
    other = _model(AttentionPool(H))
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    other.load_state_dict(m.state_dict())
    for (k, a), (_, b) in zip(m.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k
    back = pickle.loads(pickle.dumps(m))
    assert isinstance(back.pooling_fn, AttentionPool)
    assert list(back.state_dict()) == keys
    for (k, a), (_, b) in zip(m.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a, b), k
    buf = io.BytesIO()
    torch.save(m.state_dict(), buf)
    buf.seek(0)
    other.load_state_dict(torch.load(buf))


def test_cpu_tensors_raise():
    x = torch.randn(6, H)
    batch = torch.tensor([0, 0, 0, 1, 1, 2])
    p = AttentionPool(H)
    with pytest.raises(RuntimeError, match="GPU only"):
        p(x, batch, size=3)
    with pytest.raises(RuntimeError, match="GPU only"):
        attention_pool(x, batch, p.gate.weight, p.gate.bias)

    class Data:
        pass

    d = Data()
    d.x, d.edge_index = torch.randn(6, 7), torch.zeros(2, 4, dtype=torch.int64)
    d.edge_attr, d.batch = torch.randn(4, 3), batch
    with pytest.raises(RuntimeError, match="GPU only"):
        _model(AttentionPool(H))(d)
    with pytest.raises(RuntimeError, match="GPU only"):
        _model(AttentionPool(H)).encode(d)


def test_workspace_bytes_grow_with_both_sizes():
    lib = native.load()
    f = lib.cgr_attention_pool_workspace_bytes
    assert 0 < f(1, 5) < f(1, 39) < f(1, 400) < f(256, 400) < f(512, 400)
    assert f(7, 100) >= 7 * 100 * 4
    assert f(3, 0) == -1 and f(-1, 8) == -1


def _last_error(lib):
    return lib.cgr_last_error().decode()


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """Host memory stands in for every buffer: a refusal never reads or launches anything."""
    lib = native.load()
    N, B, Hh = 6, 3, 8
    fbuf = (ctypes.c_float * (N * Hh))()
    ibuf = (ctypes.c_int64 * (N + 1))()
    p, q = ctypes.addressof(fbuf), ctypes.addressof(ibuf)
    fwd, bwd = lib.cgr_attention_pool_forward, lib.cgr_attention_pool_backward

    def forward(x=p, ldx=Hh, n=N, h=Hh, batch=q, ptr=None, b=B, w=p, g=p, alpha=p):
        return fwd(x, ldx, n, h, batch, ptr, b, w, None, None, g, alpha, None)

    def backward(x=p, ldx=Hh, n=N, h=Hh, batch=q, ptr=None, b=B, w=p, alpha=p, dg=p, dx=p,
                 dw=None, ws=None):
        return bwd(x, ldx, n, h, batch, ptr, b, w, alpha, dg, dx, dw, ws, None)

    for call, name in ((forward, "cgr_attention_pool_forward"),
                       (backward, "cgr_attention_pool_backward")):
        for kw, word in (({"h": 0}, "H"), ({"h": -4}, "H"), ({"ldx": Hh - 1}, "ldx"),
                         ({"batch": None}, "batch"), ({"x": None}, "NULL"),
                         ({"w": None}, "NULL"), ({"n": -1}, "range"), ({"b": -1}, "range"),
                         ({"alpha": None}, "NULL")):
            assert call(**kw) != 0, (name, kw)
            msg = _last_error(lib)
            assert name in msg and word in msg, (kw, msg)
    assert forward(g=None) != 0 and "NULL" in _last_error(lib)
    assert backward(dg=None) != 0 and "NULL" in _last_error(lib)
    # dw without its workspace, or with a misaligned one
    assert backward(dw=p) != 0 and "workspace" in _last_error(lib)
    assert backward(dw=p, ws=(p | 15) + 1 - 12) != 0 and "workspace" in _last_error(lib)
