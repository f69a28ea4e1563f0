"""CPU: the surface of the heteroscedastic-regression pieces -- MeanVarianceHead's parameters and
a model's state dict with it as ``ffn``, the GPU-only refusals, the argument checks of
GaussianNLLLoss (both call forms) and of the weighted losses, ``predict_ensemble``'s arithmetic on
stub models, and the new C entries' refusals (ctypes, nothing is launched: every refusal comes
before the first launch)."""

import ctypes
import io
import pickle

import numpy as np
import pytest
import torch

from cgr_mpnn_3D._amd import native
from cgr_mpnn_3D._amd.heads import MeanVarianceHead
from cgr_mpnn_3D._amd.infer import predict_ensemble
from cgr_mpnn_3D._amd.loss import GaussianNLLLoss, HuberLoss, L1Loss, MSELoss
from cgr_mpnn_3D.models import GNN as gnn_module
from cgr_mpnn_3D.models.GNN import GNN

H = 39


def _model(head=True):
    torch.manual_seed(5)
    m = GNN(7, 3, depth=2, hidden_sizes=[H] * 2, dropout_ps=[0.0] * 2)
    if head:
        m.ffn = MeanVarianceHead(H)
    return m


def test_head_parameters():
    h = MeanVarianceHead(H)
    assert {k: tuple(v.shape) for k, v in h.named_parameters()} == \
        {"mean.weight": (1, H), "mean.bias": (1,), "var.weight": (1, H), "var.bias": (1,)}
    assert list(h.state_dict()) == ["mean.weight", "mean.bias", "var.weight", "var.bias"]
    assert h.min_var == 1e-6 and MeanVarianceHead(H, min_var=0.0).min_var == 0.0
    assert "MeanVarianceHead" in gnn_module.__all__
    assert gnn_module.MeanVarianceHead is MeanVarianceHead


@pytest.mark.parametrize("bad", [-1e-6, float("nan"), float("inf")])
def test_head_refuses_bad_min_var(bad):
    with pytest.raises(ValueError, match="min_var"):
        MeanVarianceHead(H, min_var=bad)


def test_model_state_dict_round_trips():
    plain = _model(head=False)
    m = _model()
    keys = list(m.state_dict())
    want = {k for k in plain.state_dict() if not k.startswith("ffn.")} | \
        {"ffn.mean.weight", "ffn.mean.bias", "ffn.var.weight", "ffn.var.bias"}
    assert set(keys) == want
    other = _model()
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    other.load_state_dict(m.state_dict())
    for (k, a), (_, b) in zip(m.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k
    back = pickle.loads(pickle.dumps(m))
    assert isinstance(back.ffn, MeanVarianceHead) and back.ffn.min_var == m.ffn.min_var
    assert list(back.state_dict()) == keys
    for (k, a), (_, b) in zip(m.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a, b), k
    buf = io.BytesIO()
    torch.save(m.state_dict(), buf)
    buf.seek(0)
    other.load_state_dict(torch.load(buf))


def test_cpu_tensors_raise():
    with pytest.raises(RuntimeError, match="GPU only"):
        MeanVarianceHead(H)(torch.randn(4, H))

    class Data:
        pass

    d = Data()
    d.x, d.edge_index = torch.randn(6, 7), torch.zeros(2, 4, dtype=torch.int64)
    d.edge_attr, d.batch = torch.randn(4, 3), torch.tensor([0, 0, 0, 1, 1, 2])
    with pytest.raises(RuntimeError, match="GPU only"):
        _model()(d)
    out2, y, var, w = torch.rand(5, 2), torch.rand(5), torch.rand(5), torch.ones(5)
    with pytest.raises(RuntimeError, match="GPU only"):
        GaussianNLLLoss()(out2, y)
    with pytest.raises(RuntimeError, match="GPU only"):
        GaussianNLLLoss()(y, y, var)
    for loss in (MSELoss(), L1Loss(), HuberLoss()):
        with pytest.raises(RuntimeError, match="GPU only"):
            loss(y, y, weight=w)


def test_loss_constructor_refusals():
    for red in ("none", "batchmean", None):
        with pytest.raises(NotImplementedError, match="reduction"):
            GaussianNLLLoss(reduction=red)
    for eps in (0.0, -1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            GaussianNLLLoss(eps=eps)
    loss = GaussianNLLLoss(full=True, eps=1e-4, reduction="sum")
    assert (loss.full, loss.eps, loss.reduction) == (True, 1e-4, "sum")
    assert GaussianNLLLoss().reduction == "mean" and GaussianNLLLoss().eps == 1e-6
    assert GaussianNLLLoss.pads_by_weight is True
    assert not hasattr(MSELoss, "pads_by_weight")


def _fake_cuda(*shape, dtype=torch.float32):
    """A shape and dtype without storage that claims to be on the GPU: the shape checks under
    test come after the GPU-only check and before any kernel."""
    t = torch.empty(*shape, dtype=dtype, device="meta")

    class T:  # the attributes the checks read
        is_cuda = True
        device = torch.device("cuda:0")

        def __init__(self):
            self.shape, self.dtype = t.shape, t.dtype

        def dim(self):
            return len(self.shape)

        def numel(self):
            return t.numel()
    return T()


def test_loss_call_forms_check_shapes_and_dtypes():
    loss = GaussianNLLLoss()
    f = _fake_cuda
    # [n, 2] form
    for inp, tgt in ((f(5, 3), f(5)), (f(5), f(5)), (f(5, 2), f(4)), (f(5, 2), f(5, 1)),
                     (f(2, 5), f(5))):
        with pytest.raises(ValueError, match=r"\[n, 2\]"):
            loss(inp, tgt)
    with pytest.raises(TypeError, match="fp32"):
        loss(f(5, 2, dtype=torch.float64), f(5))
    with pytest.raises(ValueError, match="weight"):
        loss(f(5, 2), f(5), weight=f(4))
    with pytest.raises(ValueError, match="weight"):
        loss(f(5, 2), f(5), f(4))           # positionally: the third tensor is the weight
    with pytest.raises(TypeError, match="weight"):
        loss(f(5, 2), f(5), weight=f(5, dtype=torch.float64))
    # three-tensor form
    with pytest.raises(ValueError, match="same shape"):
        loss(f(5), f(4), f(5))
    with pytest.raises(ValueError, match="same shape"):
        loss(f(5), f(5), f(4))
    with pytest.raises(ValueError, match="same shape"):
        loss(f(5), f(5), f(5, 1))           # no broadcasting of a [n, 1] variance
    with pytest.raises(TypeError, match="fp32"):
        loss(f(5), f(5), f(5, dtype=torch.float16))
    with pytest.raises(ValueError, match="weight"):
        loss(f(5), f(5), f(5), f(6))
    # the weighted point losses
    for pl in (MSELoss(), L1Loss(), HuberLoss(delta=0.5)):
        with pytest.raises(ValueError, match="weight"):
            pl(f(5), f(5), weight=f(4))
        with pytest.raises(TypeError, match="weight"):
            pl(f(5), f(5), weight=f(5, dtype=torch.int64))
        with pytest.raises(ValueError, match="same shape"):
            pl(f(5), f(4), weight=f(5))


class _Stub:
    """What ``predict`` needs of a model and of a store."""

    def __init__(self, table):
        self.table, self.training, self.calls = table, True, 0

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode

    def __call__(self, ids):
        assert not self.training
        self.calls += 1
        return self.table[torch.as_tensor(ids)]


class _Store:
    num_graphs, device = 7, "cpu"

    @staticmethod
    def collate(ids):
        return ids


def test_predict_ensemble_arithmetic():
    g = torch.Generator().manual_seed(3)
    tables = [torch.rand(7, 2, generator=g, dtype=torch.float64) for _ in range(3)]
    models = [_Stub(t) for t in tables]
    mean, alea, epi = predict_ensemble(models, _Store(), batch_size=3)
    assert all(m.calls == 3 and m.training for m in models)          # 7 ids in batches of 3
    mus = np.stack([t[:, 0].numpy() for t in tables])
    np.testing.assert_allclose(mean.numpy(), mus.mean(0), rtol=1e-14)
    np.testing.assert_allclose(alea.numpy(), np.stack([t[:, 1].numpy() for t in tables]).mean(0),
                               rtol=1e-14)
    np.testing.assert_allclose(epi.numpy(), mus.var(0), rtol=1e-12)  # population variance
    assert mean.shape == alea.shape == epi.shape == (7,)
    # a subset, in the order asked for
    ids = [5, 0, 3]
    mean_s, alea_s, epi_s = predict_ensemble(models, _Store(), ids=ids)
    assert torch.equal(mean_s, mean[ids]) and torch.equal(alea_s, alea[ids])
    assert torch.equal(epi_s, epi[ids])
    # members with point outputs: no aleatoric part; one member: no spread
    mean_p, alea_p, epi_p = predict_ensemble([_Stub(t[:, 0]) for t in tables], _Store())
    assert alea_p is None and torch.equal(mean_p, mean) and torch.equal(epi_p, epi)
    one = predict_ensemble([_Stub(tables[0])], _Store())
    assert torch.equal(one[0], tables[0][:, 0]) and torch.equal(one[1], tables[0][:, 1])
    assert bool((one[2] == 0).all())
    with pytest.raises(ValueError, match="no models"):
        predict_ensemble([], _Store())
    with pytest.raises(ValueError, match="alike"):
        predict_ensemble([_Stub(tables[0]), _Stub(tables[1][:, 0])], _Store())


def _last_error(lib):
    return lib.cgr_last_error().decode()


def test_head_entries_refuse_bad_arguments_before_any_launch():
    """Host memory stands in for every buffer: a refusal never reads or launches anything."""
    lib = native.load()
    B, Hh = 3, 8
    fbuf = (ctypes.c_float * (B * Hh))()
    p = ctypes.addressof(fbuf)

    def forward(g=p, ldg=Hh, b=B, h=Hh, wm=p, wv=p, min_var=1e-6, out=p, raw=p):
        return lib.cgr_meanvar_head_forward(g, ldg, b, h, wm, None, wv, None, min_var, out, raw,
                                            None)

    def backward(g=p, ldg=Hh, b=B, h=Hh, wm=p, wv=p, raw=p, dout=p, dg=p, dW=p, db=p):
        return lib.cgr_meanvar_head_backward(g, ldg, b, h, wm, wv, raw, dout, dg, dW, db, None)

    for call, name in ((forward, "cgr_meanvar_head_forward"),
                       (backward, "cgr_meanvar_head_backward")):
        for kw, word in (({"h": 0}, "H"), ({"h": -4}, "H"), ({"ldg": Hh - 1}, "ldg"),
                         ({"g": None}, "NULL"), ({"wm": None}, "NULL"), ({"wv": None}, "NULL"),
                         ({"b": -1}, "range")):
            assert call(**kw) != 0, (name, kw)
            msg = _last_error(lib)
            assert name in msg and word in msg, (kw, msg)
    assert forward(out=None) != 0 and "NULL" in _last_error(lib)
    for bad in (-1e-9, float("nan"), float("inf"), 1e39):
        assert forward(min_var=bad) != 0 and "min_var" in _last_error(lib), bad
    assert backward(raw=None) != 0 and "NULL" in _last_error(lib)
    assert backward(dout=None) != 0 and "NULL" in _last_error(lib)
    # nothing wanted: accepted, and nothing is launched
    assert backward(dg=None, dW=None, db=None) == 0


def test_loss_entries_refuse_bad_arguments_before_any_launch():
    lib = native.load()
    n = 6
    fbuf = (ctypes.c_float * (2 * n))()
    p = ctypes.addressof(fbuf)

    def nll_fwd(mu=p, ms=1, var=p, vs=1, t=p, nn=n, eps=1e-6, loss=p):
        return lib.cgr_gaussian_nll_loss_forward(mu, ms, var, vs, t, None, nn, 0, 0, eps, loss,
                                                 None)

    def nll_bwd(mu=p, ms=1, var=p, vs=1, t=p, g=p, nn=n, eps=1e-6, gs=1):
        return lib.cgr_gaussian_nll_loss_backward(mu, ms, var, vs, t, None, g, nn, 0, eps, p, p,
                                                  gs, p, None)

    for call, name in ((nll_fwd, "cgr_gaussian_nll_loss_forward"),
                       (nll_bwd, "cgr_gaussian_nll_loss_backward")):
        for kw, word in (({"mu": None}, "NULL"), ({"var": None}, "NULL"), ({"t": None}, "NULL"),
                         ({"nn": -1}, "range"), ({"ms": 0}, "stride"), ({"vs": -2}, "stride"),
                         ({"eps": 0.0}, "eps"), ({"eps": float("nan")}, "eps"),
                         ({"eps": float("inf")}, "eps")):
            assert call(**kw) != 0, (name, kw)
            msg = _last_error(lib)
            assert name in msg and word in msg, (kw, msg)
    assert nll_fwd(loss=None) != 0 and "NULL" in _last_error(lib)
    assert nll_bwd(g=None) != 0 and "NULL" in _last_error(lib)
    assert nll_bwd(gs=0) != 0 and "stride" in _last_error(lib)

    def w_fwd(kind=0, x=p, t=p, w=p, nn=n, delta=1.0, loss=p):
        return lib.cgr_weighted_loss_forward(kind, x, t, w, nn, 0, delta, loss, None)

    def w_bwd(kind=0, x=p, t=p, w=p, g=p, nn=n, delta=1.0):
        return lib.cgr_weighted_loss_backward(kind, x, t, w, g, nn, 0, delta, p, p, None)

    for call, name in ((w_fwd, "cgr_weighted_loss_forward"),
                       (w_bwd, "cgr_weighted_loss_backward")):
        for kw, word in (({"kind": 3}, "kind"), ({"kind": -1}, "kind"), ({"x": None}, "NULL"),
                         ({"t": None}, "NULL"), ({"w": None}, "NULL"), ({"nn": -1}, "range"),
                         ({"kind": 2, "delta": 0.0}, "delta"),
                         ({"kind": 2, "delta": float("nan")}, "delta")):
            assert call(**kw) != 0, (name, kw)
            msg = _last_error(lib)
            assert name in msg and word in msg, (kw, msg)
    assert w_fwd(loss=None) != 0 and "NULL" in _last_error(lib)
    assert w_bwd(g=None) != 0 and "NULL" in _last_error(lib)
