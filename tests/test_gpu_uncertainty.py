"""GPU: heteroscedastic regression on the native path -- MeanVarianceHead
(cgr_meanvar_head_forward / _backward), GaussianNLLLoss (cgr_gaussian_nll_loss_*), the weighted
forms of MSE / L1 / Huber (cgr_weighted_loss_*), and CapturedTrainer with a loss that pads by
weight.

Reference: the torch composition of each piece (`compose_head`, torch.nn.functional's losses,
sum(w * term)) evaluated in float64 on the CPU from the same fp32 inputs.

Bar (per tensor, per case), the one of test_gpu_attention_pool.py: with e_native the largest
absolute error of the native result against float64 and e_torch that of the same composition run
in fp32 by torch on the GPU,
    e_native <= 4 e_torch + 2^-22 max|ref|.
Every case's figures go to uncertainty_errors.json in the test report directory.  The bar cases of
the Gaussian loss keep var >= 1e-3; variances below, at and above eps are checked against float64
at rtol 1e-5 (the tolerance of test_gpu_captured_epoch.py for fp32 elementwise results), since
1 / v^2 at v = 1e-6 leaves no absolute bar meaningful.

Shapes.  Head: H = 5 (fewer than one float4 pair, H % 4 != 0), 39 (H % 4 != 0), 100, 400 (lanes
0-35 of a wave take a second column group; seven backward workgroups); B = 1, 3, 17 (more rows
than the backward's 16 row phases), 70 (more rows than a wave has lanes); g with ldg > H in the
float4 form (ldg % 4 == 0) and in the element form.  Losses: n = 1, 5, 63, 64, 65 (around a
wave), 257 (a second block of the backward, a second round of the forward's loop), 1000."""

import copy
import ctypes
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from encode_common import ragged_batch
from test_gpu_parity import _write_report

from cgr_mpnn_3D._amd import native
from cgr_mpnn_3D._amd.captured import CapturedTrainer
from cgr_mpnn_3D._amd.data import GraphStore
from cgr_mpnn_3D._amd.heads import MeanVarianceHead
from cgr_mpnn_3D._amd.loss import GaussianNLLLoss, HuberLoss, L1Loss, MSELoss
from cgr_mpnn_3D._amd.optim import FusedAdam
from cgr_mpnn_3D._amd.pool import AttentionPool
from cgr_mpnn_3D._amd.synth import make_batch
from cgr_mpnn_3D.models.GNN import GNN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HS = (5, 39, 100, 400)
BS = (1, 3, 17, 70)
NS = (1, 5, 63, 64, 65, 257, 1000)
MIN_VAR = 1e-6
ROWS = []  # the report


def hold_bar(case, nat, t32, ref, names):
    bad = []
    for k in names:
        r = ref[k].detach()
        e_native = float((nat[k].detach().cpu().double().reshape(r.shape) - r).abs().max())
        e_torch = float((t32[k].detach().cpu().double().reshape(r.shape) - r).abs().max())
        scale = float(r.abs().max())
        bar = 4.0 * e_torch + 2.0 ** -22 * scale
        ROWS.append(dict(case=case, tensor=k, e_native=e_native, e_torch=e_torch, ref_max=scale,
                         bar=bar))
        print(f"{case} {k}: e_native {e_native:.3e} e_torch {e_torch:.3e} max|ref| {scale:.3e} "
              f"bar {bar:.3e}")
        if not e_native <= bar:
            bad.append((k, e_native, e_torch, bar))
    _write_report("uncertainty_errors.json", ROWS)
    assert not bad, (case, bad)


# ----------------------------------------------------------------------------------------------
# 1. the head
# ----------------------------------------------------------------------------------------------
def compose_head(g, wm, bm, wv, bv):
    """out [B, 2] and raw [B] with torch ops, any dtype / device."""
    mu = F.linear(g, wm, bm)
    raw = F.linear(g, wv, bv)
    return torch.cat([mu, F.softplus(raw) + MIN_VAR], 1), raw[:, 0]


def compose_head_run(t):
    g, wm, bm, wv, bv = (t[k].detach().clone().requires_grad_(True)
                         for k in ("g", "wm", "bm", "wv", "bv"))
    out, raw = compose_head(g, wm, bm, wv, bv)
    dg, dwm, dbm, dwv, dbv = torch.autograd.grad(out, (g, wm, bm, wv, bv), t["dout"])
    return dict(out=out.detach(), raw=raw.detach(), dg=dg, dW=torch.cat([dwm, dwv], 0),
                db=torch.cat([dbm, dbv], 0))


def head_module(t, dev=DEV):
    head = MeanVarianceHead(t["g"].shape[1], min_var=MIN_VAR).to(dev)
    with torch.no_grad():
        for p, k in ((head.mean.weight, "wm"), (head.mean.bias, "bm"), (head.var.weight, "wv"),
                     (head.var.bias, "bv")):
            p.copy_(t[k])
    return head


def native_head_run(t, g=None):
    """The module on DEV; `g`: the device tensor to feed (a strided view), default t["g"]."""
    head = head_module(t)
    g = (t["g"].to(DEV) if g is None else g).detach().requires_grad_(True)
    out = head(g)
    ps = (head.mean.weight, head.mean.bias, head.var.weight, head.var.bias)
    dg, dwm, dbm, dwv, dbv = torch.autograd.grad(out, (g,) + ps, t["dout"].to(DEV))
    torch.cuda.synchronize()
    assert dwm.shape == (1, g.shape[1]) and dwv.shape == dwm.shape
    assert dbm.shape == (1,) and dbv.shape == (1,)
    return dict(out=out.detach(), dg=dg, dW=torch.cat([dwm, dwv], 0), db=torch.cat([dbm, dbv], 0))


def head_inputs(H, B, seed=0):
    """fp32 CPU tensors.  raw = g.wv + bv has a standard deviation of ~25, so both softplus
    branches (raw > 20: the identity) and raw < -20 (var ~ min_var) occur."""
    rng = np.random.default_rng(100 * H + B + 7919 * seed)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))  # noqa: E731
    return dict(g=f(B, H), wm=f(1, H) / np.sqrt(H), bm=f(1), wv=f(1, H) * (25.0 / np.sqrt(H)),
                bv=f(1), dout=f(B, 2))


def to_double(t):
    return {k: v.double() for k, v in t.items()}


def to_dev(t):
    return {k: v.to(DEV) for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def head_case(H, B):
    t = head_inputs(H, B)
    return t, native_head_run(t), compose_head_run(to_dev(t)), compose_head_run(to_double(t))


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("H", HS)
def test_head_values_against_float64(H, B, cuda_device):
    t, nat, t32, ref = head_case(H, B)
    assert tuple(nat["out"].shape) == (B, 2) and tuple(nat["dg"].shape) == (B, H)
    if B >= 17:
        assert float(ref["raw"].max()) > 20 and float(ref["raw"].min()) < -20
    assert bool((nat["out"][:, 1] >= MIN_VAR).all())
    hold_bar(f"head_h{H}_b{B}", nat, t32, ref, ("out", "dg", "dW", "db"))


@pytest.mark.parametrize("H,ld", [(100, 104), (400, 404), (400, 401), (39, 45), (5, 8)])
def test_head_strided_rows(H, ld, cuda_device):
    """ldg > H: rows of a wider buffer, in the float4 form (ld % 4 == 0, H % 4 == 0) and the
    element form -- the same bits as from contiguous rows, and under the bar."""
    t, nat, t32, ref = head_case(H, 17)
    wide = torch.full((17, ld), float("nan"), device=DEV)
    wide[:, :H] = t["g"].to(DEV)
    view = wide[:, :H]
    assert view.stride() == (ld, 1)
    got = native_head_run(t, g=view)
    for k in ("out", "dg", "dW", "db"):
        assert torch.equal(got[k], nat[k]), k
    hold_bar(f"head_h{H}_ld{ld}", got, t32, ref, ("out", "dg", "dW", "db"))


@pytest.mark.parametrize("H", HS)
def test_head_rows_are_batch_independent_and_reproducible(H, cuda_device):
    B = 70
    t, nat, _, _ = head_case(H, B)
    again = native_head_run(t)
    for k in ("out", "dg", "dW", "db"):
        assert torch.equal(again[k], nat[k]), k
    g = t["g"].to(DEV)
    for b in (0, 1, 16, 17, 63, 64, 69):  # (rows at every alignment of an H % 4 != 0 stride)
        one = dict(t, g=t["g"][b:b + 1], dout=t["dout"][b:b + 1])
        alone = native_head_run(one, g=g[b:b + 1])
        assert torch.equal(alone["out"][0], nat["out"][b]), b
        assert torch.equal(alone["dg"][0], nat["dg"][b]), b
        sub = dict(t, g=t["g"][b:b + 3], dout=t["dout"][b:b + 3])
        few = native_head_run(sub, g=g[b:b + 3].clone())
        n = few["out"].shape[0]
        assert torch.equal(few["out"], nat["out"][b:b + n]), b
        assert torch.equal(few["dg"], nat["dg"][b:b + n]), b


def test_head_partial_gradients(cuda_device):
    """Only what requires grad is computed; each combination gives the full run's bits."""
    t, nat, _, _ = head_case(39, 17)
    head = head_module(t)
    g = t["g"].to(DEV)
    dout = t["dout"].to(DEV)
    gin = g.clone().requires_grad_(True)
    for p in head.parameters():
        p.requires_grad_(False)
    (dg,) = torch.autograd.grad(head(gin), (gin,), dout)
    assert torch.equal(dg, nat["dg"])
    head.var.weight.requires_grad_(True)
    (dwv,) = torch.autograd.grad(head(g), (head.var.weight,), dout)
    assert torch.equal(dwv, nat["dW"][1:2])
    head.mean.bias.requires_grad_(True)
    dbm, dwv = torch.autograd.grad(head(g), (head.mean.bias, head.var.weight), dout)
    assert torch.equal(dbm, nat["db"][0:1]) and torch.equal(dwv, nat["dW"][1:2])
    with torch.no_grad():
        assert torch.equal(head(g), nat["out"])


# ----------------------------------------------------------------------------------------------
# 2. the model with the head
# ----------------------------------------------------------------------------------------------
F_, FE, HM, DEPTH = 7, 3, 39, 2


def model_batch(seed=0):
    """encode_common.ragged_batch's graphs (B 5, N 73, one single-atom graph) with F = 7 node and
    Fe = 3 edge features."""
    b = ragged_batch()
    rng = np.random.default_rng(77 + seed)
    return replace(b, x=rng.standard_normal((b.x.shape[0], F_)).astype(np.float32),
                   edge_attr=rng.standard_normal((b.edge_index.shape[1], FE)).astype(np.float32),
                   y=rng.standard_normal(b.num_graphs).astype(np.float32))


def head_model(dev, pool=None):
    torch.manual_seed(11)
    kw = {} if pool is None else {"pooling_fn": pool}
    m = GNN(F_, FE, depth=DEPTH, hidden_sizes=[HM] * DEPTH, dropout_ps=[0.0] * DEPTH,
            activation_fn=F.silu, **kw)
    m.ffn = MeanVarianceHead(HM)
    return m.to(dev).train()


@pytest.mark.parametrize("attention", [False, True])
def test_model_equals_head_on_encode_and_trains_end_to_end(attention, cuda_device):
    m = head_model(cuda_device, AttentionPool(HM) if attention else None)
    data = model_batch().to_torch(cuda_device)
    data.x.requires_grad_(True)
    B = data.ptr.numel() - 1
    out = m(data)
    assert tuple(out.shape) == (B, 2) and out.requires_grad
    assert torch.equal(out.detach(), m.ffn(m.encode(data)).detach())
    with torch.no_grad():
        assert torch.equal(m(data), out.detach())
        g = m.encode(data)
    # the head against float64 on the model's own fingerprint
    ffn64 = copy.deepcopy(m.ffn).cpu().double()
    t = dict(g=g.cpu(), wm=ffn64.mean.weight, bm=ffn64.mean.bias, wv=ffn64.var.weight,
             bv=ffn64.var.bias)
    with torch.no_grad():
        ref = compose_head(*(t[k].double() for k in ("g", "wm", "bm", "wv", "bv")))[0]
        t32 = compose_head(*(t[k].float().to(cuda_device)
                             for k in ("g", "wm", "bm", "wv", "bv")))[0]
    hold_bar(f"model_attention{int(attention)}", dict(out=out), dict(out=t32), dict(out=ref),
             ("out",))
    # one backward through GNN + head + NLL: every gradient, full shapes
    loss = GaussianNLLLoss(reduction="sum")(out, data.y)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    names = {k for k, _ in m.named_parameters()}
    assert {"ffn.mean.weight", "ffn.mean.bias", "ffn.var.weight", "ffn.var.bias"} <= names
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        assert bool(torch.isfinite(p.grad).all()), k
        if k != "pooling_fn.gate.bias":
            assert float(p.grad.abs().max()) > 0, k
    assert data.x.grad is not None and data.x.grad.shape == data.x.shape
    assert bool(torch.isfinite(data.x.grad).all()) and float(data.x.grad.abs().max()) > 0


# ----------------------------------------------------------------------------------------------
# 3. the Gaussian negative log-likelihood
# ----------------------------------------------------------------------------------------------
def nll_inputs(n, seed=0, var_min=1e-3):
    rng = np.random.default_rng(31 * n + seed)
    f = lambda: torch.from_numpy(rng.standard_normal(n).astype(np.float32))  # noqa: E731
    var = torch.from_numpy((var_min + 10.0 ** rng.uniform(-3.0, 1.0, n)).astype(np.float32))
    w = torch.from_numpy(rng.uniform(0.25, 2.0, n).astype(np.float32))
    return dict(mu=f(), var=var, y=f(), w=w, gl=torch.tensor(float(rng.uniform(0.5, 2.0))))


def torch_nll_run(t, full, reduction, eps=1e-6, weight=False, n=None):
    """torch.nn.functional.gaussian_nll_loss on the tensors' device and dtype; weighted:
    sum(w * term) (/ n), the terms from reduction="none" (n: default the number of elements)."""
    mu, var, y = (t[k].detach().clone().requires_grad_(True) for k in ("mu", "var", "y"))
    if weight:
        terms = F.gaussian_nll_loss(mu, y, var, full=full, eps=eps, reduction="none")
        loss = (t["w"] * terms).sum()
        if reduction == "mean":
            loss = loss / (n or mu.numel())
    else:
        loss = F.gaussian_nll_loss(mu, y, var, full=full, eps=eps, reduction=reduction)
    dmu, dvar, dy = torch.autograd.grad(loss, (mu, var, y), t["gl"].to(loss.dtype))
    return dict(loss=loss.detach(), dmu=dmu, dvar=dvar, dy=dy)


def native_nll_run(t, full, reduction, form, eps=1e-6, weight=False):
    """form "three": loss(mu, y, var); form "pair": loss(out2 [n, 2], y)."""
    d = to_dev(t)
    loss_fn = GaussianNLLLoss(full=full, eps=eps, reduction=reduction)
    y = d["y"].clone().requires_grad_(True)
    w = d["w"] if weight else None
    if form == "three":
        mu, var = (d[k].clone().requires_grad_(True) for k in ("mu", "var"))
        loss = loss_fn(mu, y, var, weight=w)
        dmu, dvar, dy = torch.autograd.grad(loss, (mu, var, y), d["gl"])
    else:
        out2 = torch.stack([d["mu"], d["var"]], 1).requires_grad_(True)
        loss = loss_fn(out2, y, weight=w)
        dout, dy = torch.autograd.grad(loss, (out2, y), d["gl"])
        assert dout.shape == out2.shape and dout.is_contiguous()
        dmu, dvar = dout[:, 0], dout[:, 1]
    torch.cuda.synchronize()
    assert loss.shape == ()
    return dict(loss=loss.detach(), dmu=dmu, dvar=dvar, dy=dy)


@pytest.mark.parametrize("n", NS)
def test_gaussian_nll_against_float64(n, cuda_device):
    t = nll_inputs(n)
    for full in (False, True):
        for reduction in ("sum", "mean"):
            ref = torch_nll_run(to_double(t), full, reduction)
            t32 = torch_nll_run(to_dev(t), full, reduction)
            three = native_nll_run(t, full, reduction, "three")
            pair = native_nll_run(t, full, reduction, "pair")
            for k in ("loss", "dmu", "dvar", "dy"):
                assert torch.equal(three[k], pair[k]), (k, full, reduction)
            hold_bar(f"nll_n{n}_full{int(full)}_{reduction}", three, t32, ref,
                     ("loss", "dmu", "dvar", "dy"))
    again = native_nll_run(t, True, "mean", "pair")
    for k in ("loss", "dmu", "dvar", "dy"):
        assert torch.equal(again[k], pair[k]), k


def test_gaussian_nll_clamp_is_straight_through(cuda_device):
    """var below, at and above eps: the term and every gradient at v = max(var, eps), the
    gradient handed to var unchanged also below eps (torch 2.x); against float64 at rtol 1e-5."""
    eps = 1e-6
    var = torch.tensor([1e-9, 0.0, 5e-7, 1e-6, 1.0000001e-6, 2e-6, 1e-3, 0.5, 3.0] * 8,
                       dtype=torch.float32)
    n = var.numel()
    t = nll_inputs(n, seed=5)
    # mu - y from 0 to 1.5: at v = 1e-6 either part of dvar = (1 / v - d^2 / v^2) / 2 leads in
    # some element; |d| = 1e-3, where the two cancel and no relative tolerance holds, is kept out
    d = torch.tensor([0.0, 3e-4, 2e-3, 0.5, -1.5, 0.01, -3e-4, 0.1]).repeat(9)
    t = dict(t, var=var, y=t["mu"] + d)
    assert bool((var < eps).any()) and bool((var == eps).any()) and bool((var > eps).any())
    for reduction in ("sum", "mean"):
        ref = torch_nll_run(to_double(t), True, reduction, eps)
        for form in ("three", "pair"):
            got = native_nll_run(t, True, reduction, form, eps)
            assert float(ref["dvar"][var < eps].abs().min()) > 0     # not the clamp's zero
            for k in ("loss", "dmu", "dvar", "dy"):
                torch.testing.assert_close(got[k].cpu().double(), ref[k], rtol=1e-5, atol=0.0,
                                           msg=lambda m, k=k: f"{k} ({form}, {reduction}): {m}")


def test_gaussian_nll_strict_mode_refuses_negative_var(cuda_device, monkeypatch):
    from cgr_mpnn_3D._amd import config

    out2 = torch.tensor([[0.0, 1.0], [0.5, -1.0]], device=cuda_device)
    y = torch.zeros(2, device=cuda_device)
    w = torch.tensor([1.0, 0.0], device=cuda_device)
    loss = GaussianNLLLoss(reduction="sum")
    assert bool(torch.isfinite(loss(out2, y)))          # unchecked by default: the clamp applies
    monkeypatch.setattr(config, "strict", True)
    with pytest.raises(ValueError, match="negative"):
        loss(out2, y)
    with pytest.raises(ValueError, match="negative"):
        loss(out2[:, 0], y, out2[:, 1])
    assert bool(torch.isfinite(loss(out2, y, weight=w)))  # a weight-0 slot may hold anything


# ----------------------------------------------------------------------------------------------
# 4. weights, on all four losses
# ----------------------------------------------------------------------------------------------
POINT = {"mse": (MSELoss, {}, lambda a, b: F.mse_loss(a, b, reduction="none")),
         "l1": (L1Loss, {}, lambda a, b: F.l1_loss(a, b, reduction="none")),
         "huber": (HuberLoss, {"delta": 0.7},
                   lambda a, b: F.huber_loss(a, b, reduction="none", delta=0.7))}


def point_run(kind, t, reduction, native_form, n=None):
    """sum(w * term) (/ n) and its gradients: the native weighted loss, or torch's terms (n:
    default the number of elements)."""
    cls, kw, terms = POINT[kind]
    x, y = (t[k].detach().clone().requires_grad_(True) for k in ("mu", "y"))
    if native_form:
        loss = cls(reduction=reduction, **kw)(x, y, weight=t["w"])
    else:
        loss = (t["w"] * terms(x, y)).sum()
        if reduction == "mean":
            loss = loss / (n or x.numel())
    dx, dy = torch.autograd.grad(loss, (x, y), t["gl"].to(loss.dtype))
    return dict(loss=loss.detach(), dx=dx, dy=dy)


def weighted_inputs(n, seed=0):
    t = nll_inputs(n, seed)
    w = t["w"].clone()
    w[::3] = 0.0           # n = 1: the only element
    return dict(t, w=w)


@pytest.mark.parametrize("n", NS)
def test_weighted_values_against_float64(n, cuda_device):
    t = weighted_inputs(n, seed=1)
    for reduction in ("sum", "mean"):
        for kind in POINT:
            ref = point_run(kind, to_double(t), reduction, False)
            t32 = point_run(kind, to_dev(t), reduction, False)
            nat = point_run(kind, to_dev(t), reduction, True)
            torch.cuda.synchronize()
            hold_bar(f"w{kind}_n{n}_{reduction}", nat, t32, ref, ("loss", "dx", "dy"))
        ref = torch_nll_run(to_double(t), True, reduction, weight=True)
        t32 = torch_nll_run(to_dev(t), True, reduction, weight=True)
        three = native_nll_run(t, True, reduction, "three", weight=True)
        pair = native_nll_run(t, True, reduction, "pair", weight=True)
        for k in ("loss", "dmu", "dvar", "dy"):
            assert torch.equal(three[k], pair[k]), (k, reduction)
        hold_bar(f"wnll_n{n}_{reduction}", pair, t32, ref, ("loss", "dmu", "dvar", "dy"))


@pytest.mark.parametrize("n", (5, 65, 257))
def test_weight_zero_elements_are_skipped(n, cuda_device):
    """NaN, inf and var = -1 at w = 0: the loss is the loss over the remaining elements (under
    the bar, against float64) and those elements' gradients are exact zeros."""
    t = weighted_inputs(n, seed=2)
    off = t["w"] == 0
    keep = ~off
    assert bool(off.any()) and bool(keep.any())
    rest = {k: (v[keep] if v.dim() else v) for k, v in t.items()}
    poison = torch.tensor([float("nan"), float("inf"), -float("inf")]).repeat(n)[:n]
    bad = dict(t, mu=torch.where(off, poison, t["mu"]),
               y=torch.where(off, poison.flip(0), t["y"]),
               var=torch.where(off, torch.tensor(-1.0), t["var"]))
    bad["var"][0] = float("nan")    # (index 0 has weight 0)
    for reduction in ("sum", "mean"):
        for kind in POINT:
            ref = point_run(kind, to_double(rest), reduction, False, n)  # "mean" divides by n
            t32 = point_run(kind, to_dev(rest), reduction, False, n)
            nat = point_run(kind, to_dev(bad), reduction, True)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(nat["loss"]))
            for k in ("dx", "dy"):
                assert bool((nat[k][off] == 0).all()), (kind, k)
            hold_bar(f"w0{kind}_n{n}_{reduction}",
                     dict(loss=nat["loss"], dx=nat["dx"][keep], dy=nat["dy"][keep]),
                     t32, ref, ("loss", "dx", "dy"))
        ref = torch_nll_run(to_double(rest), False, reduction, weight=True, n=n)
        t32 = torch_nll_run(to_dev(rest), False, reduction, weight=True, n=n)
        for form in ("three", "pair"):
            nat = native_nll_run(bad, False, reduction, form, weight=True)
            assert bool(torch.isfinite(nat["loss"]))
            for k in ("dmu", "dvar", "dy"):
                assert bool((nat[k][off] == 0).all()), (form, k)
            hold_bar(f"w0nll_{form}_n{n}_{reduction}",
                     dict(loss=nat["loss"], **{k: nat[k][keep] for k in ("dmu", "dvar", "dy")}),
                     t32, ref, ("loss", "dmu", "dvar", "dy"))


@pytest.mark.parametrize("n", (5, 257))
def test_unweighted_point_losses_run_the_existing_entries(n, cuda_device):
    """weight=None: the bits of a direct call of cgr_mse / l1 / huber_loss_forward / _backward."""
    lib = native.load()
    t = to_dev(nll_inputs(n, seed=3))
    st = native.stream_ptr(cuda_device)
    for kind, (cls, kw, _) in POINT.items():
        extra = (ctypes.c_double(kw["delta"]),) if kw else ()
        for mean in (0, 1):
            x, y = (t[k].clone().requires_grad_(True) for k in ("mu", "y"))
            loss = cls(reduction="mean" if mean else "sum", **kw)(x, y, weight=None)
            dx, dy = torch.autograd.grad(loss, (x, y), t["gl"])
            l0, dx0, dy0 = torch.empty((), device=cuda_device), torch.empty_like(x), \
                torch.empty_like(y)
            native.check(getattr(lib, f"cgr_{kind}_loss_forward")(
                x.data_ptr(), y.data_ptr(), n, mean, *extra, l0.data_ptr(), st))
            native.check(getattr(lib, f"cgr_{kind}_loss_backward")(
                x.data_ptr(), y.data_ptr(), t["gl"].data_ptr(), n, mean, *extra, dx0.data_ptr(),
                dy0.data_ptr(), st))
            torch.cuda.synchronize()
            assert torch.equal(loss.detach(), l0), (kind, mean)
            assert torch.equal(dx, dx0) and torch.equal(dy, dy0), (kind, mean)


# ----------------------------------------------------------------------------------------------
# 5. captured training
# ----------------------------------------------------------------------------------------------
CD, CH = 2, 48


def captured_model(F_in, dev, head):
    torch.manual_seed(0)
    m = GNN(F_in, 14, depth=CD, hidden_sizes=[CH] * CD, dropout_ps=[0.0] * CD,
            activation_fn=F.silu)
    if head:
        m.ffn = MeanVarianceHead(CH)
    return m.to(dev).train()


@pytest.fixture(scope="module")
def epoch(cuda_device):
    """test_gpu_captured_epoch.py's epoch: B = 8, ragged batches, a short last batch."""
    b = make_batch(44, n_atoms=10, n_bonds=12, n_mace=3, seed=22, n_atoms_jitter=3)
    store = GraphStore.from_batch(b, cuda_device)
    order = np.argsort(-np.diff(b.ptr), kind="stable")
    rest = np.random.default_rng(3).permutation(order[8:])
    batches = [rest[0:8], rest[8:16], order[:8], rest[16:24], rest[24:32], rest[32:36]]
    batches = [np.asarray(x, np.int64) for x in batches]
    sizes = [store.batch_sizes(_full(ids, 8)[0]) for ids in batches]
    caps = (max(n for n, _ in sizes) + 40, max(e for _, e in sizes) + 8)
    assert len(set(sizes)) == len(sizes)   # ragged: every batch has its own N, E
    return b, store, batches, caps


def _full(ids, B):
    n = len(ids)
    w = np.zeros(B, np.float32)
    w[:n] = 1.0
    return (np.resize(ids, B) if n < B else ids), w


def _eager_epoch(m, opt, loss_fn, store, batches, B, caps, by_weight):
    losses = []
    total = torch.zeros((), device=store.device)
    for ids in batches:
        opt.zero_grad(set_to_none=True)
        full, w = _full(ids, B)
        pb = store.collate_padded(full, *caps, weight_dev=torch.from_numpy(w).to(store.device))
        if by_weight:
            loss = loss_fn(m(pb), pb.y, weight=pb.mask)
        else:
            loss = loss_fn(m(pb) * pb.mask, pb.y * pb.mask)
        loss.backward()
        opt.step()
        total += loss.detach()
        losses.append(loss.detach().clone())
    return losses, total


def _assert_same_training_state(m1, o1, m2, o2):
    for (k, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), k
        for s in ("step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert torch.equal(o1.state[p][s], o2.state[q][s]), (k, s)


def test_captured_epoch_with_the_head_equals_eager_padded_epoch(epoch, cuda_device):
    b, store, batches, caps = epoch
    B = 8
    loss_fn = GaussianNLLLoss(reduction="sum")

    m1 = captured_model(b.x.shape[1], cuda_device, head=True)
    o1 = FusedAdam(m1.parameters(), lr=1e-3, amsgrad=True)
    ref_losses, ref_total = _eager_epoch(m1, o1, loss_fn, store, batches, B, caps, True)

    m2 = captured_model(b.x.shape[1], cuda_device, head=True)
    o2 = FusedAdam(m2.parameters(), lr=1e-3, amsgrad=True)
    tr = CapturedTrainer(m2, o2, loss_fn, store, B, *caps)
    losses = [tr.step(ids).clone() for ids in batches]
    assert tr.fallbacks == 0
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(losses, ref_losses)):
        assert bool(torch.isfinite(x)) and torch.equal(x, y), (i, float(x), float(y))
    _assert_same_training_state(m1, o1, m2, o2)
    assert tr.epoch_loss() == float(ref_total)

    for ids in (batches[0], batches[5], batches[2]):   # full, short (4 ids), full
        got = tr.predict(ids).clone()
        assert got.shape == (len(ids), 2) and m2.training
        m2.eval()
        with torch.no_grad():
            ref = m2(store.collate(ids))
        m2.train()
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)
    assert tr.fallbacks == 0
    tr.close()


def test_captured_step_with_mse_is_unchanged(epoch, cuda_device):
    """A loss that does not pad by weight keeps the pred * mask form, and predict its [n]."""
    b, store, batches, caps = epoch
    B = 8
    loss_fn = MSELoss("sum")
    steps = batches[4:6]                               # a full batch and the short one
    m1 = captured_model(b.x.shape[1], cuda_device, head=False)
    o1 = FusedAdam(m1.parameters(), lr=1e-3, amsgrad=True)
    ref_losses, _ = _eager_epoch(m1, o1, loss_fn, store, steps, B, caps, False)
    m2 = captured_model(b.x.shape[1], cuda_device, head=False)
    o2 = FusedAdam(m2.parameters(), lr=1e-3, amsgrad=True)
    tr = CapturedTrainer(m2, o2, loss_fn, store, B, *caps)
    losses = [tr.step(ids).clone() for ids in steps]
    assert tr.fallbacks == 0
    torch.cuda.synchronize()
    for x, y in zip(losses, ref_losses):
        assert torch.equal(x, y)
    _assert_same_training_state(m1, o1, m2, o2)
    assert tr.predict(batches[5]).shape == (4,)
    tr.close()
