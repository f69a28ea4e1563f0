"""GPU: the attention-pooling readout (cgr_attention_pool_forward / _backward, _amd/pool.py
attention_pool / AttentionPool, GNN(pooling_fn=AttentionPool(H))).

Reference: the torch composition INTEGRATION.md §5 gives for this readout (`compose` below),
evaluated in float64 on the CPU from the same fp32 inputs, its division guarded so that a graph
without atoms gives 0.  One detail differs from the text there: the scores are shifted by their
graph's maximum, not by the batch's.  Any per-graph constant leaves the softmax unchanged, so it
is the same function; but the batch-wide shift underflows a whole graph to 0 / 0 once two graphs'
score ranges are ~745 apart in float64 (~103 in fp32), and the |s| ~ 1e4 case below needs a
reference that is defined there.

Bar (per tensor, per case): with e_native the largest absolute error of the native result against
float64 and e_torch that of `compose` run in fp32 by torch on the GPU,
    e_native <= 4 e_torch + 2^-22 max|ref|
(both are fp32 sums of the same terms in different orders; the floor covers tensors on which torch
happens to be exact).  Every case's figures go to attention_pool_errors.json in the test report
directory.

Shapes: H = 5 (fewer than one float4 pair, H % 4 != 0), 39 (H % 4 != 0), 100, 400 (cfg2's width;
lanes 0-35 of a wave take a second column group); graphs of [1, 3, 0, 17, 70, 2] atoms: a single
atom, an empty graph in the middle, more atoms than a wave has lanes and than the 16-atom load
batch; one 1,500-atom graph (past the backward's 1,024-atom LDS chunk)."""

import copy
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

from encode_common import ragged_batch
from test_gpu_parity import _write_report

from cgr_mpnn_3D._amd.loss import MSELoss
from cgr_mpnn_3D._amd.optim import FusedAdam
from cgr_mpnn_3D._amd.pool import AttentionPool, attention_pool, global_mean_pool
from cgr_mpnn_3D.models.GNN import GNN

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 0, 17, 70, 2)
HS = (5, 39, 100, 400)
DEV = "cuda:0"
ROWS = []  # the report


def compose(x, batch, B, w, b, mask=None):
    """(g [B, H], alpha [N]) with torch ops, any dtype / device (see the module docstring)."""
    s = x @ w + b
    on = torch.ones_like(s, dtype=torch.bool) if mask is None else mask
    neg = torch.full((B,), -torch.inf, dtype=x.dtype, device=x.device)
    m = neg.scatter_reduce(0, batch, s.detach().masked_fill(~on, -torch.inf), "amax")
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.where(on, torch.exp(torch.where(on, s - m[batch], torch.zeros_like(s))),
                    torch.zeros_like(s))
    z = torch.zeros(B, dtype=x.dtype, device=x.device).index_add_(0, batch, e)
    alpha = e / torch.where(z > 0, z, torch.ones_like(z))[batch]
    g = torch.zeros(B, x.shape[1], dtype=x.dtype, device=x.device).index_add_(
        0, batch, alpha[:, None] * x)
    return g, alpha


def compose_run(x, batch, B, w, b, dg, mask=None):
    """compose and its gradients from dg on the tensors' own device and dtype."""
    x, w, b = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    g, alpha = compose(x, batch, B, w, b, mask)
    dx, dw, db = torch.autograd.grad(g, (x, w, b), dg)
    return dict(g=g.detach(), alpha=alpha.detach(), dx=dx, dw=dw, db=db)


def native_run(x, batch, w, b, B, dg, ptr=None, mask=None):
    x, w, b = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    g, alpha = attention_pool(x, batch, w, b, B, ptr=ptr, mask=mask)
    assert not alpha.requires_grad and g.requires_grad
    dx, dw, db = torch.autograd.grad(g, (x, w, b), dg)
    torch.cuda.synchronize()
    return dict(g=g.detach(), alpha=alpha, dx=dx, dw=dw, db=db)


def inputs(H, sizes=SIZES, seed=0, scale=1.0):
    """fp32 CPU tensors of a ragged batch: x, batch, ptr, w [H], b [1], dg [B, H]."""
    rng = np.random.default_rng(1000 * H + seed)
    N, B = int(sum(sizes)), len(sizes)
    x = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal(H) / np.sqrt(H)).astype(np.float32)) * scale
    b = torch.tensor([0.3], dtype=torch.float32)
    dg = torch.from_numpy(rng.standard_normal((B, H)).astype(np.float32))
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    return dict(x=x, batch=batch, ptr=ptr, w=w, b=b, dg=dg, B=B, N=N, sizes=tuple(sizes))


def three_way(inp, mask=None):
    """(native, torch fp32 on the GPU, float64 on the CPU) of one input set."""
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inp.items()}
    mk = None if mask is None else mask.to(DEV)
    nat = native_run(d["x"], d["batch"], d["w"], d["b"], d["B"], d["dg"], ptr=d["ptr"], mask=mk)
    t32 = compose_run(d["x"], d["batch"], d["B"], d["w"], d["b"], d["dg"], mk)
    ref = compose_run(inp["x"].double(), inp["batch"], inp["B"], inp["w"].double(),
                      inp["b"].double(), inp["dg"].double(), mask)
    return nat, t32, ref


def hold_bar(case, nat, t32, ref, names=("g", "alpha", "dx", "dw")):
    bad = []
    for k in names:
        r = ref[k]
        e_native = float((nat[k].detach().cpu().double().reshape(r.shape) - r).abs().max()) \
            if r.numel() else 0.0
        e_torch = float((t32[k].detach().cpu().double().reshape(r.shape) - r).abs().max()) \
            if r.numel() else 0.0
        scale = float(r.abs().max()) if r.numel() else 0.0
        bar = 4.0 * e_torch + 2.0 ** -22 * scale
        ROWS.append(dict(case=case, tensor=k, e_native=e_native, e_torch=e_torch, ref_max=scale,
                         bar=bar))
        print(f"{case} {k}: e_native {e_native:.3e} e_torch {e_torch:.3e} max|ref| {scale:.3e} "
              f"bar {bar:.3e}")
        if not e_native <= bar:
            bad.append((k, e_native, e_torch, bar))
    _write_report("attention_pool_errors.json", ROWS)
    assert not bad, (case, bad)


def all_finite(run):
    return all(bool(torch.isfinite(t).all()) for t in run.values())


@functools.lru_cache(maxsize=None)
def ragged(H):
    inp = inputs(H)
    return (inp,) + three_way(inp)


# ----------------------------------------------------------------------------------------------
# 1. values
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", HS)
def test_values_against_float64(H, cuda_device):
    inp, nat, t32, ref = ragged(H)
    assert tuple(nat["g"].shape) == (inp["B"], H) and tuple(nat["alpha"].shape) == (inp["N"],)
    assert tuple(nat["dx"].shape) == (inp["N"], H) and tuple(nat["dw"].shape) == (H,)
    hold_bar(f"ragged_h{H}", nat, t32, ref)
    # the softmax is shift-invariant: the bias gradient is exact zeros
    assert tuple(nat["db"].shape) == (1,) and bool((nat["db"] == 0).all())
    assert float(ref["db"].abs().max()) < 1e-12


def test_gate_weight_shapes(cuda_device):
    """weight [1, H] (the module's nn.Linear) and [H] are the same call; dw keeps the shape."""
    inp, nat, _, _ = ragged(39)
    pool = AttentionPool(39).to(DEV)
    with torch.no_grad():
        pool.gate.weight.copy_(inp["w"][None])
        pool.gate.bias.copy_(inp["b"])
    x = inp["x"].to(DEV).requires_grad_(True)
    g, alpha = pool(x, inp["batch"].to(DEV), ptr=inp["ptr"].to(DEV), return_weights=True)
    (g * inp["dg"].to(DEV)).sum().backward()
    assert torch.equal(g.detach(), nat["g"]) and torch.equal(alpha, nat["alpha"])
    assert torch.equal(x.grad, nat["dx"])
    assert tuple(pool.gate.weight.grad.shape) == (1, 39)
    assert torch.equal(pool.gate.weight.grad[0], nat["dw"])
    assert bool((pool.gate.bias.grad == 0).all())
    g2 = pool(x, inp["batch"].to(DEV), size=inp["B"])
    assert torch.is_tensor(g2) and torch.equal(g2.detach(), nat["g"])


# ----------------------------------------------------------------------------------------------
# 2. exact properties
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", HS)
def test_exact_properties(H, cuda_device):
    inp, nat, _, _ = ragged(H)
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inp.items()}
    ptr = inp["ptr"].tolist()
    # twice: the same bits
    again = native_run(d["x"], d["batch"], d["w"], d["b"], d["B"], d["dg"], ptr=d["ptr"])
    for k in nat:
        assert torch.equal(nat[k], again[k]), k
    # the segment from ptr and from the binary searches in batch: the same bits; so is the
    # one-sync form that reads B from batch.max() (the last graph is not empty)
    for B in (d["B"], None):
        by_batch = native_run(d["x"], d["batch"], d["w"], d["b"], B, d["dg"])
        for k in nat:
            assert torch.equal(nat[k], by_batch[k]), (k, B)
    # nothing non-finite anywhere; the empty graph's row is +0.0
    assert all_finite(nat)
    for b, n in enumerate(inp["sizes"]):
        row = nat["g"][b]
        if n == 0:
            assert bool((row == 0).all()) and not bool(torch.signbit(row).any())
        else:
            a = nat["alpha"][ptr[b]:ptr[b + 1]].double()
            assert abs(float(a.sum()) - 1.0) <= n * 2.0 ** -23, (b, n)
        if n == 1:  # alpha exactly 1, the g row is the x row
            assert float(nat["alpha"][ptr[b]]) == 1.0
            assert torch.equal(row, d["x"][ptr[b]])
    # every graph pooled alone (batch=None on its own rows) == inside the batch, bit for bit
    for b, n in enumerate(inp["sizes"]):
        v0, v1 = ptr[b], ptr[b + 1]
        alone = native_run(d["x"][v0:v1], None, d["w"], d["b"], None, d["dg"][b:b + 1])
        assert torch.equal(alone["g"][0], nat["g"][b]), b
        assert torch.equal(alone["alpha"], nat["alpha"][v0:v1]), b
        assert torch.equal(alone["dx"], nat["dx"][v0:v1]), b


@pytest.mark.parametrize("H", (39, 400))
def test_scores_of_1e4_stay_finite(H, cuda_device):
    inp = inputs(H, seed=1)
    s = inp["x"].double() @ inp["w"].double()
    inp["w"] = (inp["w"].double() * (1e4 / float(s.abs().max()))).float()
    assert 0.99e4 < float((inp["x"].double() @ inp["w"].double()).abs().max()) < 1.01e4
    nat, t32, ref = three_way(inp)
    assert all_finite(nat)
    # float64's weights are one-hot to fp32 resolution in every graph of two or more atoms
    ptr = inp["ptr"].tolist()
    for b, n in enumerate(inp["sizes"]):
        if n:
            assert float(ref["alpha"][ptr[b]:ptr[b + 1]].max()) > 1.0 - 1e-6, b
    # (dw is left out here: with one-hot weights it is a sum of terms below 1e-28, nothing but
    # the fp32 rounding of scores of 1e4 in either fp32 implementation)
    hold_bar(f"scores_1e4_h{H}", nat, t32, ref, names=("g", "alpha", "dx"))


def test_one_long_graph(cuda_device):
    """1,500 atoms in one graph, H = 8: batch=None and an all-zero batch, the same bits."""
    inp = inputs(8, sizes=(1500,), seed=2)
    nat, t32, ref = three_way(inp)
    hold_bar("long_h8", nat, t32, ref)
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inp.items()}
    none = native_run(d["x"], None, d["w"], d["b"], None, d["dg"])
    zeros = native_run(d["x"], torch.zeros_like(d["batch"]), d["w"], d["b"], 1, d["dg"])
    for k in nat:
        assert torch.equal(nat[k], none[k]) and torch.equal(nat[k], zeros[k]), k
    assert abs(float(nat["alpha"].double().sum()) - 1.0) <= 1500 * 2.0 ** -23


# ----------------------------------------------------------------------------------------------
# 3. mask
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", (39, 100))
def test_mask(H, cuda_device):
    inp = inputs(H, seed=3)
    rng = np.random.default_rng(H)
    mask = torch.from_numpy(rng.random(inp["N"]) < 0.6)
    ptr = inp["ptr"].tolist()
    mask[ptr[1]:ptr[2]] = False  # the three-atom graph: no unmasked atom
    mask[ptr[3]] = True
    nat, t32, ref = three_way(inp, mask)
    hold_bar(f"mask_h{H}", nat, t32, ref)
    assert all_finite(nat)
    off = (~mask).to(DEV)
    assert bool((nat["alpha"][off] == 0).all())
    assert bool((nat["dx"][off] == 0).all())  # (x is a leaf here: the pool's own dx)
    assert bool((nat["g"][1] == 0).all()) and not bool(torch.signbit(nat["g"][1]).any())
    # the reference restricted to the unmasked atoms: the same numbers
    keep = mask.nonzero().squeeze(1)
    sub = compose_run(inp["x"].double()[keep], inp["batch"][keep], inp["B"], inp["w"].double(),
                      inp["b"].double(), inp["dg"].double())
    assert float((sub["g"] - ref["g"]).abs().max()) < 1e-12
    assert float((sub["alpha"] - ref["alpha"][keep]).abs().max()) < 1e-12
    # uint8 mask == bool mask, bit for bit
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inp.items()}
    u8 = native_run(d["x"], d["batch"], d["w"], d["b"], d["B"], d["dg"], ptr=d["ptr"],
                    mask=mask.to(torch.uint8).to(DEV))
    for k in nat:
        assert torch.equal(nat[k], u8[k]), k


# ----------------------------------------------------------------------------------------------
# 4. zero gate == mean pooling
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", (39, 400))
def test_zero_gate_is_mean_pooling(H, cuda_device):
    """gate.weight = 0: every score is the bias, e = exp(0) = 1, S = n exactly, alpha = fl(1 / n)
    (relative error 2^-24), and g = the fused-multiply-add chain sum_v alpha x[v]: n roundings of
    at most 2^-24 |partial sum|, each partial at most mean|x| (the column's mean of |x[v]| over
    the graph).  So |g - mean| <= (n + 1) 2^-24 mean|x| <= n 2^-23 mean|x| per column, against
    global_mean_pool in float64."""
    inp = inputs(H, seed=4)
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inp.items()}
    g, alpha = attention_pool(d["x"], d["batch"], torch.zeros_like(d["w"]), d["b"], d["B"],
                              ptr=d["ptr"])
    want = global_mean_pool(inp["x"].double(), inp["batch"], inp["B"])
    mean_abs = global_mean_pool(inp["x"].double().abs(), inp["batch"], inp["B"])
    n = torch.tensor(inp["sizes"], dtype=torch.float64)[:, None]
    assert bool(((g.cpu().double() - want).abs() <= n * 2.0 ** -23 * mean_abs).all())
    ptr = inp["ptr"].tolist()
    for b, k in enumerate(inp["sizes"]):
        if k:
            assert bool((alpha[ptr[b]:ptr[b + 1]] == float(np.float32(1.0) / np.float32(k))).all())


# ----------------------------------------------------------------------------------------------
# 5. the model
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


def attention_model(dev):
    torch.manual_seed(11)
    m = GNN(F_, FE, depth=DEPTH, hidden_sizes=[HM] * DEPTH, dropout_ps=[0.0] * DEPTH,
            activation_fn=torch.nn.functional.silu, pooling_fn=AttentionPool(HM))
    return m.to(dev).train()


def test_model_with_attention_readout(cuda_device):
    m = attention_model(cuda_device)
    data = model_batch().to_torch(cuda_device)
    B = data.ptr.numel() - 1
    y = m(data)
    assert tuple(y.shape) == (B,)
    with torch.no_grad():
        hn = m.encode_nodes(data)
    gate, ffn = m.pooling_fn.gate, m.ffn

    def head(hn, batch, mods):
        gate, ffn = mods
        g, _ = compose(hn, batch, B, gate.weight[0], gate.bias)
        return ffn(g).squeeze(-1)

    with torch.no_grad():
        y32 = head(hn, data.batch, (gate, ffn))
        y64 = head(hn.cpu().double(), data.batch.cpu(),
                   (copy.deepcopy(gate).cpu().double(), copy.deepcopy(ffn).cpu().double()))
    hold_bar("model_h39", dict(y=y.detach()), dict(y=y32), dict(y=y64), names=("y",))
    # encode: the pooled tensor itself, grad-enabled and forward-only forms
    g = m.encode(data)
    assert tuple(g.shape) == (B, HM) and g.requires_grad
    direct = m.pooling_fn(hn, data.batch, ptr=data.ptr)
    assert torch.equal(g.detach(), direct.detach())
    with torch.no_grad():
        assert torch.equal(m.encode(data), g.detach())
        assert torch.equal(m(data), y.detach())
    assert torch.equal(m.ffn(g).squeeze(-1).detach(), y.detach())
    # every gradient, full shapes
    loss = MSELoss("sum")(y, data.y)
    loss.backward()
    torch.cuda.synchronize()
    names = [k for k, _ in m.named_parameters()]
    assert "pooling_fn.gate.weight" in names and "pooling_fn.gate.bias" in names
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        assert bool(torch.isfinite(p.grad).all()), k
        if k != "pooling_fn.gate.bias":
            assert float(p.grad.abs().max()) > 0, k
    assert bool((m.pooling_fn.gate.bias.grad == 0).all())


# ----------------------------------------------------------------------------------------------
# 6. capture
# ----------------------------------------------------------------------------------------------
def test_captured_step_equals_eager(cuda_device):
    """forward, MSELoss("sum"), backward, FusedAdam.step() captured once and replayed twice on
    fresh input contents == the same two steps run eagerly, parameters bit for bit.  The batch
    carries ptr, so the step has no sync."""
    feeds = [model_batch(seed=k) for k in (1, 2)]

    def fresh():
        m = attention_model(cuda_device)
        params = list(m.parameters())
        return m, model_batch().to_torch(cuda_device), params, FusedAdam(params, lr=1e-3), \
            MSELoss("sum")

    def load(data, k):
        f = feeds[k]
        data.x.copy_(torch.from_numpy(f.x))
        data.edge_attr.copy_(torch.from_numpy(f.edge_attr))
        data.y.copy_(torch.from_numpy(f.y))

    def step(m, data, params, opt, loss_fn):
        loss = loss_fn(m(data), data.y)
        for p, gr in zip(params, torch.autograd.grad(loss, params)):
            p.grad = gr
        opt.step()

    def warm(state):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                step(*state)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()

    a = fresh()
    warm(a)
    eager = []
    for k in range(2):
        load(a[1], k)
        step(*a)
        eager.append([p.detach().clone() for p in a[2]])
    torch.cuda.synchronize()

    b = fresh()
    warm(b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(*b)
    for k in range(2):
        load(b[1], k)
        graph.replay()
        torch.cuda.synchronize()
        for p, q in zip(b[2], eager[k]):
            assert torch.equal(p.detach(), q), k
    assert any(not torch.equal(p, q) for p, q in zip(eager[0], eager[1]))
