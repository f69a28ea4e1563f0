"""GPU: GNN.encode_nodes (cgr_gnn_encode_nodes / _backward / _input_grads / _predict), the per-atom
embedding hn [N, H] as a differentiable output of the native kernels.

Reference: tests/nodes_common.py (oracle/dmpnn_numpy.py in float64 with every atom its own graph,
pinned to the encode reference by tests/test_encode_nodes_surface.py).  Bars, the
ones tests/test_gpu_encode.py uses: per tensor max|got - ref| <= 1e-4 max|ref|; learnable-skip
scalars test_gpu_parity.SKIP_COND_U with the oracle's skip_abs of the whole cotangent; predictions
1e-4 |y| + 1e-6 max|y|.  ReLU cases hand the oracle the GPU's own h > 0 decisions.

Shapes: test_gpu_encode's batches (N 70..75: three 32-row slabs of the dzn kernel, the last
partial; a one-atom graph; F odd); H = 39 (Hp 40: n_out rows 4-byte aligned only, the row's last
float4 group partial), 100 (two 64-column blocks, the second ragged), 64, 528 (the H > 512 forward
and the fp32 weight-gradient families)."""

import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from arena_contract_common import guarded_run_buffers
from conftest import golden_cases, load_golden
from encode_common import general_dg
from nodes_common import nodes_backward, nodes_forward
from stagewise_common import TORCH_F32, mixed_dy
from test_gpu_encode import (PAD, SENTINEL, Case, _raw_backward, _raw_input_grads,
                             native_precision)
from test_gpu_parity import (_pool_fn, assert_g_close, assert_y_close, batch_from_golden,
                             model_from_golden)

from cgr_mpnn_3D._amd import native
from cgr_mpnn_3D._amd.debug import ArenaRun
from cgr_mpnn_3D._amd.optim import FusedAdam
from oracle import stagewise as sw

pytestmark = pytest.mark.gpu

POOL_CODE = {"add": 0, "mean": 1, "max": 2}


class NCase(Case):
    """test_gpu_encode.Case (built with add pooling) plus the nodes-level run and reference."""

    def __init__(self, kind, H, D, act, skip, aggr, dev, precision=None, batch_none=False):
        super().__init__(kind, H, D, act, skip, aggr, "add", dev, precision, batch_none)
        self.N = self.b.x.shape[0]

    def run_nodes(self, n_out=None, pool="add", **kw):
        """cgr_gnn_encode_nodes on an arena of its own; `pool`: the config's pooling (it sizes
        the arena -- max adds a pool_arg region the nodes level never writes -- nothing else)."""
        cfg = self.cfg[:7] + (POOL_CODE[pool],) + self.cfg[8:]
        d = self.data
        return ArenaRun(cfg, d.x, d.edge_index, d.edge_attr, d.batch, d.ptr, self.B,
                        self.params(False), nodes=True, n_out=n_out, **kw)

    def nodes_reference(self, run):
        return nodes_forward(self.sd, self.b, self.D, self.act, self.skip, self.aggr,
                             self.relu_masks(run))


def _sentinel_out(N, H, dev):
    buf = torch.full((N * H + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[PAD:PAD + N * H].view(N, H)


def _dn(N, H, dev, seed=20263):
    dn_np = general_dg(N, H, seed=seed)
    return dn_np, torch.from_numpy(dn_np).to(dev)


# ----------------------------------------------------------------------------------------------
# 1. forward
# ----------------------------------------------------------------------------------------------
# name: (batch, H, D, act, skip, aggr, precision, batch=None)
FWD_CASES = {
    "ragged_silu_h39_skip": ("ragged", 39, 3, "silu", True, "add", None, False),
    "sparse_gelu_h100_mean_unbonded": ("sparse", 100, 2, "gelu", False, "mean", None, False),
    "sym_relu_h64_skip": ("sym", 64, 2, "relu", True, "add", None, False),
    "ragged_relu_h528": ("ragged", 528, 2, "relu", False, "add", None, False),
    "ragged_fe0_silu_h100_skip_fp32": ("ragged_fe0", 100, 2, "silu", True, "add", "fp32", False),
    "sym1_silu_h39_batch_none": ("sym1", 39, 2, "silu", False, "add", None, True),
}


@pytest.mark.parametrize("name", list(FWD_CASES))
def test_node_embedding_forward(name, cuda_device):
    kind, H, D, act, skip, aggr, prec, bn = FWD_CASES[name]
    c = NCase(kind, H, D, act, skip, aggr, cuda_device, prec, bn)
    N = c.N
    buf, n_out = _sentinel_out(N, H, cuda_device)
    assert n_out.data_ptr() % 16 != 0  # 4-byte aligned only
    run = c.run_nodes(n_out=n_out)
    torch.cuda.synchronize()
    # n_out is the arena's hn, bit for bit, and nothing is written outside [N, H]
    assert torch.equal(run.n_out, run.floats("hn", N))
    assert torch.all(buf[:PAD] == SENTINEL) and torch.all(buf[PAD + N * H:] == SENTINEL)
    hn_ref, _ = c.nodes_reference(run)
    assert tuple(hn_ref.shape) == (N, H)
    assert_g_close(run.n_out.cpu().numpy(), hn_ref, "hn")
    # the config's pooling takes no part: identical bits under add, mean and max
    for pool in ("mean", "max"):
        other = c.run_nodes(pool=pool)
        torch.cuda.synchronize()
        assert torch.equal(other.n_out, run.n_out), pool
    # the module: grad-enabled form == the no_grad predict form == the arena run, bitwise --
    # also for a model whose pooling_fn is a callable no native pool implements
    custom = copy.deepcopy(c.m)
    custom.pooling_fn = lambda h, batch: h.max(0)[0]
    was = native_precision(prec)
    try:
        n1 = c.m.encode_nodes(c.data)
        with torch.no_grad():
            n2 = c.m.encode_nodes(c.data)
            n3 = custom.encode_nodes(c.data)
        n4 = custom.encode_nodes(c.data)
        with pytest.raises(NotImplementedError):  # forward keeps raising
            custom(c.data)
    finally:
        native_precision(was)
    assert n1.requires_grad and n4.requires_grad and not n2.requires_grad
    assert tuple(n1.shape) == (N, H)
    for t in (n1.detach(), n2, n3, n4.detach()):
        assert torch.equal(t, run.n_out)


# ----------------------------------------------------------------------------------------------
# 2. gradients from a general dn against the float64 reference
# ----------------------------------------------------------------------------------------------
# name: (batch, H, D, act, skip, aggr, precision, batch=None, the config's pooling)
GRAD_CASES = {
    "ragged_silu_h39_skip": ("ragged", 39, 3, "silu", True, "add", None, False, "add"),
    "ragged_fe0_gelu_h100": ("ragged_fe0", 100, 2, "gelu", False, "add", None, False, "add"),
    "sparse_relu_h64_mean_skip": ("sparse", 64, 2, "relu", True, "mean", None, False, "add"),
    "unpaired_gelu_h64_skip": ("unpaired", 64, 2, "gelu", True, "add", None, False, "add"),
    "ragged_relu_h528": ("ragged", 528, 2, "relu", False, "add", None, False, "add"),
    "ragged_silu_h39_skip_fp32": ("ragged", 39, 2, "silu", True, "add", "fp32", False, "add"),
    "sym1_silu_h100_batch_none": ("sym1", 100, 2, "silu", False, "add", None, True, "add"),
    # an arena with a pool_arg region nobody wrote: a stray read of it shows here
    "ragged_silu_h39_skip_cfg_max": ("ragged", 39, 3, "silu", True, "add", None, False, "max"),
}


def _check_grads(c, grads, dx, de, g_ref, gin_ref, skip_abs):
    for name, g in zip(c.names, grads):
        if name.startswith("ffn."):
            assert g is None
            continue
        assert_g_close(g.cpu().numpy(), g_ref[name], name, skip_abs.get(name))
    assert_g_close(dx.cpu().numpy(), gin_ref["x"], "dx")
    if de is not None:
        assert_g_close(de.cpu().numpy(), gin_ref["edge_attr"], "dedge_attr")


@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_gradients_from_general_dn(name, cuda_device):
    kind, H, D, act, skip, aggr, prec, bn, pool = GRAD_CASES[name]
    c = NCase(kind, H, D, act, skip, aggr, cuda_device, prec, bn)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (the unpaired-order notice)
        if pool == "max":  # make the unwritten pool_arg region hold something to trip over
            torch.full((1 << 22,), -7, dtype=torch.int32, device=cuda_device)
        run = c.run_nodes(pool=pool)
        dn_np, dn = _dn(c.N, H, cuda_device)
        params = c.params(False)
        grads = run.backward(dn, params)
        dx, de = run.input_grads(dn, params, run.ws)
        torch.cuda.synchronize()
        _, cache = c.nodes_reference(run)
        g_ref, gin_ref, skip_abs = nodes_backward(c.sd, cache, dn_np)
        _check_grads(c, grads, dx, de, g_ref, gin_ref, skip_abs)
        # bitwise reproducible
        again = run.backward(dn, params)
        dx2, de2 = run.input_grads(dn, params, run.ws)
        torch.cuda.synchronize()
    for a, k in zip(grads, again):
        assert (a is None and k is None) or torch.equal(a, k)
    assert torch.equal(dx, dx2) and (de is None or torch.equal(de, de2))


# ----------------------------------------------------------------------------------------------
# 3. consistency with encode: under add pooling dn = dg[batch] is the same float per element
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["relu", "silu"])
@pytest.mark.parametrize("H", [39, 100])
def test_gathered_cotangent_reproduces_the_encode_backward_bitwise(H, act, cuda_device):
    c = NCase("ragged", H, 2, act, True, "add", cuda_device)
    dg = torch.from_numpy(general_dg(c.B, H)).to(cuda_device)
    dn = dg[c.data.batch].contiguous()
    enc, run = c.run(True), c.run_nodes()
    p = c.params(False)
    ge = enc.backward(dg, p)
    dxe, dee = enc.input_grads(dg, p, enc.ws)
    gn = run.backward(dn, p)
    dxn, den = run.input_grads(dn, p, run.ws)
    torch.cuda.synchronize()
    for n, a, k in zip(c.names, ge, gn):
        assert (a is None and k is None) or torch.equal(a, k), n
    assert torch.equal(dxe, dxn) and torch.equal(dee, den)


# ----------------------------------------------------------------------------------------------
# 4. the dzn stage, elementwise
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,H", [("relu", 39), ("sigmoid", 100)])
def test_dzn_stage_against_float64(act, H, cuda_device):
    """dzn = dn act'(zn) from the GPU's own zn / hn, elementwise: rho = max (|got - ref| - T)+ /
    (u S) <= max(8, 4 rho_ref) with S = |ref|, T = tol_act(zn) |dn| (oracle/stagewise.py's
    activation-derivative stage), rho_ref from an honest fp32 evaluation.
    Pad columns exactly 0.  Also: the nodes level launches its own two kernels and none of the
    pool's, the head's or encode's."""
    c = NCase("ragged", H, 2, act, True, "add", cuda_device)
    N = c.N
    dn_np, dn = _dn(N, H, cuda_device)
    params = c.params(False)
    lib = native.load()
    lib.cgr_profile_reset()
    lib.cgr_profile_enable(1)
    def once(fill):
        # arena, workspace and gradient buffer: guarded caller buffers that start from `fill`
        # (arena_contract_common.py; "ones": every float NaN, every int -1)
        E = c.b.edge_index.shape[1]
        bufs, gviews = guarded_run_buffers(c.cfg, N, E, c.B, params, fill, cuda_device)
        r = c.run_nodes(arena=bufs["arena"].payload)
        gr = r.backward(dn, params, ws=bufs["ws"].payload, grads=gviews)
        torch.cuda.synchronize()
        for k, g in bufs.items():
            g.check_guards(k)
        return r, gr

    try:
        run, grads = once("ones")  # the run judged against float64 starts from NaN
    finally:
        lib.cgr_profile_enable(0)
    classes = set(native.profile_report())
    lib.cgr_profile_reset()
    run2, grads2 = once("zero")  # ... and equals, bit for bit, the one that starts from 0
    same = [("n_out", run.n_out, run2.n_out), ("hn", run.floats("hn", N), run2.floats("hn", N)),
            ("dzn_main", run.ws_floats_padded("dzn_main", N),
             run2.ws_floats_padded("dzn_main", N)),
            ("ds", run.ws_floats("ds", N), run2.ws_floats("ds", N))]
    same += [(k, a, b) for k, a, b in zip(c.names, grads, grads2) if a is not None]
    for k, a, b in same:
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f"{k} depends on the fill"
    assert {"nodes_out_fwd", "nodes_act_bwd"} <= classes, sorted(classes)
    assert not {"pool_only_fwd", "pool_head_fwd", "head_bwd", "readout_act_bwd_dg",
                "readout_act_bwd"} & classes, sorted(classes)
    got = run.ws_floats_padded("dzn_main", N).cpu().numpy()
    assert got.shape == (N, run.Hp)
    assert not got[:, H:].any()  # pad columns: exactly 0
    assert np.array_equal(run.ws_floats("dzn_main", N).cpu().numpy(), got[:, :H])
    hn = run.floats("hn", N).cpu().numpy()
    zn = None if act == "relu" else run.floats("zn", N).cpu().numpy()

    def stage(ops):
        d, t = sw.act_grad_of(zn, hn, act, ops)
        ref = ops.arr(dn_np) * d
        return sw.Stage(ref, np.abs(np.asarray(ref, np.float64)),
                        t * np.abs(np.asarray(dn_np, np.float64)))

    st, st32 = stage(sw.REF), stage(TORCH_F32)
    r, at = sw.rho(got[:, :H], st)
    rr, _ = sw.rho(st32.ref, st)
    print(f"dzn {act} H {H}: rho {r:.2f}  rho_ref {rr:.2f}  bar {sw.bar(rr):.2f}  at {at}")
    assert r <= sw.bar(rr), (r, rr, at)
    assert np.abs(got).max() > 0


# ----------------------------------------------------------------------------------------------
# 5. dropout: same keying, same counter advance
# ----------------------------------------------------------------------------------------------
def test_dropout_nodes_equal_fused_arena_and_counter_advances(cuda_device):
    c = NCase("ragged", 39, 3, "sigmoid", True, "add", cuda_device)
    ps, seed = [0.25] * 3, 2**40 + 77
    outs, keys = [], []
    for nodes in (False, True):
        counter = torch.tensor([9], dtype=torch.int64, device=cuda_device)
        kw = dict(dropout_ps=ps, seed=seed, training=True, rng_counter=counter)
        r = c.run_nodes(**kw) if nodes else c.run(False, **kw)
        torch.cuda.synchronize()
        assert int(counter.item()) == 10
        outs.append(r.n_out if nodes else r.floats("hn", c.N))
        keys.append(r.rng_key())
        E = c.b.edge_index.shape[1]
        assert bool((r.floats("h", E, index=1) == 0).any())  # sigmoid: zeros are drops
    assert keys[0] == keys[1] and torch.equal(outs[0], outs[1])
    counter = torch.tensor([9], dtype=torch.int64, device=cuda_device)
    c.run_nodes(dropout_ps=[0.0] * 3, seed=seed, training=True, rng_counter=counter)
    torch.cuda.synchronize()
    assert int(counter.item()) == 9  # a no-drop forward leaves the counter alone


# ----------------------------------------------------------------------------------------------
# 6. composition: any readout in PyTorch on the native node embedding
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", golden_cases())
def test_pool_and_head_on_node_embedding_match_golden_predictions(case, cuda_device):
    z, meta = load_golden(case)
    m = model_from_golden(z, meta, cuda_device)
    m.eval()
    data = batch_from_golden(z, meta, cuda_device)
    pool = _pool_fn(meta.get("pool", "add"))
    with torch.no_grad():
        hn = m.encode_nodes(data)
        g = pool(hn, data.batch) if data.batch is None else \
            pool(hn, data.batch, int(z["out_y_eval"].shape[0]))
        y = m.ffn(g).squeeze(-1)
    assert tuple(y.shape) == tuple(z["out_y_eval"].shape)
    assert_y_close(y.cpu().numpy(), z["out_y_eval"])


def attention_readout(att, hn, batch, B, dense=False):
    """g[b] = sum_{v in b} softmax_b(att(hn))[v] hn[v].  The scores are shifted by their global
    maximum (any per-graph constant leaves the softmax unchanged).  dense: the per-graph sums as
    masked reductions over a one-hot [B, N] instead of index_add_ -- the same sums without
    atomics, so that a captured step and an eager one add in the same order."""
    s = att(hn).squeeze(-1)
    e = torch.exp(s - s.max().detach())
    if dense:
        onehot = (batch[None, :] == torch.arange(B, device=batch.device)[:, None]).to(hn.dtype)
        w = e / (onehot * e[None, :]).sum(1)[batch]
        return (onehot[:, :, None] * (w[:, None] * hn)[None]).sum(1)
    w = e / torch.zeros(B, dtype=hn.dtype, device=hn.device).index_add_(0, batch, e)[batch]
    return torch.zeros(B, hn.shape[1], dtype=hn.dtype, device=hn.device).index_add_(
        0, batch, w[:, None] * hn)


def test_attention_readout_loss_gradients(cuda_device):
    H, D = 39, 2
    c = NCase("ragged", H, D, "silu", True, "add", cuda_device)
    torch.manual_seed(6)
    att = nn.Linear(H, 1).to(cuda_device)
    c.data.x.requires_grad_(True)
    c.data.edge_attr.requires_grad_(True)
    y = c.m.ffn(attention_readout(att, c.m.encode_nodes(c.data), c.data.batch, c.B)).squeeze(-1)
    wgt = torch.from_numpy(mixed_dy(c.B)).to(cuda_device)
    (wgt * y).sum().backward()
    torch.cuda.synchronize()
    # reference: readout and head in float64 torch on the oracle's hn; its dn into the oracle
    hn_ref, cache = nodes_forward(c.sd, c.b, D, "silu", True, "add")
    att64, ffn64 = copy.deepcopy(att).cpu().double(), copy.deepcopy(c.m.ffn).cpu().double()
    att64.zero_grad(), ffn64.zero_grad()
    hn64 = torch.from_numpy(hn_ref).requires_grad_(True)
    scores = []  # att64's output, with its gradient kept

    def keep(mod, inp, out):
        out.retain_grad()
        scores.append(out)

    att64.register_forward_hook(keep)
    y64 = ffn64(attention_readout(att64, hn64, torch.from_numpy(c.b.batch), c.B)).squeeze(-1)
    assert_y_close(y.detach().cpu().numpy(), y64.detach().numpy())
    (wgt.cpu().double() * y64).sum().backward()
    # att.bias's gradient is one scalar, the sum over atoms of the scores' gradients, and a
    # softmax is shift-invariant: the sum cancels to exactly 0.  Like a learnable-skip scalar it
    # is held to its conditioning, SKIP_COND_U sum |terms| (test_gpu_parity.assert_g_close)
    cond = {"att.bias": float(scores[0].grad.abs().sum())}
    for mod, mod64, tag in ((att, att64, "att."), (c.m.ffn, ffn64, "ffn.")):
        for (k, p), (_, q) in zip(mod.named_parameters(), mod64.named_parameters()):
            assert_g_close(p.grad.cpu().numpy(), q.grad.numpy(), tag + k, cond.get(tag + k))
    gr, gin, skip_abs = nodes_backward(c.sd, cache, hn64.grad.numpy())
    for k, p in c.m.named_parameters():
        if not k.startswith("ffn."):
            assert_g_close(p.grad.cpu().numpy(), gr[k], k, skip_abs.get(k))
    assert_g_close(c.data.x.grad.cpu().numpy(), gin["x"], "dx")
    assert_g_close(c.data.edge_attr.grad.cpu().numpy(), gin["edge_attr"], "dedge_attr")
    # per-atom attribution under add pooling and the linear head: the shares sum to y - bf
    with torch.no_grad():
        share = c.m.encode_nodes(c.data) @ c.m.ffn.weight.T
        tot = torch.zeros(c.B, 1, device=cuda_device).index_add_(0, c.data.batch, share)
        assert_y_close((tot + c.m.ffn.bias).squeeze(-1).cpu().numpy(),
                       c.m(c.data).cpu().numpy())


# ----------------------------------------------------------------------------------------------
# 7. capture
# ----------------------------------------------------------------------------------------------
def test_captured_attention_adam_step_equals_eager(cuda_device):
    """encode_nodes -> attention readout -> ffn -> loss -> backward -> FusedAdam.step(),
    captured: three replays equal three eager steps from the same state, parameters and node
    embeddings (the method of test_gpu_encode's captured step)."""
    H, D = 39, 2

    def fresh():
        c = NCase("ragged", H, D, "silu", True, "add", cuda_device)
        torch.manual_seed(6)
        att = nn.Linear(H, 1).to(cuda_device)
        params = list(c.m.parameters()) + list(att.parameters())
        return c, att, params, FusedAdam(params, lr=1e-3), torch.zeros(c.N, H, device=cuda_device)

    def step(c, att, params, opt, emb):
        hn = c.m.encode_nodes(c.data)
        y = c.m.ffn(attention_readout(att, hn, c.data.batch, c.B, dense=True)).squeeze(-1)
        loss = ((y - c.data.y) ** 2).sum()
        for p, gr in zip(params, torch.autograd.grad(loss, params)):
            p.grad = gr
        opt.step()
        emb.copy_(hn.detach())

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
    for _ in range(3):
        step(*a)
        eager.append((a[4].clone(), [p.detach().clone() for p in a[2]]))
    torch.cuda.synchronize()

    b = fresh()
    warm(b)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(*b)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(b[4], eager[k][0]), k
        for p, q in zip(b[2], eager[k][1]):
            assert torch.equal(p.detach(), q), k


# ----------------------------------------------------------------------------------------------
# 8. refusals
# ----------------------------------------------------------------------------------------------
def test_arena_level_and_precision_refusals(cuda_device):
    """Every refusal returns an error code, names the call that belongs to the arena in
    cgr_last_error and enqueues nothing: sentinel-filled gradients, workspace and input-gradient
    buffers stay untouched."""
    H = 39
    c = NCase("ragged", H, 2, "silu", False, "add", cuda_device)
    lib = native.load()
    dy = torch.from_numpy(mixed_dy(c.B)).to(cuda_device)
    dg = torch.from_numpy(general_dg(c.B, H)).to(cuda_device)
    _, dn = _dn(c.N, H, cuda_device)
    nodes, enc, fused = c.run_nodes(), c.run(True), c.run(False)
    pf, pe = c.params(True), c.params(False)
    N, E = c.N, c.b.edge_index.shape[1]
    nws = lib.cgr_gnn_workspace_bytes(ctypes.byref(nodes.cfg), N, E, c.B)

    def sentinels():
        ws = torch.full((nws,), 0x5A, dtype=torch.uint8, device=cuda_device)
        grads = [torch.full_like(p, SENTINEL) for p in pf]
        dx = torch.full((N, c.b.x.shape[1]), SENTINEL, device=cuda_device)
        de = torch.full((E, 14), SENTINEL, device=cuda_device)
        return ws, grads, dx, de

    def untouched(ws, grads, dx, de):
        torch.cuda.synchronize()
        return bool((ws == 0x5A).all()) and all(bool((g == SENTINEL).all()) for g in grads) \
            and bool((dx == SENTINEL).all()) and bool((de == SENTINEL).all())

    def refused(rc, text, bufs):
        assert rc != 0 and text in lib.cgr_last_error().decode(), lib.cgr_last_error()
        assert untouched(*bufs)

    bufs = sentinels()
    ws, grads, dx, de = bufs
    # a nodes arena given to the fused and the encode entries
    own_b = "its backward is cgr_gnn_encode_nodes_backward"
    own_i = "its input gradients are cgr_gnn_encode_nodes_input_grads"
    refused(_raw_backward(lib.cgr_gnn_backward, nodes, dy, pf, grads, ws),
            "cgr_gnn_backward: `arena` was filled by cgr_gnn_encode_nodes (", bufs)
    assert own_b in lib.cgr_last_error().decode()
    refused(_raw_backward(lib.cgr_gnn_encode_backward, nodes, dg, pf, grads, ws),
            "cgr_gnn_encode_backward: `arena` was filled by cgr_gnn_encode_nodes (", bufs)
    assert own_b in lib.cgr_last_error().decode()
    refused(_raw_input_grads(lib.cgr_gnn_input_grads, nodes, dy, pf, ws, dx, de),
            "cgr_gnn_input_grads: `arena` was filled by cgr_gnn_encode_nodes (", bufs)
    assert own_i in lib.cgr_last_error().decode()
    refused(_raw_input_grads(lib.cgr_gnn_encode_input_grads, nodes, dg, pe, ws, dx, de),
            "cgr_gnn_encode_input_grads: `arena` was filled by cgr_gnn_encode_nodes (", bufs)
    assert own_i in lib.cgr_last_error().decode()
    # a fused or an encode arena given to the nodes entries
    refused(_raw_backward(lib.cgr_gnn_encode_nodes_backward, fused, dn, pf, grads, ws),
            "cgr_gnn_encode_nodes_backward: `arena` was filled by cgr_gnn_forward (with the ffn "
            "head); its backward is cgr_gnn_backward", bufs)
    refused(_raw_backward(lib.cgr_gnn_encode_nodes_backward, enc, dn, pf, grads, ws),
            "cgr_gnn_encode_nodes_backward: `arena` was filled by cgr_gnn_encode (headless, no "
            "ffn head); its backward is cgr_gnn_encode_backward", bufs)
    refused(_raw_input_grads(lib.cgr_gnn_encode_nodes_input_grads, fused, dn, pe, ws, dx, de),
            "cgr_gnn_encode_nodes_input_grads: `arena` was filled by cgr_gnn_forward (with the "
            "ffn head); its input gradients are cgr_gnn_input_grads", bufs)
    refused(_raw_input_grads(lib.cgr_gnn_encode_nodes_input_grads, enc, dn, pe, ws, dx, de),
            "cgr_gnn_encode_nodes_input_grads: `arena` was filled by cgr_gnn_encode (headless, no "
            "ffn head); its input gradients are cgr_gnn_encode_input_grads", bufs)
    # no backward was recorded by any of these: the nodes input gradients find none
    refused(_raw_input_grads(lib.cgr_gnn_encode_nodes_input_grads, nodes, dn, pe, ws, dx, de),
            "does not hold a cgr_gnn_encode_nodes_backward", bufs)
    nodes.backward(dn, pe)  # a real one, into nodes.ws
    nodes.cfg.precision = 1  # the arena's forward ran in the split-bf16 mode
    refused(_raw_backward(lib.cgr_gnn_encode_nodes_backward, nodes, dn, pf, grads, ws),
            "cgr_gnn_encode_nodes_backward: the config's precision differs", bufs)
    refused(_raw_input_grads(lib.cgr_gnn_encode_nodes_input_grads, nodes, dn, pe, nodes.ws, dx,
                             de),
            "cgr_gnn_encode_nodes_input_grads: the config's precision differs", bufs)


def test_encode_nodes_with_a_bucket_hook_raises_when_gradients_are_wanted(cuda_device):
    from cgr_mpnn_3D._amd import config

    c = NCase("ragged", 39, 2, "silu", False, "add", cuda_device)
    c.m._grad_bucket_hook = lambda flat, buckets, events: None
    with pytest.raises(NotImplementedError, match="gradient-bucket hook"):
        c.m.encode_nodes(c.data)
    with torch.no_grad():
        assert tuple(c.m.encode_nodes(c.data).shape) == (c.N, 39)
    c.m._grad_bucket_hook = None
    was = config.grad_bucket_hook
    config.grad_bucket_hook = lambda flat, buckets, events: None
    try:
        with pytest.raises(NotImplementedError, match="gradient-bucket hook"):
            c.m.encode_nodes(c.data)
    finally:
        config.grad_bucket_hook = was
    assert c.m.encode_nodes(c.data).requires_grad
