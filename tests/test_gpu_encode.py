"""GPU: GNN.encode (cgr_gnn_encode / _encode_backward / _encode_input_grads / _encode_predict) and
the routed GNN.forward for any ffn head.

Reference: tests/encode_common.py (oracle/dmpnn_numpy.py in float64, pinned against finite
differences by tests/test_encode_surface.py).  Bars: per tensor
max|got - ref| <= 1e-4 max|ref|; learnable-skip scalars test_gpu_parity.SKIP_COND_U with the
oracle's skip_abs; predictions 1e-4 |y| + 1e-6 max|y|.  ReLU cases hand the oracle the GPU's own
h > 0 decisions read from the arena (relu_masks), as tests/test_gpu_parity.py does.

Shapes: H = 39 (Hp 40, H = 3 mod 4: unaligned g_out rows, one partial 64-column image block),
100 (two image column blocks, the second ragged), 64, 528 (fp32 TN families); N >= 70 (three
32-row slabs of the dzn kernel, the last partial); 5 ragged graphs, one a single atom; atoms
without bonds under mean aggregation; F odd; Fe = 14 and 0; D = 2 or 3."""

import copy
import ctypes
import io
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn

from arena_contract_common import guarded_run_buffers
from conftest import golden_cases, load_golden
from encode_common import encode_backward, encode_forward, general_dg, ragged_batch
from stagewise_common import TORCH_F32, failures, mixed_dy, param_names, write_report
from test_gpu_parity import (ACT, SKIP_COND_U, _cfg_tuple, _pool_fn, _shuffled_pairs,
                             _sparse_batch, assert_g_close, assert_y_close, batch_from_golden,
                             model_from_golden)

from cgr_mpnn_3D._amd import native
from cgr_mpnn_3D._amd.debug import ArenaRun
from cgr_mpnn_3D._amd.optim import FusedAdam
from cgr_mpnn_3D._amd.synth import TorchBatch, make_batch, make_symmetric_batch
from cgr_mpnn_3D.models.GNN import GNN
from oracle import stagewise as sw

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
PAD = 5  # floats around g_out in its sentinel buffer (g_out itself then 4-byte aligned only)


def _batch(kind):
    if kind == "ragged":  # N 73, B 5, a one-atom graph, F odd, Fe 14
        return ragged_batch()
    if kind == "ragged_fe0":
        return ragged_batch(seed=8, fe0=True)
    if kind == "sparse":  # N 75: most atoms without bonds (in-degree 0), F 21, Fe 14
        return _sparse_batch(5, 15, seed=33)
    if kind == "sym":  # N 70: three identical leaves per graph -> max-pool ties
        return make_symmetric_batch(5, n_leaves=3, n_chain=10, n_mace=3, seed=21)
    if kind == "sym1":  # one graph, run with batch=None: N 74
        return make_symmetric_batch(1, n_leaves=3, n_chain=70, n_mace=3, seed=22)
    if kind == "unpaired":  # N 75, edges shuffled inside every graph
        return _shuffled_pairs(make_batch(5, n_atoms=15, n_bonds=16, n_mace=3, seed=23), seed=4)
    raise KeyError(kind)


class Case:
    """Model (seeded), its float64 parameters, the batch on the device and the config tuple."""

    def __init__(self, kind, H, D, act, skip, aggr, pool, dev, precision=None, batch_none=False):
        self.b = b = _batch(kind)
        self.H, self.D, self.act, self.skip, self.aggr, self.pool = H, D, act, skip, aggr, pool
        self.batch_none = batch_none
        F_, Fe = b.x.shape[1], b.edge_attr.shape[1]
        torch.manual_seed(3)
        m = GNN(F_, Fe, depth=D, hidden_sizes=[H] * D, dropout_ps=[0.0] * D,
                activation_fn=ACT[act], use_learnable_skip=skip, aggr=aggr,
                pooling_fn=_pool_fn(pool))
        if skip:
            with torch.no_grad():
                for i, w in enumerate(m.skip_weights):
                    w.fill_(0.5 + 0.25 * i)
        self.sd = {k: v.detach().numpy().astype(np.float64) for k, v in m.state_dict().items()}
        self.m = m.to(dev).train()
        d = b.to_torch(dev)
        # (ArenaRun hands raw pointers to the library: _sparse_batch's edge_index is a transpose)
        d.edge_index = d.edge_index.contiguous()
        self.data = TorchBatch(d.x, d.edge_index, d.edge_attr, None, None, d.y) if batch_none \
            else d
        self.B = 1 if batch_none else b.num_graphs
        self.cfg = _cfg_tuple(F_, Fe, H, D, act, skip, aggr, pool)
        if precision is not None:
            self.cfg = self.cfg + ({"split": 0, "fp32": 1}[precision],)
        self.names = param_names(D, skip)

    def params(self, head=True):
        return [None if p is None else p.detach().contiguous()
                for p in self.m.native_parameters(head)]

    def run(self, encode, g_out=None, **kw):
        d = self.data
        return ArenaRun(self.cfg, d.x, d.edge_index, d.edge_attr, d.batch, d.ptr, self.B,
                        self.params(not encode), encode=encode, g_out=g_out, **kw)

    def relu_masks(self, run):
        """The GPU's own h > 0 decisions, in the caller's edge order (ReLU cases)."""
        if self.act != "relu":
            return None
        N, E = self.b.x.shape[0], self.b.edge_index.shape[1]
        perm = run.ints("perm", E).long().cpu().numpy()

        def unsort(t):
            out = np.empty_like(t)
            out[perm] = t
            return out

        return {"z0": unsort(run.floats("h", E, index=0).cpu().numpy()) > 0,
                "zs": [unsort(run.floats("h", E, index=l + 1).cpu().numpy()) > 0
                       for l in range(self.D)],
                "zn": run.floats("hn", N).cpu().numpy() > 0}

    def reference(self, run):
        return encode_forward(self.sd, self.b, self.D, self.act, self.skip, self.aggr, self.pool,
                              self.batch_none, self.relu_masks(run))


def _sentinel_out(B, H, dev):
    buf = torch.full((B * H + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[PAD:PAD + B * H].view(B, H)


# ----------------------------------------------------------------------------------------------
# 1. the fingerprint, forward
# ----------------------------------------------------------------------------------------------
FWD_CASES = {
    "add_add_silu_h39": ("ragged", 39, 3, "silu", True, "add", "add", None, False),
    "mean_mean_gelu_h100_unbonded": ("sparse", 100, 2, "gelu", False, "mean", "mean", None, False),
    "max_ties_relu_h64": ("sym", 64, 2, "relu", True, "add", "max", None, False),
    "max_batch_none_silu_h39": ("sym1", 39, 2, "silu", False, "add", "max", None, True),
    "add_relu_h528": ("ragged", 528, 2, "relu", False, "add", "add", None, False),
    "mean_silu_h100_fe0_fp32": ("ragged_fe0", 100, 2, "silu", True, "add", "mean", "fp32", False),
}


@pytest.mark.parametrize("name", list(FWD_CASES))
def test_fingerprint_forward(name, cuda_device):
    kind, H, D, act, skip, aggr, pool, prec, bn = FWD_CASES[name]
    c = Case(kind, H, D, act, skip, aggr, pool, cuda_device, prec, bn)
    fused = c.run(False)
    buf, g_out = _sentinel_out(c.B, H, cuda_device)
    enc = c.run(True, g_out=g_out)
    torch.cuda.synchronize()
    # the pool variant keeps the summation order: the fused arena's g, bit for bit
    assert torch.equal(enc.g_out, fused.floats("g", c.B))
    assert torch.equal(enc.floats("g", c.B), fused.floats("g", c.B))
    # nothing written outside [B, H] (H = 39: the row's last float4 group)
    assert torch.all(buf[:PAD] == SENTINEL) and torch.all(buf[PAD + c.B * H:] == SENTINEL)
    g_ref, _ = c.reference(enc)
    assert tuple(g_ref.shape) == (c.B, H)
    assert_g_close(enc.g_out.cpu().numpy(), g_ref, "g")
    # the module: grad-enabled form == the no_grad predict form == the arena run, bitwise
    was = native_precision(prec)
    try:
        g1 = c.m.encode(c.data)
        with torch.no_grad():
            g2 = c.m.encode(c.data)
    finally:
        native_precision(was)
    assert g1.requires_grad and not g2.requires_grad and tuple(g1.shape) == (c.B, H)
    assert torch.equal(g1.detach(), g2) and torch.equal(g2, enc.g_out)


def native_precision(value):
    """Set the process precision switch (None: leave), return the previous value."""
    from cgr_mpnn_3D._amd import config

    was = config.precision
    if value is not None:
        config.precision = value
    return was


# ----------------------------------------------------------------------------------------------
# 2. dropout: same keying, same counter advance
# ----------------------------------------------------------------------------------------------
def test_dropout_fingerprint_equals_fused_arena_and_counter_advances(cuda_device):
    c = Case("ragged", 39, 3, "sigmoid", True, "add", "add", cuda_device)
    ps, seed = [0.25] * 3, 2**40 + 77
    outs, keys = [], []
    for encode in (False, True):
        counter = torch.tensor([9], dtype=torch.int64, device=cuda_device)
        r = c.run(encode, dropout_ps=ps, seed=seed, training=True, rng_counter=counter)
        torch.cuda.synchronize()
        assert int(counter.item()) == 10
        outs.append(r.g_out if encode else r.floats("g", c.B))
        keys.append(r.rng_key())
        E = c.b.edge_index.shape[1]
        assert bool((r.floats("h", E, index=1) == 0).any())  # sigmoid: zeros are drops
    assert keys[0] == keys[1] and torch.equal(outs[0], outs[1])
    counter = torch.tensor([9], dtype=torch.int64, device=cuda_device)
    c.run(True, dropout_ps=[0.0] * 3, seed=seed, training=True, rng_counter=counter)
    torch.cuda.synchronize()
    assert int(counter.item()) == 9  # a no-drop forward leaves the counter alone


# ----------------------------------------------------------------------------------------------
# 3. gradients from a general dg against the float64 reference
# ----------------------------------------------------------------------------------------------
GRAD_CASES = {
    "add_add_silu_h39_skip": ("ragged", 39, 3, "silu", True, "add", "add", None, False),
    "mean_add_gelu_h100_fe0": ("ragged_fe0", 100, 2, "gelu", False, "add", "mean", None, False),
    "max_add_silu_h39_ties_skip": ("sym", 39, 2, "silu", True, "add", "max", None, False),
    "add_mean_relu_h64_unbonded_skip": ("sparse", 64, 2, "relu", True, "mean", "add", None, False),
    "mean_mean_silu_h100_unbonded": ("sparse", 100, 2, "silu", False, "mean", "mean", None, False),
    "max_mean_relu_h39_skip": ("ragged", 39, 3, "relu", True, "mean", "max", None, False),
    "add_gelu_h64_unpaired_skip": ("unpaired", 64, 2, "gelu", True, "add", "add", None, False),
    "add_relu_h528": ("ragged", 528, 2, "relu", False, "add", "add", None, False),
    "mean_silu_h39_skip_fp32": ("ragged", 39, 2, "silu", True, "add", "mean", "fp32", False),
    "max_batch_none_silu_h100": ("sym1", 100, 2, "silu", False, "add", "max", None, True),
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
def test_gradients_from_general_dg(name, cuda_device):
    kind, H, D, act, skip, aggr, pool, prec, bn = GRAD_CASES[name]
    c = Case(kind, H, D, act, skip, aggr, pool, cuda_device, prec, bn)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (the unpaired-order notice)
        enc = c.run(True)
        dg_np = general_dg(c.B, H)
        dg = torch.from_numpy(dg_np).to(cuda_device)
        params = c.params(False)
        grads = enc.backward(dg, params)
        dx, de = enc.input_grads(dg, params, enc.ws)
        torch.cuda.synchronize()
        _, cache = c.reference(enc)
        g_ref, gin_ref, skip_abs = encode_backward(c.sd, cache, dg_np)
        _check_grads(c, grads, dx, de, g_ref, gin_ref, skip_abs)
        # bitwise reproducible
        again = enc.backward(dg, params)
        dx2, de2 = enc.input_grads(dg, params, enc.ws)
        torch.cuda.synchronize()
    for a, k in zip(grads, again):
        assert (a is None and k is None) or torch.equal(a, k)
    assert torch.equal(dx, dx2) and (de is None or torch.equal(de, de2))


# ----------------------------------------------------------------------------------------------
# 4. consistency with the fused path: a rank-1 cotangent dg = dy (x) wf
# ----------------------------------------------------------------------------------------------
RANK1_CASES = {
    "max_silu_h39_ties": ("sym", 39, 2, "silu", True, "add", "max", False, True),
    "max_relu_h100": ("ragged", 100, 2, "relu", False, "mean", "max", False, True),
    "max_batch_none_gelu_h64": ("sym1", 64, 2, "gelu", True, "add", "max", True, True),
    "add_relu_h39": ("ragged", 39, 3, "relu", True, "add", "add", False, False),
    "mean_relu_h100_unbonded": ("sparse", 100, 2, "relu", False, "mean", "mean", False, False),
    "add_silu_h528": ("ragged", 528, 2, "silu", False, "add", "add", False, False),
}


@pytest.mark.parametrize("name", list(RANK1_CASES))
def test_rank1_cotangent_reproduces_the_fused_backward(name, cuda_device):
    kind, H, D, act, skip, aggr, pool, bn, bitwise = RANK1_CASES[name]
    c = Case(kind, H, D, act, skip, aggr, pool, cuda_device, None, bn)
    dy = torch.from_numpy(mixed_dy(c.B)).to(cuda_device)
    wf = c.m.ffn.weight.detach()
    dg = (dy[:, None] * wf).contiguous()  # torch fp32: the product the fused dzn kernel forms
    fused, enc = c.run(False), c.run(True)
    pf, pe = c.params(True), c.params(False)
    gf = fused.backward(dy, pf)
    dxf, def_ = fused.input_grads(dy, pf, fused.ws)
    ge = enc.backward(dg, pe)
    dxe, dee = enc.input_grads(dg, pe, enc.ws)
    torch.cuda.synchronize()
    skip_abs = {}
    if not bitwise and skip:  # the oracle's skip_abs of this very cotangent
        _, cache = c.reference(enc)
        _, _, skip_abs = encode_backward(c.sd, cache, dg.cpu().numpy())
    pairs = [(n, a, k) for n, a, k in zip(c.names, gf, ge) if not n.startswith("ffn.")]
    pairs += [("dx", dxf, dxe)] + ([("dedge_attr", def_, dee)] if dee is not None else [])
    for n, a, k in pairs:
        if bitwise:  # same operands, same operation order
            assert torch.equal(a, k), n
        else:  # (dy gscale) wf vs (dy wf) gscale, LdActGradT's factors vs the materialised dzn
            assert_g_close(k.cpu().numpy(), a.cpu().numpy(), n, skip_abs.get(n))


# ----------------------------------------------------------------------------------------------
# 5. the stages the feature touches, each from the GPU's own inputs to it (oracle/stagewise.py)
# ----------------------------------------------------------------------------------------------
# name: (batch, H, D, act, skip, aggr, pool, precision, weight-gradient family of the readout)
STAGE_CASES = {
    "e01_silu_h39_mean_pool": ("ragged", 39, 3, "silu", True, "add", "mean", None, "b3"),
    "e02_relu_h100_max_ties": ("sym", 100, 2, "relu", False, "add", "max", None, "b3"),
    "e03_gelu_h64_unbonded": ("sparse", 64, 2, "gelu", True, "mean", "mean", None, "b3"),
    "e04_silu_h528": ("ragged", 528, 2, "silu", False, "add", "add", None, "f32"),
    "e05_silu_h39_fp32_mode": ("ragged", 39, 2, "silu", True, "mean", "add", "fp32", "f32"),
}
READOUT_TN = "gemm_tn_wgrad_readout"


def _encode_stages(rec, ops):
    """(name, got, Stage, additive bar term) of g, ds, dW_n, db_n and dx, each evaluated by `ops`
    with oracle/stagewise.py's public functions from the record's own inputs to that stage.  dzn
    is the one stage no implementation has to store: formed here as stagewise.readout_dzn forms
    it, with the upstream value dg[graph(v)] in place of dy[graph(v)] wf."""
    gid, act = rec["node_graph"], rec["act"]
    yield "g", rec["g"], sw.pool(rec["hn"], gid, rec["B"], rec["pool"], rec["inv_cnt"], ops), 0.0
    up = ops.arr(rec["dg"])[gid]
    if rec["inv_cnt"] is not None:
        up = up * ops.arr(rec["inv_cnt"])[gid][:, None]
    if rec["pool"] == "max":
        up = up * ops.arr(sw.max_pool_share(rec["hn"], rec["g"], gid, True))
    d, t = sw.act_grad_of(rec["zn"], rec["hn"], act, ops)
    ref = up * d
    up64 = np.abs(np.asarray(up, np.float64))
    dzn = sw.Stage(ref, np.abs(np.asarray(ref, np.float64)), t * up64)
    yield "ds", rec["ds"], sw.readout_ds(dzn, rec["wn"][:, rec["F"]:], rec["inv_deg"], ops), 0.0
    b3 = rec["family"] == "b3"
    qn = np.concatenate([np.asarray(rec["x"], np.float64), np.asarray(rec["aD"], np.float64)], 1)
    yield ("dW_n", rec["dWn"], sw.tn(dzn.ref, qn, ops, dzn.T),
           sw.TN_SPLIT_WORST if b3 else 0.0)
    yield "db_n", rec["dbn"], sw.colsum(dzn.ref, ops, dzn.T), sw.TN_BIAS_WORST if b3 else 0.0
    dx, _ = sw.input_grads(rec["dpre0"], dzn, rec["w0"], rec["wn"], rec["src_s"], rec["perm"],
                           rec["x"].shape[0], rec["F"], ops)
    yield "dx", rec["dx"], dx, 0.0


@pytest.mark.parametrize("name", list(STAGE_CASES))
def test_encode_stages_against_float64(name, cuda_device):
    """rho = max (|got - ref| - T)+ / (u S) <= max(8, 4 rho_ref), + 768 /
    + 256 for dW_n / db_n where the readout weight gradient runs on the split-bf16 family (dzn
    reaches it as an e-image only); rho_ref from stagewise_common.TORCH_F32."""
    kind, H, D, act, skip, aggr, pool, prec, family = STAGE_CASES[name]
    c = Case(kind, H, D, act, skip, aggr, pool, cuda_device, prec)
    N, E, F_ = c.b.x.shape[0], c.b.edge_index.shape[1], c.b.x.shape[1]
    dg_np = general_dg(c.B, H)
    dg = torch.from_numpy(dg_np).to(cuda_device)
    params = c.params(False)
    lib = native.load()
    lib.cgr_profile_reset()
    lib.cgr_profile_enable(1)
    def once(fill):
        # arena, workspace and gradient buffer: guarded caller buffers that start from `fill`
        # (arena_contract_common.py; "ones": every float NaN, every int -1)
        bufs, gviews = guarded_run_buffers(c.cfg, N, E, c.B, params, fill, cuda_device)
        run = c.run(True, arena=bufs["arena"].payload)
        gr = run.backward(dg, params, ws=bufs["ws"].payload, grads=gviews)
        gx, _ = run.input_grads(dg, params, run.ws)
        torch.cuda.synchronize()
        for k, g in bufs.items():
            g.check_guards(k)
        return run, gr, gx

    try:
        enc, grads, dx = once("ones")  # the run judged against float64 starts from NaN
    finally:
        lib.cgr_profile_enable(0)
    classes = set(native.profile_report())
    lib.cgr_profile_reset()
    enc2, grads2, dx2 = once("zero")  # ... and equals, bit for bit, the one that starts from 0
    same = [("g_out", enc.g_out, enc2.g_out), ("dx", dx, dx2)]
    same += [(k, a, b) for k, a, b in zip(c.names, grads, grads2) if a is not None]
    same += [(k, enc.floats(k, n), enc2.floats(k, n)) for k, n in (("hn", N), ("g", c.B))]
    same += [(k, enc.ws_floats(k, n), enc2.ws_floats(k, n))
             for k, n in (("ds", N), ("dpre0", E), ("dzn_main", N))]
    for k, a, b in same:
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), \
            f"{name}: {k} depends on the fill"
    assert {"pool_only_fwd", "readout_act_bwd_dg"} <= classes and "head_bwd" not in classes
    forms = [f for f in ("", "[tnr]", "[f32]") if READOUT_TN + f in classes]
    assert len(forms) == 1 and (forms[0] == "") == (family == "b3"), sorted(classes)

    def npa(t):
        return t.detach().cpu().numpy().copy()

    G = dict(zip(c.names, grads))
    gid = npa(enc.ints("node_graph", N)).astype(np.int64)
    dst = npa(enc.ints("dst_s", E)).astype(np.int64)
    rec = dict(B=c.B, act=act, pool=pool, F=F_, family=family, dg=dg_np, node_graph=gid,
               x=c.b.x, hn=npa(enc.floats("hn", N)), g=npa(enc.floats("g", c.B)),
               zn=None if act == "relu" else npa(enc.floats("zn", N)),
               aD=npa(enc.floats("a", N, index=D)), ds=npa(enc.ws_floats("ds", N)),
               dpre0=npa(enc.ws_floats("dpre0", E)),
               src_s=npa(enc.ints("src_s", E)).astype(np.int64),
               perm=npa(enc.ints("perm", E)).astype(np.int64),
               w0=c.sd["edge_init.weight"], wn=c.sd["edge_to_node.weight"],
               dWn=npa(G["edge_to_node.weight"]), dbn=npa(G["edge_to_node.bias"]), dx=npa(dx),
               inv_deg=None, inv_cnt=None)
    assert np.array_equal(npa(enc.g_out), rec["g"])
    if aggr == "mean":
        rec["inv_deg"] = 1.0 / np.maximum(np.bincount(dst, minlength=N)[:N], 1)
    if pool == "mean":
        rec["inv_cnt"] = 1.0 / np.maximum(np.bincount(gid, minlength=c.B)[:c.B], 1)
    rows = []
    for (stage, got, st, extra), (_, _, st32, _) in zip(_encode_stages(rec, sw.REF),
                                                        _encode_stages(rec, TORCH_F32)):
        r, at = sw.rho(got, st)
        rr, _ = sw.rho(st32.ref, st)
        rows.append(dict(stage=stage, rho=r, rho_ref=rr, bar=sw.bar(rr) + extra, argmax=list(at),
                         rho_fp64=r))
        print(f"{name:>24s} {stage:<6s} rho {r:9.2f}  rho_ref {rr:7.2f}  bar {rows[-1]['bar']:7.2f}"
              f"  at {at}")
    write_report("encode_" + name, rows)
    bad = failures(rows)
    assert not bad, f"{name}:\n" + "\n".join(bad)


# ----------------------------------------------------------------------------------------------
# 6. heads
# ----------------------------------------------------------------------------------------------
def _heads(H):
    return {"linear_h_3": lambda: nn.Linear(H, 3),
            "mlp": lambda: nn.Sequential(nn.Linear(H, 16), nn.SiLU(), nn.Linear(16, 1)),
            "linear_no_bias": lambda: nn.Linear(H, 1, bias=False)}


@pytest.mark.parametrize("head", ["linear_h_3", "mlp", "linear_no_bias"])
def test_custom_heads_forward_and_gradients(head, cuda_device):
    H, D = 39, 2
    c = Case("ragged", H, D, "silu", True, "add", "mean", cuda_device)
    torch.manual_seed(5)
    c.m.ffn = _heads(H)[head]().to(cuda_device)
    c.data.x.requires_grad_(True)
    c.data.edge_attr.requires_grad_(True)
    y = c.m(c.data)
    assert tuple(y.shape) == ((c.B, 3) if head == "linear_h_3" else (c.B,))
    w = general_dg(c.B, 3, seed=9)  # the weights of the weighted-sum loss
    w = torch.from_numpy(w if y.dim() == 2 else np.ascontiguousarray(w[:, 0])).to(cuda_device)
    (w * y).sum().backward()
    torch.cuda.synchronize()
    # reference: the head in float64 on the oracle's g (torch autograd on the CPU)
    g_ref, cache = encode_forward(c.sd, c.b, D, "silu", True, "add", "mean")
    head64 = copy.deepcopy(c.m.ffn).cpu().double()
    g64 = torch.from_numpy(g_ref).requires_grad_(True)
    y64 = head64(g64).squeeze(-1)
    assert_y_close(y.detach().cpu().numpy().ravel(), y64.detach().numpy().ravel())
    (w.cpu().double() * y64).sum().backward()
    for (k, p), (_, q) in zip(c.m.ffn.named_parameters(), head64.named_parameters()):
        assert p.grad is not None and p.grad.shape == p.shape, k
        assert bool(torch.isfinite(p.grad).all()), k
        assert_g_close(p.grad.cpu().numpy(), q.grad.numpy(), "ffn." + k)
    gr, gin, skip_abs = encode_backward(c.sd, cache, g64.grad.numpy())
    for k, p in c.m.named_parameters():
        if not k.startswith("ffn."):
            assert_g_close(p.grad.cpu().numpy(), gr[k], k, skip_abs.get(k))
    assert_g_close(c.data.x.grad.cpu().numpy(), gin["x"], "dx")
    assert_g_close(c.data.edge_attr.grad.cpu().numpy(), gin["edge_attr"], "dedge_attr")


def test_default_head_stays_on_the_fused_path(cuda_device):
    c = Case("ragged", 39, 2, "silu", False, "add", "add", cuda_device)
    fused = c.run(False)
    lib = native.load()
    lib.cgr_profile_reset()
    lib.cgr_profile_enable(1)
    try:
        y = c.m(c.data)
        with torch.no_grad():
            y2 = c.m(c.data)
        torch.cuda.synchronize()
    finally:
        lib.cgr_profile_enable(0)
    classes = set(native.profile_report())
    lib.cgr_profile_reset()
    assert torch.equal(y.detach(), fused.y) and torch.equal(y2, fused.y)
    assert "pool_head_fwd" in classes
    assert "pool_only_fwd" not in classes and "readout_act_bwd_dg" not in classes


@pytest.mark.parametrize("case", golden_cases())
def test_head_on_fingerprint_matches_golden_predictions(case, cuda_device):
    z, meta = load_golden(case)
    m = model_from_golden(z, meta, cuda_device)
    m.eval()
    with torch.no_grad():
        y = m.ffn(m.encode(batch_from_golden(z, meta, cuda_device))).squeeze(-1)
    assert tuple(y.shape) == tuple(z["out_y_eval"].shape)
    assert_y_close(y.cpu().numpy(), z["out_y_eval"])


def test_pickled_module_still_encodes(cuda_device):
    c = Case("ragged", 39, 2, "silu", False, "add", "add", cuda_device)
    buf = io.BytesIO()
    pickle.dump(c.m, buf)
    m2 = pickle.loads(buf.getvalue())
    with torch.no_grad():
        assert torch.equal(m2.encode(c.data), c.m.encode(c.data))


# ----------------------------------------------------------------------------------------------
# 7. capture
# ----------------------------------------------------------------------------------------------
def test_captured_encode_head_adam_step_equals_eager(cuda_device):
    """encode -> Linear(H, 3) head -> loss -> backward -> FusedAdam.step(), captured: three
    replays equal three eager steps from the same state, parameters and fingerprints.  Both
    models start from the same seed and take the same two eager warm-up steps first (lazy
    streams, optimizer state), so the state at capture is the eager run's state."""
    H, D = 39, 2

    def fresh():
        c = Case("ragged", H, D, "silu", True, "add", "add", cuda_device)
        torch.manual_seed(5)
        c.m.ffn = nn.Linear(H, 3).to(cuda_device)
        params = list(c.m.parameters())
        return c, params, FusedAdam(params, lr=1e-3), torch.zeros(c.B, H, device=cuda_device)

    def step(c, params, opt, fp):
        g = c.m.encode(c.data)
        loss = ((c.m.ffn(g) - c.data.y[:, None]) ** 2).sum()
        for p, gr in zip(params, torch.autograd.grad(loss, params)):
            p.grad = gr
        opt.step()
        fp.copy_(g.detach())

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
        eager.append((a[3].clone(), [p.detach().clone() for p in a[1]]))
    torch.cuda.synchronize()

    b = fresh()
    warm(b)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(*b)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(b[3], eager[k][0]), k
        for p, q in zip(b[1], eager[k][1]):
            assert torch.equal(p.detach(), q), k


# ----------------------------------------------------------------------------------------------
# 8. refusals
# ----------------------------------------------------------------------------------------------
def _raw_backward(entry, run, up, params, grads, ws):
    """One backward entry point called directly on `run`'s arena (the refusal tests call the one
    that does not belong to it) -> return code."""
    from cgr_mpnn_3D._amd.functional import _param_table

    return entry(ctypes.byref(run.cfg), _param_table(params), ctypes.byref(run.bs), None,
                 ctypes.c_uint64(0), run.flags, native.ptr(run.arena), native.ptr(up),
                 _param_table(grads), native.ptr(ws), None, native.stream_ptr(up.device))


def _raw_input_grads(entry, run, up, params, ws, dx, de):
    from cgr_mpnn_3D._amd.functional import _param_table

    return entry(ctypes.byref(run.cfg), _param_table(params), ctypes.byref(run.bs),
                 native.ptr(run.arena), native.ptr(up), native.ptr(ws), native.ptr(dx),
                 native.ptr(de), native.stream_ptr(up.device))


def test_arena_kind_and_precision_refusals(cuda_device):
    """Every refusal returns an error code with its reason in cgr_last_error and enqueues
    nothing: sentinel-filled gradients, workspace and input-gradient buffers stay untouched."""
    c = Case("ragged", 39, 2, "silu", False, "add", "add", cuda_device)
    lib = native.load()
    dy = torch.from_numpy(mixed_dy(c.B)).to(cuda_device)
    dg = torch.from_numpy(general_dg(c.B, 39)).to(cuda_device)
    enc, fused = c.run(True), c.run(False)
    pf, pe = c.params(True), c.params(False)
    N, E = c.b.x.shape[0], c.b.edge_index.shape[1]
    nws = lib.cgr_gnn_workspace_bytes(ctypes.byref(enc.cfg), N, E, c.B)

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
    refused(_raw_backward(lib.cgr_gnn_backward, enc, dy, pf, bufs[1], bufs[0]),
            "cgr_gnn_backward: `arena` was filled by cgr_gnn_encode (headless", bufs)
    refused(_raw_backward(lib.cgr_gnn_encode_backward, fused, dg, pf, bufs[1], bufs[0]),
            "cgr_gnn_encode_backward: `arena` was filled by cgr_gnn_forward", bufs)
    # no backward was recorded either: the input gradients find none
    refused(_raw_input_grads(lib.cgr_gnn_encode_input_grads, enc, dg, pe, bufs[0], bufs[2],
                             bufs[3]),
            "does not hold a cgr_gnn_encode_backward", bufs)
    enc.backward(dg, pe)  # a real one, into enc.ws
    refused(_raw_input_grads(lib.cgr_gnn_input_grads, enc, dy, pf, enc.ws, bufs[2], bufs[3]),
            "cgr_gnn_input_grads: `arena` was filled by cgr_gnn_encode (headless", bufs)
    enc.cfg.precision = 1  # the arena's forward ran in the split-bf16 mode
    refused(_raw_backward(lib.cgr_gnn_encode_backward, enc, dg, pf, bufs[1], bufs[0]),
            "cgr_gnn_encode_backward: the config's precision differs", bufs)
    refused(_raw_input_grads(lib.cgr_gnn_encode_input_grads, enc, dg, pe, enc.ws, bufs[2],
                             bufs[3]),
            "cgr_gnn_encode_input_grads: the config's precision differs", bufs)


def test_encode_with_a_bucket_hook_raises_when_gradients_are_wanted(cuda_device):
    from cgr_mpnn_3D._amd import config

    c = Case("ragged", 39, 2, "silu", False, "add", "add", cuda_device)
    c.m._grad_bucket_hook = lambda flat, buckets, events: None
    with pytest.raises(NotImplementedError, match="gradient-bucket hook"):
        c.m.encode(c.data)
    with torch.no_grad():
        assert tuple(c.m.encode(c.data).shape) == (c.B, 39)
    c.m._grad_bucket_hook = None
    was = config.grad_bucket_hook
    config.grad_bucket_hook = lambda flat, buckets, events: None
    try:
        with pytest.raises(NotImplementedError, match="gradient-bucket hook"):
            c.m.encode(c.data)
    finally:
        config.grad_bucket_hook = was
    assert c.m.encode(c.data).requires_grad
