"""GPU: the arena and workspace contract of the GNN entry points (include/cgr_mpnn3d.h): the
contents of every caller-owned buffer on entry are arbitrary, and nothing outside the bytes the
library reports is written.

Every case runs forward, backward and input gradients once per fill (arena_contract_common.py:
0x00, 0xFF, and the bytes a finished run of a different case left behind; here also "twin": the
bytes a finished run of the same configuration and shape on another graph left behind, every
region's leftovers under the same region, as in captured, padded training), each run on fresh
Guarded buffers for everything the call writes -- arena, workspace, one flat gradient buffer viewed
per parameter as functional._function_backward views it, dx, de, the output -- and asserts

  * every output, gradient, named stage buffer ([:, :H]), named workspace buffer and bookkeeping
    array bit-identical across the fills (run-to-run determinism is pinned elsewhere, so the
    bar is equality);
  * every guard byte intact, every slack range (region end .. next 256-byte boundary; the flat
    gradient buffer's bucket padding) still holding its fill;
  * the status word's bits 1, 2 and 16 clear and no device error raised.

A production arena is a torch.empty: the caching allocator hands back whichever block was freed
last, so a kernel that reads what it never wrote sees another batch's values, and the stage tests'
second run sees the first run's correct ones.
"""

import ctypes

import numpy as np
import pytest
import torch

from arena_contract_common import (ALIGN, FILLS, Guarded, Outcome, byte_runs, check_fills,
                                   slack_ranges)
from stagewise_common import mask_batch, mixed_dy
from test_gpu_parity import ACT, _cfg_tuple, _hub_batch, _pool_fn, _shuffled_pairs, _sparse_batch

from cgr_mpnn_3D._amd import config, native
from cgr_mpnn_3D._amd.debug import ArenaRun, PredictRun, pack_images
from cgr_mpnn_3D._amd.functional import LEVEL_FUSED, LEVEL_NODES, LEVEL_POOLED, _grad_views
from cgr_mpnn_3D._amd.synth import RxnBatch, TorchBatch, make_batch
from cgr_mpnn_3D.models.GNN import GNN

pytestmark = pytest.mark.gpu

HUB = [150, 3, 70, 300, 5]
HUB_STALE = [5, 300, 3, 150, 70]  # the same N, E and layout, other crossing nodes
HUB128 = [130 + (37 * g) % 271 for g in range(48)]  # test_case07's list: >= 96 x 128 rows


def _tiny_batch():
    # the smallest legal batch: one bond, one graph (run with batch = None), F = 1, Fe = 0
    return RxnBatch(x=np.array([[0.75], [-1.5]], np.float32),
                    edge_index=np.array([[0, 1], [1, 0]], np.int64),
                    edge_attr=np.zeros((2, 0), np.float32), batch=np.zeros(2, np.int64),
                    ptr=np.array([0, 2], np.int64), y=np.zeros(1, np.float32))


def _tile_plus_one_batch():
    # N = 65, E = 66: one row past a 64-row tile both ways; a 34-atom chain in graph 0, graph 1's
    # 25 atoms unbonded; F = 5 (padded copy), Fe = 3
    rng = np.random.default_rng(651)
    ei = []
    for i in range(33):
        ei += [(i, i + 1), (i + 1, i)]
    return RxnBatch(x=rng.standard_normal((65, 5)).astype(np.float32),
                    edge_index=np.ascontiguousarray(np.array(ei, np.int64).T),
                    edge_attr=rng.standard_normal((66, 3)).astype(np.float32),
                    batch=np.repeat(np.arange(2), [40, 25]).astype(np.int64),
                    ptr=np.array([0, 40, 65], np.int64), y=np.zeros(2, np.float32))


def _twin_batch(b):
    """The same N, E, B and node ranges, another graph: the nodes of every graph in reverse
    order (a hub moves from its graph's first node to its last), x negated."""
    from dataclasses import replace

    new = np.concatenate([np.arange(lo, hi)[::-1] for lo, hi in zip(b.ptr[:-1], b.ptr[1:])])
    return replace(b, x=np.ascontiguousarray(-b.x[new]),
                   edge_index=np.ascontiguousarray(new[b.edge_index]))


def _wide_batch(n_mace, seed, graphs=7):
    return make_batch(graphs, 21, 23, n_mace=n_mace, seed=seed)


BATCHES = {
    "c02": lambda: make_batch(6, 14, 16, n_mace=7, seed=102),  # F 85: the xp padded copy
    "c03": lambda: make_batch(10, 24, 26, n_mace=2, seed=103),  # F 80: x read in place
    "c01": lambda: make_batch(12, n_atoms=30, n_bonds=34, n_mace=40, seed=101),
    "c04": lambda: make_batch(32, seed=104),
    "c05": lambda: make_batch(8, n_atoms=20, n_bonds=22, n_mace=16, seed=105),
    "c16": lambda: _sparse_batch(6, 40, seed=31),
    "c12": lambda: _wide_batch(40, 112),
    "c13": lambda: _wide_batch(7, 113),  # E 322: a 2-row last split
    "c14": lambda: _wide_batch(2, 114),
    "hub": lambda: _hub_batch(HUB, seed=41),
    "hub_stale": lambda: _hub_batch(HUB_STALE, seed=45),
    "hub128": lambda: _hub_batch(HUB128, seed=42),
    "c08": lambda: _shuffled_pairs(make_batch(8, n_atoms=30, n_bonds=30, n_mace=16, seed=28), 5),
    "c17": lambda: _shuffled_pairs(_wide_batch(2, 115, graphs=6), seed=5),
    "c09_mean": lambda: _sparse_batch(6, 40, seed=27),
    "c09_max": lambda: _sparse_batch(6, 40, seed=29),
    "m1": lambda: mask_batch("base"),
    "tiny": _tiny_batch,
    "n65": _tile_plus_one_batch,
    "stale": lambda: make_batch(5, 11, 13, n_mace=3, seed=77),  # the stale fills' donor
}

# name: (batch, H, D, act, skip, aggr, pool, dropout p, flags).  flags: "unpaired" the edge order
# is not reverse-paired (DEVERR_UNPAIRED_SEEN expected); "batch_none" one graph, batch = NULL;
# "hub" the stale bytes come from the HUB_STALE run of the same widths
CASES = {
    "c02_gelu_h37": ("c02", 37, 2, "gelu", True, "add", "add", 0.0, ()),
    "c02_gelu_h39": ("c02", 39, 2, "gelu", True, "add", "add", 0.0, ()),
    "c03_relu_h96": ("c03", 96, 3, "relu", False, "add", "add", 0.0, ()),
    "c05_silu_h528": ("c05", 528, 2, "silu", False, "add", "add", 0.0, ()),
    "c13_gelu_h515": ("c13", 515, 2, "gelu", True, "add", "add", 0.0, ()),
    "c14_relu_h521": ("c14", 521, 3, "relu", False, "add", "add", 0.0, ()),
    "c06_hub_h64": ("hub", 64, 3, "relu", True, "add", "add", 0.0, ("hub",)),
    "c07_hub128_h48": ("hub128", 48, 2, "relu", True, "add", "add", 0.0, ()),
    "c08_unpaired_h64": ("c08", 64, 3, "gelu", True, "add", "add", 0.0, ("unpaired",)),
    "c17_unpaired_h560": ("c17", 560, 2, "gelu", True, "add", "add", 0.0, ("unpaired",)),
    "c09_mean_mean": ("c09_mean", 64, 2, "silu", True, "mean", "mean", 0.0, ()),
    "c09_max_pool": ("c09_max", 64, 2, "silu", False, "add", "max", 0.0, ()),
    "m1_dropout_sigmoid": ("m1", 64, 3, "sigmoid", True, "add", "add", 0.5, ()),
    "tiny_n2_e2_h4": ("tiny", 4, 1, "silu", False, "add", "add", 0.0, ("batch_none",)),
    "n65_e66_h12": ("n65", 12, 2, "silu", True, "add", "add", 0.0, ()),
    # beyond the list above, from the same suite: F = 118 / H = 128 with every pre stored; cfg2's
    # widths (F = 846, H = 400, D = 4); tnr<5, 5> at H = 1000; hub segments over three column
    # tiles at H = 520; dropout in the unfused forward with scale_rows (mean / mean, H = 516)
    "c01_silu_h128": ("c01", 128, 3, "silu", True, "add", "add", 0.0, ()),
    "c04_cfg2_32": ("c04", 400, 4, "relu", False, "add", "add", 0.0, ()),
    "c12_silu_h1000": ("c12", 1000, 2, "silu", True, "add", "add", 0.0, ()),
    "c15_hub_h520": ("hub", 520, 2, "relu", True, "add", "add", 0.0, ()),
    "c16_mean_h516_dropout": ("c16", 516, 2, "silu", True, "mean", "mean", 0.02, ()),
}
LEVEL_CASES = ("c02_gelu_h39", "c06_hub_h64", "c09_max_pool")
FP32_CASES = ("c02_gelu_h39", "c06_hub_h64", "c05_silu_h528")
# name: (batch, H, D, act, skip, pool)
PREDICT_CASES = {
    "h39": ("c02", 39, 2, "gelu", True, "add"),
    "hub_h64": ("hub", 64, 3, "relu", True, "add"),
    "h1000_d4_rings": ("c12", 1000, 4, "silu", True, "add"),
}
LEVELS = {"fused": LEVEL_FUSED, "pooled": LEVEL_POOLED, "nodes": LEVEL_NODES}
DROP_SEED = 2**40 + 1234567


class Spec:
    """One case on the device: batch, config tuple, parameters, upstream gradient."""

    def __init__(self, batch, H, D, act, skip, aggr, pool, p_drop, flags, level, dev, scale=1.0,
                 precision=None, twin=False):
        self.args = (batch, H, D, act, skip, aggr, pool, p_drop, flags, level, dev)
        b = BATCHES[batch]()
        if twin:
            b = _twin_batch(b)
        self.F, self.Fe = b.x.shape[1], b.edge_attr.shape[1]
        self.N, self.E = b.x.shape[0], b.edge_index.shape[1]
        self.H, self.D, self.level, self.dev, self.flags = H, D, level, dev, flags
        torch.manual_seed(11)
        m = GNN(self.F, self.Fe, depth=D, hidden_sizes=[H] * D, dropout_ps=[p_drop] * D,
                activation_fn=ACT[act], use_learnable_skip=skip, aggr=aggr,
                pooling_fn=_pool_fn(pool))
        if skip:
            with torch.no_grad():
                for i, w in enumerate(m.skip_weights):
                    w.fill_(0.5 + 0.25 * i)
        m = m.to(dev)
        self.full_params = [(q.detach() * scale).contiguous() for q in m.native_parameters()]
        # below the fused level: None in the ffn slots
        self.params = [None if q is None else p for q, p in
                       zip(m.native_parameters(level == LEVEL_FUSED), self.full_params)]
        d = b.to_torch(dev)
        d.edge_index = d.edge_index.contiguous()
        if "batch_none" in flags:
            d = TorchBatch(d.x, d.edge_index, d.edge_attr, None, None, d.y)
        self.data, self.B = d, 1 if "batch_none" in flags else b.num_graphs
        self.cfg_t = _cfg_tuple(self.F, self.Fe, H, D, act, skip, aggr, pool)
        if precision is not None:
            self.cfg_t = self.cfg_t + (precision,)
        self.pool = pool
        self.training = p_drop > 0
        self.dps = [p_drop] * D if self.training else None
        rows = {LEVEL_FUSED: None, LEVEL_POOLED: self.B, LEVEL_NODES: self.N}[level]
        if rows is None:
            up = mixed_dy(self.B)
        else:  # a general dg / dn: seeded normals over three decades, as mixed_dy's
            rng = np.random.default_rng(20262 + level)
            up = (rng.standard_normal((rows, H)) *
                  10.0 ** rng.uniform(-2.0, 1.0, (rows, 1))).astype(np.float32)
        self.up = torch.from_numpy(up).to(dev)
        self.out_shape = (self.B,) if rows is None else (rows, H)
        self.geo, _, self.grad_floats = _grad_views(self.params, D)

    def run(self, bufs=None):
        """forward, backward, input gradients; bufs: {name: Guarded} (None: plain torch.empty)
        -> (ArenaRun, grads, dx, de, out)."""
        d, p = self.data, self.params
        kw, bkw, ikw, out, flat = {}, {}, {}, None, None
        if bufs is not None:
            out = bufs["out"].floats(*self.out_shape)
            kw = dict(arena=bufs["arena"].payload,
                      **{("y", "g_out", "n_out")[self.level]: out})
            flat = bufs["grads"].floats(self.grad_floats)
            ikw = dict(dx=bufs["dx"].floats(self.N, self.F),
                       de=bufs["de"].floats(self.E, self.Fe) if self.Fe else None)
        else:
            flat = torch.empty(self.grad_floats, dtype=torch.float32, device=self.dev)
        # one flat gradient buffer viewed per parameter, as functional._function_backward's
        grads = [None if q is None else flat[o:o + int(np.prod(s, dtype=np.int64))].view(s)
                 for q, (s, _, o) in zip(p, self.geo)]
        if bufs is not None:
            bkw = dict(ws=bufs["ws"].payload)
        run = ArenaRun(self.cfg_t, d.x, d.edge_index, d.edge_attr, d.batch, d.ptr, self.B, p,
                       dropout_ps=self.dps, seed=DROP_SEED, training=self.training,
                       encode=self.level == LEVEL_POOLED, nodes=self.level == LEVEL_NODES, **kw)
        run.backward(self.up, p, grads=grads, **bkw)
        dx, de = run.input_grads(self.up, p, run.ws, **ikw)
        torch.cuda.synchronize()
        out = (run.y, run.g_out if run.encode else None, run.n_out if run.nodes else None)[
            self.level]
        return run, grads, dx, de, out

    def sizes(self):
        lib, c = native.load(), ctypes.byref(_config_of(self.cfg_t))
        return (lib.cgr_gnn_arena_bytes(c, self.N, self.E, self.B),
                lib.cgr_gnn_workspace_bytes(c, self.N, self.E, self.B))

    def grad_gaps(self):
        """Byte ranges of the flat gradient buffer that no parameter's view covers (the buckets'
        16-byte padding): they keep the fill."""
        used = np.zeros(4 * self.grad_floats, bool)
        for q, (s, _, o) in zip(self.params, self.geo):
            if q is not None:
                used[4 * o:4 * (o + int(np.prod(s, dtype=np.int64)))] = True
        return [("bucket padding", lo, hi) for lo, hi in byte_runs(~used)]


def _config_of(cfg_t):
    from cgr_mpnn_3D._amd.functional import make_config

    return make_config(*cfg_t)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _record(spec, run, grads, dx, de, out):
    """Everything the three calls computed, as numpy: the outputs, every gradient, the logical
    region of every named stage and workspace buffer, the bookkeeping arrays."""
    N, E, B, D = spec.N, spec.E, spec.B, spec.D
    cfg = run.cfg
    relu = cfg.activation == native.ACT_RELU
    rec = {"out": _np(out), "dx": _np(dx), "de": None if de is None else _np(de),
           "grads": [None if g is None else _np(g) for g in grads]}
    for k, n in (("perm", E), ("src_s", E), ("dst_s", E), ("rev_s", E), ("src_list", E),
                 ("dst_ptr", N + 1), ("src_ptr", N + 1), ("graph_ptr", B + 1), ("node_graph", N),
                 ("status", 1)):
        rec[k] = _np(run.ints(k, n))
    if spec.training:
        rec["rng"] = _np(run.uint64("rng"))
    if spec.Fe:
        rec["e_s"] = _np(run.floats("e_s", E, cols=(spec.Fe + 3) // 4 * 4))[:, :spec.Fe]
    rec["P"], rec["Q"] = _np(run.floats("P", N)), _np(run.floats("Q", N))
    rec["h"] = [_np(run.floats("h", E, index=l)) for l in range(D + 1)]
    rec["a"] = [_np(run.floats("a", N, index=l)) for l in range(D + 1)]
    if not relu:
        rec["pre"] = [_np(run.floats("pre", E, index=l)) for l in range(D + 1)]
        rec["zn"] = _np(run.floats("zn", N))
    rec["hn"] = _np(run.floats("hn", N))
    if spec.level != LEVEL_NODES:  # the nodes level pools nothing
        rec["g"] = _np(run.floats("g", B))
    rec["ds"] = _np(run.ws_floats("ds", N))
    rec["dpre"] = [_np(run.ws_floats("dpre", E, index=l)) for l in range(D)]
    rec["dpre0"] = _np(run.ws_floats("dpre0", E))
    # dzn in fp32: below the fused level, and under max pooling (cgr_gnn_workspace_offset)
    if spec.level != LEVEL_FUSED or spec.pool == "max":
        rec["dzn_main"] = _np(run.ws_floats("dzn_main", N))
    return rec


_DONORS = {}
TWIN = "twin"  # a fourth fill: see _twin_bytes
ALL_FILLS = FILLS + (TWIN,)


def _finished_bytes(s, dev):
    """What a finished run of `s` at the fused level (training calls, predict, packed images) left
    in its buffers, by buffer name, as host bytes."""
    run, grads, dx, de, out = s.run()
    d = s.data
    pred = PredictRun(s.cfg_t, d.x, d.edge_index, d.edge_attr, d.batch, d.ptr, s.B, s.params)
    images = pack_images(s.cfg_t, s.params, dev)
    torch.cuda.synchronize()
    native.raise_device_errors(dev)
    flat = np.concatenate([_np(g).reshape(-1) for g in grads])
    return {"arena": _np(run.arena), "ws": _np(run.ws), "grads": flat, "dx": _np(dx),
            "de": np.zeros(1, np.float32) if de is None else _np(de), "out": _np(out),
            "predict": _np(pred.arena), "images": _np(images)}


def _donor(kind, dev):
    """The stale fills' bytes: a finished run of a different case -- another graph, other widths
    (the hub donor: the same widths, other crossing nodes), parameters scaled by -64 so its
    values are large."""
    if kind not in _DONORS:
        if kind == "hub":
            s = Spec("hub_stale", 64, 3, "relu", True, "add", "add", 0.0, (), LEVEL_FUSED, dev,
                     scale=-64.0)
        else:
            s = Spec("stale", 44, 2, "silu", True, "mean", "max", 0.0, (), LEVEL_FUSED, dev,
                     scale=-64.0)
        _DONORS[kind] = _finished_bytes(s, dev)
    return _DONORS[kind]


def _twin_bytes(spec, dev):
    """The twin fill's bytes: a finished run of the case's own configuration and shape -- so of
    its exact layout, every region's leftovers under the same region -- on another graph
    (_twin_batch) with x negated and the parameters scaled by -64: what a step of captured,
    padded training finds in a buffer of the step before."""
    if getattr(spec, "_twin", None) is None:
        a = spec.args
        spec._twin = _finished_bytes(Spec(*a[:9], LEVEL_FUSED, dev, scale=-64.0, twin=True), dev)
    return spec._twin


def _fill(spec, fill, name, dev):
    if fill == TWIN:
        return _twin_bytes(spec, dev)[name]
    if fill != "stale":
        return fill
    return _donor("hub" if "hub" in spec.flags else "general", dev)[name]


def _contract(name, spec, dev):
    arena_bytes, ws_bytes = spec.sizes()
    slack_n = [0]

    def runner(fill):
        sizes = {"arena": arena_bytes, "ws": ws_bytes, "grads": 4 * spec.grad_floats,
                 "dx": 4 * spec.N * spec.F, "de": 4 * spec.E * spec.Fe,
                 "out": 4 * int(np.prod(spec.out_shape))}
        bufs = {k: Guarded(n, _fill(spec, fill, k, dev), dev) for k, n in sizes.items()
                if n or k != "de"}
        run, grads, dx, de, out = spec.run(bufs)
        assert run.arena.data_ptr() == bufs["arena"].payload.data_ptr()
        assert run.ws.data_ptr() == bufs["ws"].payload.data_ptr()
        assert out.data_ptr() == bufs["out"].payload.data_ptr()
        bits = native.raise_device_errors(dev)  # raises on a completion timeout
        assert bool(bits & native.DEVERR_UNPAIRED_SEEN) == ("unpaired" in spec.flags), bits
        slack = slack_ranges(run)
        slack["grads"] = spec.grad_gaps()
        if spec.level == LEVEL_NODES:  # no pool, its state untouched: g keeps the fill
            slack["arena"].append(("hn (in g itself, which the nodes level leaves alone)",
                                   run.offset("g"), run.offset("g") + 4 * spec.B * run.Hp))
        slack_n[0] = sum(len(v) for v in slack.values())
        rec = _record(spec, run, grads, dx, de, out)
        status = int(rec["status"][0])
        assert status & (1 | 2 | 16) == 0, status
        assert bool(status & 4) == ("unpaired" in spec.flags), status
        return Outcome(bufs, rec, slack)

    check_fills(runner, ALL_FILLS, what=name)
    print(f"{name}: arena {arena_bytes} B, workspace {ws_bytes} B, {slack_n[0]} slack ranges")


@pytest.mark.parametrize("prep_split", [None, "1"], ids=["prep_fused", "prep_split"])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_level_fill_independence(name, prep_split, cuda_device, monkeypatch):
    # both forms of the forward's start: the x-GEMM launch's side workgroup, graph_prep.hip's
    # launches (CGR_PREP_SPLIT is read per call)
    if prep_split is None:
        monkeypatch.delenv("CGR_PREP_SPLIT", raising=False)
    else:
        monkeypatch.setenv("CGR_PREP_SPLIT", prep_split)
    _contract(f"{name}/{'split' if prep_split else 'fused'}",
              Spec(*CASES[name], LEVEL_FUSED, cuda_device), cuda_device)


@pytest.mark.parametrize("level", ["pooled", "nodes"])
@pytest.mark.parametrize("name", LEVEL_CASES)
def test_pooled_and_nodes_levels_fill_independence(name, level, cuda_device):
    # a general dg / dn; dzn_main among the compared buffers; nodes under max pooling: the arena
    # has a pool_arg region that no kernel of this level writes
    _contract(f"{name}/{level}", Spec(*CASES[name], LEVELS[level], cuda_device), cuda_device)


@pytest.mark.parametrize("name", FP32_CASES)
def test_fp32_mode_fill_independence(name, cuda_device):
    was = config.precision
    config.precision = "fp32"  # the process switch, as tests/test_gpu_precision.py sets it
    try:
        spec = Spec(*CASES[name], LEVEL_FUSED, cuda_device)
        assert _config_of(spec.cfg_t).precision == native.PRECISION_FP32
        _contract(f"{name}/fp32", spec, cuda_device)
    finally:
        config.precision = was


@pytest.mark.parametrize("packed", [False, True], ids=["own_images", "packed_images"])
@pytest.mark.parametrize("level", list(LEVELS))
@pytest.mark.parametrize("name", list(PREDICT_CASES))
def test_predict_fill_independence(name, level, packed, cuda_device):
    """The forward-only entries on a Guarded predict arena (h on a two-buffer ring, a on a
    three-buffer one), with the call's own weight images and with a Guarded images buffer that
    cgr_gnn_pack_images filled: y bit-identical across the arena's fills and equal to the training
    forward of the same inputs; the packed images' bytes equal across the images buffer's fills."""
    dev = cuda_device
    batch, H, D, act, skip, pool = PREDICT_CASES[name]
    spec = Spec(batch, H, D, act, skip, "add", pool, 0.0, ("hub",) if batch == "hub" else (),
                LEVELS[level], dev)
    d, lib, cfg = spec.data, native.load(), _config_of(spec.cfg_t)
    nbytes = lib.cgr_gnn_predict_arena_bytes(ctypes.byref(cfg), spec.N, spec.E, spec.B)
    ibytes = lib.cgr_gnn_image_bytes(ctypes.byref(cfg))
    assert nbytes > 0 and ibytes > 0
    train = ArenaRun(spec.cfg_t, d.x, d.edge_index, d.edge_attr, d.batch, d.ptr, spec.B,
                     spec.params, encode=level == "pooled", nodes=level == "nodes",
                     prepare_backward=False)
    torch.cuda.synchronize()
    y_train = _np((train.y, train.g_out if train.encode else None,
                   train.n_out if train.nodes else None)[spec.level])

    def runner(fill):
        bufs = {"arena": Guarded(nbytes, _fill(spec, fill, "predict", dev), dev),
                "out": Guarded(4 * int(np.prod(spec.out_shape)), _fill(spec, fill, "out", dev),
                               dev)}
        rec = {}
        images = None
        if packed:
            bufs["images"] = Guarded(ibytes, _fill(spec, fill, "images", dev), dev)
            # (cgr_gnn_pack_images takes the whole parameter table, whatever the level)
            images = pack_images(spec.cfg_t, spec.full_params, dev, bufs["images"].payload)
        run = PredictRun(spec.cfg_t, d.x, d.edge_index, d.edge_attr, d.batch, d.ptr, spec.B,
                         spec.params, level=spec.level, arena=bufs["arena"].payload,
                         images=images, y=bufs["out"].floats(*spec.out_shape))
        torch.cuda.synchronize()
        native.raise_device_errors(dev)
        assert run.status() & (1 | 2 | 16) == 0
        rec["y"] = _np(run.y)
        return Outcome(bufs, rec)

    outs = check_fills(runner, ALL_FILLS, what=f"predict {name}/{level}")
    assert outs["zero"].record["y"].tobytes() == y_train.tobytes(), \
        "predict differs from the training forward"
    if packed:
        # the images buffer has no offset query: what no fill changes is nobody's only where it
        # is the layout's rounding (under 256 bytes, up to a 256-byte boundary or the end);
        # everything else is bit-identical across the buffer's fills
        img = {f: o.buffers["images"] for f, o in outs.items()}
        free = np.ones(ibytes, bool)
        for g in img.values():
            free &= g.bytes() == g.fill
        bad = [(lo, hi) for lo, hi in byte_runs(free)
               if hi - lo >= ALIGN or (hi % ALIGN and hi != ibytes)]
        assert not bad, f"packed images: bytes left unwritten inside an image: {bad[:4]}"
        for f in ALL_FILLS[1:]:
            diff = np.flatnonzero((img["zero"].bytes() != img[f].bytes()) & ~free)
            assert diff.size == 0, f"packed images differ (zero vs {f} fill) at {diff[:4]}"
