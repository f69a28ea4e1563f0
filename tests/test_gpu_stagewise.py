"""GPU: every kernel stage of the forward and the backward, element by element, against a float64
evaluation of that one stage from the GPU's own inputs to it (oracle/stagewise.py).

tests/test_gpu_parity.py judges the two ends of the model at 1e-4 of a tensor's maximum; an error
of one kernel in one element (an edge missing from one segment sum, a row that lost its low bf16
pieces, a split-K slab left out of one tile) is diluted below that by the pooling and the
products behind it (tests/test_stagewise_refs.py shows one that passes).  Here each stage's
saved output (the arena's P, Q, pre, h, a, zn, hn, g; the backward workspace's ds, dpre, dpre0;
the gradients) is compared with the stage recomputed in float64 from the saved outputs of the
stages before it, the error of each element scaled by u x that element's sum of |terms|:

    rho = max (|got - ref| - T)+ / (u S)  <=  max(8, 4 rho_ref)  (+ the split's worst case for
                                                                   two weight gradients)

rho_ref is torch fp32 on the CPU for the same stage from the same inputs; T the activation
allowance u (8 + |z|)(1 + |z|) (x |upstream gradient| for a derivative).  DESIGN.md §2 derives
the bars and records the measured rho per stage (stage_errors.json of this file's run).

Every case also asserts that a second run on the same inputs reproduces every stage buffer bit
for bit -- the judged run on an arena, workspace and gradient buffer that start from 0xFF bytes
(NaN floats, -1 ints), the second from 0x00, both between guards (arena_contract_common.py), so
the equality is also independence of what the buffers held on entry -- and which
weight-gradient kernel family (split-bf16 e-image TN, the register-direct fp32 TN or the
LDS-staged fp32 TN) produced each class of gradients, from the library's per-class profile of a
third run.
"""

import numpy as np
import pytest
import torch

from arena_contract_common import guarded_run_buffers
from conftest import ACT_NAMES
from stagewise_common import (TORCH_F32, failures, mixed_dy, model_masks, param_names,
                              write_report)
from test_gpu_parity import ACT, _cfg_tuple, _hub_batch, _pool_fn, _shuffled_pairs, _sparse_batch

from cgr_mpnn_3D._amd import native
from cgr_mpnn_3D._amd.debug import ArenaRun
from cgr_mpnn_3D._amd.synth import make_batch
from cgr_mpnn_3D.models.GNN import GNN
from oracle import dropout as od
from oracle import stagewise as sw

pytestmark = pytest.mark.gpu

DY_SEED = 20261  # the one seed of every case's dy (stagewise_common.mixed_dy)
DROP_SEED = 1234567  # the dropout seed of the cases that name none
TN_CLASSES = {"readout": "gemm_tn_wgrad_readout", "layer": "gemm_tn_wgrad_layer",
              "node": "gemm_tn_wgrad_node"}


def _np(t):
    return t.detach().cpu().numpy().copy()


def _run_once(cfg_t, data, B, params, dy, dropout_ps, training, inputs, drop_seed=DROP_SEED,
              fill=None):
    """fill: "ones" / "zero": arena, workspace and gradient buffer are guarded caller buffers
    that start from that byte (arena_contract_common.py; 0xFF: every float NaN, every int -1);
    None: torch.empty ones."""
    bufs, grads = {}, None
    if fill is not None:
        bufs, grads = guarded_run_buffers(cfg_t, data.x.shape[0], data.edge_index.shape[1], B,
                                          params, fill, data.x.device)
    run = ArenaRun(cfg_t, data.x, data.edge_index, data.edge_attr, data.batch, data.ptr, B, params,
                   dropout_ps=dropout_ps, seed=drop_seed, training=training, prepare_backward=True,
                   arena=bufs["arena"].payload if bufs else None)
    assert run.bs.x == data.x.data_ptr()  # the x pointer the library is handed
    grads = run.backward(dy, params, ws=bufs["ws"].payload if bufs else None, grads=grads)
    gin = run.input_grads(dy, params, run.ws) if inputs else (None, None)
    torch.cuda.synchronize()
    for k, g in bufs.items():
        g.check_guards(k)
    return run, grads, gin


def _read(run, grads, gin, names, cfg, N, E, B):
    """Every stage buffer of a finished run, once, as numpy (edge rows in sorted order)."""
    D, relu = cfg["D"], cfg["act"] == "relu"
    rec = dict(B=B, pool_arg=None, inv_deg=None, inv_cnt=None)
    for k, n in (("perm", E), ("src_s", E), ("dst_s", E), ("rev_s", E), ("node_graph", N)):
        rec[k] = _np(run.ints(k, n)).astype(np.int64)
    Fep = (cfg["Fe"] + 3) // 4 * 4
    es = _np(run.floats("e_s", E, cols=Fep)) if cfg["Fe"] else np.zeros((E, 0), np.float32)
    assert not es[:, cfg["Fe"]:].any(), "e_s pad columns (read by the edge-feature TN) not zero"
    rec["e_s"] = es[:, :cfg["Fe"]]
    rec["P"], rec["Q"] = _np(run.floats("P", N)), _np(run.floats("Q", N))
    rec["h"] = [_np(run.floats("h", E, index=l)) for l in range(D + 1)]
    rec["a"] = [_np(run.floats("a", N, index=l)) for l in range(D + 1)]
    rec["pre"] = [None if relu else _np(run.floats("pre", E, index=l)) for l in range(D + 1)]
    rec["zn"] = None if relu else _np(run.floats("zn", N))
    rec["hn"], rec["g"], rec["y"] = _np(run.floats("hn", N)), _np(run.floats("g", B)), _np(run.y)
    rec["ds"] = _np(run.ws_floats("ds", N))
    rec["dpre"] = [_np(run.ws_floats("dpre", E, index=l)) for l in range(D)]
    rec["dpre0"] = _np(run.ws_floats("dpre0", E))
    rec["grads"] = {k: _np(g) for k, g in zip(names, grads)}
    rec["dx"] = None if gin[0] is None else _np(gin[0])
    rec["de"] = None if gin[1] is None else _np(gin[1])
    rec["key"] = run.rng_key() if run.training else None  # the dropout key the forward wrote
    return rec


def _flat(rec):
    for k, v in rec.items():
        if isinstance(v, np.ndarray):
            yield k, v
        elif isinstance(v, list):
            for i, t in enumerate(v):
                if t is not None:
                    yield f"{k}[{i}]", t
        elif isinstance(v, dict):
            yield from ((f"{k}.{n}", t) for n, t in v.items())


def _tn_families(cfg_t, data, B, params, dy, dropout_ps, training, drop_seed=DROP_SEED):
    """{"readout" | "layer" | "node": "b3" | "tnr" | "f32"} from the per-class profile of one run:
    the split-bf16 e-image TN (plain class name), the register-direct fp32 TN ("[tnr]") or the
    LDS-staged fp32 TN ("[f32]")."""
    lib = native.load()
    lib.cgr_profile_reset()
    lib.cgr_profile_enable(1)
    try:
        _run_once(cfg_t, data, B, params, dy, dropout_ps, training, False, drop_seed)
    finally:
        lib.cgr_profile_enable(0)
    classes = set(native.profile_report())
    lib.cgr_profile_reset()
    fam = {}
    for k, c in TN_CLASSES.items():
        forms = [s for s in ("", "[tnr]", "[f32]") if c + s in classes]
        assert len(forms) == 1, (c, sorted(classes))
        fam[k] = {"": "b3", "[tnr]": "tnr", "[f32]": "f32"}[forms[0]]
    return fam, classes


def _stagewise(case, b, H, D, act, skip, dev, *, inputs=False, aggr="add", pool="add", p_drop=0.0,
               x_row_scales=None, expect_tn=None, seed=0, mask="recovered", drop_seed=DROP_SEED,
               x_offset=0):
    """x_offset: x handed to the library as a contiguous view that many floats into a larger
    device buffer (pointer % 16 == 4 * x_offset).
    mask: where the oracle's dropout masks come from.  "recovered": h != 0 of the GPU's own
    output (checked against the host model's mask wherever the activation is not itself 0);
    "model": oracle/dropout.py's keep_mask alone (sigmoid, so h == 0 exactly where dropped)."""
    F_, Fe = b.x.shape[1], b.edge_attr.shape[1]
    torch.manual_seed(seed)
    m = GNN(F_, Fe, depth=D, hidden_sizes=[H] * D, dropout_ps=[p_drop] * D,
            activation_fn=ACT[act], use_learnable_skip=skip, aggr=aggr, pooling_fn=_pool_fn(pool))
    if skip:  # non-trivial skip weights, as test_gpu_parity._oracle_compare sets them
        with torch.no_grad():
            for i, w in enumerate(m.skip_weights):
                w.fill_(0.5 + 0.25 * i)
    m = m.to(dev)
    params = [q.detach().contiguous() for q in m.native_parameters()]
    names = param_names(D, skip)
    assert len(names) == len(params)
    sd = {k: _np(q) for k, q in zip(names, params)}
    x = b.x
    if x_row_scales is not None:  # node rows scaled, cycling: pre0 and zn span several decades
        x = (x * np.asarray(x_row_scales, np.float32)[np.arange(x.shape[0]) % len(x_row_scales),
                                                      None]).astype(np.float32)
    data = b.to_torch(dev)
    data.x = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if x_offset:
        buf = torch.zeros(x.size + 4, dtype=torch.float32, device=dev)
        view = buf[x_offset:x_offset + x.size].view(x.shape)
        data.x = view.copy_(data.x)
        assert data.x.is_contiguous() and data.x.data_ptr() % 16 == 4 * x_offset
    N, E, B = x.shape[0], b.edge_index.shape[1], b.num_graphs
    cfg_t = _cfg_tuple(F_, Fe, H, D, act, skip, aggr, pool)
    cfg = dict(F=F_, Fe=Fe, H=H, D=D, act=act, skip=skip, aggr=aggr, pool=pool, batched=True)
    dy = torch.from_numpy(mixed_dy(B, DY_SEED)).to(dev)
    training = p_drop > 0
    dps = [p_drop] * D if training else None

    # the run the oracle judges starts from 0xFF in its arena, workspace and gradient buffer (NaN
    # floats, -1 ints), the second from 0x00: bit-for-bit equality of the two is then also
    # independence of what the buffers held on entry
    rec = _read(*_run_once(cfg_t, data, B, params, dy, dps, training, inputs, drop_seed, "ones"),
                names, cfg, N, E, B)
    rec2 = _read(*_run_once(cfg_t, data, B, params, dy, dps, training, inputs, drop_seed, "zero"),
                 names, cfg, N, E, B)
    for (k, v), (_, v2) in zip(_flat(rec), _flat(rec2)):
        assert v.tobytes() == v2.tobytes(), f"{case}: {k} differs between two runs"
    fam, classes = _tn_families(cfg_t, data, B, params, dy, dps, training, drop_seed)
    if expect_tn is not None:
        assert fam == expect_tn, (fam, sorted(classes))
    # the oracle judges two arithmetics: split-bf16, and fp32 (both fp32 kernel families)
    rec["tn"] = {k: "b3" if f == "b3" else "f32" for k, f in fam.items()}

    rec["x"], rec["dy"] = x, _np(dy)
    deg = np.bincount(rec["dst_s"], minlength=N)[:N]
    assert np.array_equal(rec["dst_s"], np.sort(rec["dst_s"]))
    if aggr == "mean":
        rec["inv_deg"] = 1.0 / np.maximum(deg, 1)
    if pool == "mean":
        rec["inv_cnt"] = 1.0 / np.maximum(np.bincount(rec["node_graph"], minlength=B)[:B], 1)
    rec["keep"] = [None] * D
    model = [None] * D
    if training:
        assert act != "relu" and mask in ("recovered", "model")
        assert rec["key"] == od.forward_key(drop_seed)  # no device counter: the key is the seed
        model = model_masks(rec["key"], E, H, dps)
        for l in range(D):
            kept, pre = rec["h"][l + 1] != 0, rec["pre"][l + 1]
            if mask == "model":  # the host model's mask, in the record's (dst-sorted) row order
                assert act == "sigmoid" and np.isfinite(pre).all() and np.abs(pre).max() < 80
                scale = float(od.thresh_scale(p_drop)[1])  # the kernels' float32; 0 at p >= 1
                model[l] = model[l] & (scale > 0)
                assert np.array_equal(kept, model[l]), _first_diff(case, l, kept, model[l])
                rec["keep"][l] = model[l] * scale
                continue
            # the GPU's own dropout mask, as test_dropout_matches_oracle_with_recovered_mask
            live = np.abs(pre) > 1e-3
            assert abs((1.0 - kept[live].mean()) - p_drop) < 0.01
            rec["keep"][l] = kept / (1.0 - p_drop)
            # ... which is the model's wherever act(pre) is not itself 0 (pre 0, or far below 0)
            assert not (kept & ~model[l]).any(), _first_diff(case, l, kept, model[l])
            act_nonzero = (pre != 0) & (pre > -80)
            assert np.array_equal(kept[act_nonzero], model[l][act_nonzero]), \
                _first_diff(case, l, kept, model[l])
    rows = sw.judge(rec, sd, cfg, TORCH_F32)
    for l in range(D):  # the backward regenerates the mask: dpre exactly 0 where the model drops
        if model[l] is not None:
            bad = (rec["dpre"][l] != 0) & ~model[l]
            assert not bad.any(), f"{case}: dpre.{l} nonzero at dropped {np.argwhere(bad)[0]}"
    write_report(case, rows)
    for r in rows:
        print(f"{case:>14s} {r['stage']:<26s} rho {r['rho']:9.2f}  rho_ref {r['rho_ref']:7.2f}  "
              f"bar {r['bar']:7.2f}  fp64 {r['rho_fp64']:9.2f}  at {r['argmax']}")
    bad = failures(rows)
    assert not bad, f"{case}:\n" + "\n".join(bad)
    return rec


def _first_diff(case, l, kept, model):
    d = np.argwhere(kept != model)
    return f"{case}: layer {l} mask differs from the model at {len(d)} elements, first {d[:1]}"


B3 = dict(readout="b3", layer="b3", node="b3")
F32 = dict(readout="f32", layer="f32", node="f32")
TNR = dict(readout="tnr", layer="tnr", node="tnr")


def test_case01_every_stage_with_stored_pre(cuda_device):
    # F = 118 (padded x rows, Fp = 120), H = 128: x-GEMM over padded x, fused edge init + a_0,
    # 64-row tiles of the fused layer forward / backward, every weight gradient on the split-bf16
    # e-image TN; SiLU stores every pre-activation; input gradients
    b = make_batch(12, n_atoms=30, n_bonds=34, n_mace=40, seed=101)
    _stagewise("c01_silu_h128", b, 128, 3, "silu", True, cuda_device, inputs=True, expect_tn=B3)


def test_case02_odd_widths(cuda_device):
    # F = 85 (odd), H = 37 (Hp = 40): masked loaders, padded rows, 3 column fragments
    b = make_batch(6, 14, 16, n_mace=7, seed=102)
    _stagewise("c02_gelu_h37", b, 37, 2, "gelu", True, cuda_device, inputs=True, expect_tn=B3)


def test_case02_width_3_mod_4(cuda_device):
    # H = 39 (Hp = 40): the merged x-GEMM's last float4 column group of a Q row starts at column
    # Hp - 3; its fourth element belongs to no row (EpSplit2: it used to land on the next row's
    # Q[., 0], racing that row's own store across two 64-row tiles)
    b = make_batch(6, 14, 16, n_mace=7, seed=102)
    assert b.x.shape[0] > 64
    _stagewise("c02_gelu_h39", b, 39, 2, "gelu", True, cuda_device, inputs=True, expect_tn=B3)


def test_case03_relu_unpadded_x(cuda_device):
    # F = 80: x read in place with 16-byte loads (no padded copy); ReLU: no stored pre, the
    # derivative from h > 0
    b = make_batch(10, 24, 26, n_mace=2, seed=103)
    assert b.x.shape[1] == 80
    _stagewise("c03_relu_h96", b, 96, 3, "relu", False, cuda_device, inputs=True, expect_tn=B3)


def test_case04_cfg2_widths(cuda_device):
    # F = 846, Fe = 14, H = 400, D = 4 on 32 reactions: cfg2's column tiling (25 fragments)
    _stagewise("c04_cfg2_32", make_batch(32, seed=104), 400, 4, "relu", False, cuda_device,
               expect_tn=B3)


def test_case05_wider_than_512(cuda_device):
    # H = 528 > 512: the unfused edge init / layer forward + segment_sum launches, every weight
    # gradient on an fp32 TN family (33 fragments do not fit the e-image TN): H % 4 == 0 puts the
    # layer on tnr<4, 4>, H % 5 != 0 the x-side two on the LDS-staged TN
    b = make_batch(8, n_atoms=20, n_bonds=22, n_mace=16, seed=105)
    _stagewise("c05_silu_h528", b, 528, 2, "silu", False, cuda_device, inputs=True,
               expect_tn=dict(layer="tnr", readout="f32", node="f32"))


@pytest.mark.parametrize("skip", [True, False])
def test_case06_hub_segments_64_row_tiles(skip, cuda_device):
    # hub in-degrees 150 / 70 / 300: dst segments over 3-6 row tiles of 64 rows (tickets, slots)
    b = _hub_batch([150, 3, 70, 300, 5], seed=41)
    _stagewise(f"c06_hub64_skip{int(skip)}", b, 64, 3, "relu", skip, cuda_device, expect_tn=B3)


def test_case07_hub_segments_128_row_tiles(cuda_device):
    b = _hub_batch([130 + (37 * g) % 271 for g in range(48)], seed=42)
    assert b.edge_index.shape[1] >= 96 * 128  # >= 96 workgroups: 128-row tiles
    _stagewise("c07_hub128", b, 48, 2, "relu", True, cuda_device, expect_tn=B3)


def test_case08_unpaired_edge_order(cuda_device):
    # edges shuffled inside every graph (status 4): the layer backward's unpaired completion form,
    # at a size of a few row tiles
    u = _shuffled_pairs(make_batch(8, n_atoms=30, n_bonds=30, n_mace=16, seed=28), seed=5)
    _stagewise("c08_unpaired", u, 64, 3, "gelu", True, cuda_device, expect_tn=B3)
    torch.cuda.synchronize()
    bits = native.raise_device_errors(cuda_device)  # raises on a completion timeout
    assert bits & native.DEVERR_UNPAIRED_SEEN


def test_case09_mean_modes_with_isolated_nodes(cuda_device):
    # atoms mostly unbonded (in-degree 0: inv_deg = 1 / max(0, 1)), mean aggregation and pooling
    b = _sparse_batch(6, 40, seed=27)
    assert b.x.shape[0] > b.edge_index.shape[1]
    _stagewise("c09_mean_mean", b, 64, 2, "silu", True, cuda_device, inputs=True, aggr="mean",
               pool="mean", expect_tn=B3)


def test_case09_max_pool_with_isolated_nodes(cuda_device):
    # global_max_pool: g an exact selection, dzn through the shared arg-max mask
    b = _sparse_batch(6, 40, seed=29)
    _stagewise("c09_max_pool", b, 64, 2, "silu", False, cuda_device, inputs=True, pool="max",
               expect_tn=B3)


@pytest.mark.parametrize("act", ACT_NAMES)
def test_case10_activations_over_decades(act, cuda_device):
    # case 1's batch with node rows of x scaled by 1e-3 / 1 / 10 / 100: act through h0 and hn,
    # act' through dpre_{D-1} and dpre0, at |z| from ~1e-3 to ~1e2
    b = make_batch(12, n_atoms=30, n_bonds=34, n_mace=40, seed=101)
    _stagewise(f"c10_{act}", b, 128, 3, act, True, cuda_device, x_row_scales=[1e-3, 1, 10, 100],
               expect_tn=B3)


def test_case11_train_mode_dropout(cuda_device):
    # case 1 in train mode, p = 0.02: forward and dpre stages with the GPU's own recovered mask
    b = make_batch(12, n_atoms=30, n_bonds=34, n_mace=40, seed=101)
    _stagewise("c11_dropout", b, 128, 3, "silu", True, cuda_device, p_drop=0.02, expect_tn=B3)


# ---------------------------------------------------------------------------------------------
# H > 512: edge_init_fwd + segment_sum, a plain EpLayer launch + segment_sum per layer, every
# weight gradient on one of the fp32 TN kernels, chosen in csrc/wgrad.hpp from divisibility:
#   layer    tnr<5, 5> (H % 5 == 0), else tnr<4, 4> (H % 4 == 0), else the LDS-staged fp32 TN
#   readout  tnr<5, 4> over [x | a_D] when H % 5 == 0 and (Fp + H) % 4 == 0, else LDS-staged
#   node     tnr<5, 4> when H % 5 == 0 (x columns padded to Fp, or F % 4 == 0), else LDS-staged
# (the tnr x-side forms also need x itself 16-byte aligned when it is read in place)
# The batches have E = 2 (mod 4) and an odd N unless said otherwise: the tnr waves' last 4-row
# step and the last split-K split are partial.
# ---------------------------------------------------------------------------------------------
def _wide_batch(n_mace, seed, graphs=7):
    return make_batch(graphs, 21, 23, n_mace=n_mace, seed=seed)


def test_case12_sweep_width(cuda_device):
    # H = 1000, the reference sweep's width: 13 column tiles of tnr<5, 5>, F = 118 -> Fp = 120
    b = _wide_batch(40, 112)
    assert (b.x.shape[0], b.edge_index.shape[1], b.x.shape[1]) == (147, 322, 118)
    _stagewise("c12_silu_h1000", b, 1000, 2, "silu", True, cuda_device, inputs=True,
               expect_tn=TNR)


def test_case13_mixed_families_padded_width(cuda_device):
    # H = 515 (Hp = 516), F = 85 -> Fp = 88: H % 5 == 0 but (Fp + H) % 4 != 0, so the readout
    # runs the LDS-staged TN and the other two tnr within one backward; the layer TN's 6 splits of 64 rows
    # over E = 322 leave 2 rows to the last
    b = _wide_batch(7, 113)
    assert (b.edge_index.shape[1], b.x.shape[1]) == (322, 85)
    _stagewise("c13_gelu_h515", b, 515, 2, "gelu", True, cuda_device, inputs=True,
               expect_tn=dict(layer="tnr", readout="f32", node="tnr"))


def test_case14_prime_width_relu_x_in_place(cuda_device):
    # H = 521 (prime): every weight gradient on the LDS-staged TN; F = 80: x read in place; ReLU
    b = _wide_batch(2, 114)
    assert b.x.shape[1] == 80
    _stagewise("c14_relu_h521", b, 521, 3, "relu", False, cuda_device, inputs=True, expect_tn=F32)


def test_case15_hub_segments_three_column_tiles(cuda_device):
    # hub segments of 150 / 70 / 300 rows across row tiles, H = 520; F = 21 -> Fp = 24: one
    # ragged k tile in the node TN
    b = _hub_batch([150, 3, 70, 300, 5], seed=43)
    assert b.edge_index.shape[1] == 1056
    _stagewise("c15_hub_h520", b, 520, 2, "relu", True, cuda_device, expect_tn=TNR)


def test_case16_mean_modes_isolated_nodes_dropout(cuda_device):
    # mean / mean with in-degree-0 nodes (scale_rows after the unfused segment_sum) and dropout
    # in the unfused forward; H = 516: tnr<4, 4> for the layer
    b = _sparse_batch(6, 40, seed=31)
    _stagewise("c16_mean_h516", b, 516, 2, "silu", True, cuda_device, aggr="mean", pool="mean",
               p_drop=0.02, expect_tn=dict(layer="tnr", readout="f32", node="f32"))


def test_case17_unpaired_order_unpadded_x_tnr(cuda_device):
    # edges shuffled inside every graph with the unfused forward; F = 80, H = 560: the tnr
    # branches that read b->x directly
    u = _shuffled_pairs(_wide_batch(2, 115, graphs=6), seed=5)
    assert u.x.shape[1] == 80
    _stagewise("c17_unpaired_h560", u, 560, 2, "gelu", True, cuda_device, expect_tn=TNR)
    torch.cuda.synchronize()
    bits = native.raise_device_errors(cuda_device)  # raises on a completion timeout
    assert bits & native.DEVERR_UNPAIRED_SEEN


def test_case17_x_two_floats_off_16_bytes(cuda_device):
    # case 17's batch (edges in paired order) with x starting two floats into its buffer (pointer
    # % 16 == 8): the two-wide loaders (x-GEMM, LdConcat<2> / LdPlain<2> of the LDS-staged fp32
    # TN); H = 560 would put the x-side gradients on tnr<5, 4>, refused on the alignment alone
    b = _wide_batch(2, 115, graphs=6)
    assert b.x.shape[1] == 80
    _stagewise("c17_gelu_h560_x8", b, 560, 2, "gelu", True, cuda_device, x_offset=2,
               expect_tn=dict(layer="tnr", readout="f32", node="f32"))


def test_predict_rings_equal_training_forward_bitwise_h1000(cuda_device):
    # case 12's widths at depth 4: the no-grad forward (cgr_gnn_predict: h on a two-buffer ring,
    # a on a three-buffer ring, no fused zeroing above 512) against the grad-enabled forward
    b = _wide_batch(40, 112)
    data = b.to_torch(cuda_device)
    torch.manual_seed(4 * 7 + 1000)
    m = GNN(b.x.shape[1], b.edge_attr.shape[1], depth=4, hidden_sizes=[1000] * 4,
            dropout_ps=[0.0] * 4, activation_fn=ACT["silu"], use_learnable_skip=True)
    with torch.no_grad():
        for i, w in enumerate(m.skip_weights):
            w.fill_(0.5 + 0.25 * i)
    m = m.to(cuda_device).eval()
    y_train = m(data)  # grad enabled, parameters require grad: the training forward
    assert y_train.requires_grad
    with torch.no_grad():
        y_pred = m(data)
    assert not y_pred.requires_grad
    assert torch.equal(y_pred, y_train.detach())
