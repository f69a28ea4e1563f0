"""GPU: the fp32-faithful precision mode (config.precision = "fp32", CGR_PRECISION_FP32).

The default mode's gradients miss the plain fp32-class bars in three known places:
the sigmoid golden (held to 2e-4 in tests/test_gpu_parity.py), the cancelled learnable-skip
scalar of the H = 1000 / D = 4 sweep case (an extra 2^-20 sum |terms|), and the weight / bias
gradients of widths up to 512 (judged against a two-piece emulation, +768 / +256).  Here every one
of them is held to the plain bar under the switch: each stage against float64 at max(8, 4 rho_ref)
with no emulation and no additive term, the goldens and the sweep case at 1e-4.
tests/test_precision_mode.py shows on the CPU that the default mode's weight-gradient arithmetic
cannot pass these bars.  The shapes are the existing stagewise / parity / mask cases' own.
"""

import ctypes

import numpy as np
import pytest
import torch

import test_gpu_parity as tgp
import test_gpu_stagewise as tgs
from conftest import golden_cases, load_golden
from stagewise_common import MASK_CASES, MASK_D, mask_batch
from test_gpu_parity import (ACT, _cfg_tuple, _hub_batch, _oracle_compare, _shuffled_pairs,
                             _sparse_batch, assert_g_close, assert_y_close, batch_from_golden,
                             model_from_golden)

from cgr_mpnn_3D._amd import config, native
from cgr_mpnn_3D._amd.debug import ArenaRun
from cgr_mpnn_3D._amd.functional import (_batch_struct, _param_table, make_config,
                                         resolve_config_tuple)
from cgr_mpnn_3D._amd.synth import make_batch
from cgr_mpnn_3D.models.GNN import GNN
from oracle import dropout as od

pytestmark = pytest.mark.gpu

TN_CLASSES = tuple(tgs.TN_CLASSES.values()) + ("gemm_tn_wgrad_edge",)


@pytest.fixture
def fp32_mode():
    was = config.precision
    config.precision = "fp32"
    yield
    config.precision = was


def _assert_fp32_classes(classes):
    """Every weight-gradient class of a profiled step carries an fp32 family's suffix, and no
    e-image pass ran."""
    tn = [c for c in classes if c.startswith("gemm_tn_wgrad_")]
    assert len(tn) >= 3, sorted(classes)
    for c in tn:
        assert c.endswith("[tnr]") or c.endswith("[f32]"), (c, sorted(classes))
    assert "eimage" not in classes, sorted(classes)


# ---------------------------------------------------------------------------------------------
# 5. every stage fp32-class against float64
# ---------------------------------------------------------------------------------------------
# The first feasible fp32 family by csrc/wgrad.hpp's rules (N = hidden width, K = operand width):
#   layer    tnr<5, 5> (H % 5 == 0), else tnr<4, 4> (H % 4 == 0), else the LDS-staged fp32 TN
#   readout  tnr<5, 4> when H % 5 == 0 and (Fx + H) % 4 == 0, else LDS-staged
#   node     tnr<5, 4> when H % 5 == 0 (Fx % 4 == 0 always), else LDS-staged
L_TNR = dict(layer="tnr", readout="f32", node="f32")  # H % 4 == 0, H % 5 != 0
ALL_F32 = dict(layer="f32", readout="f32", node="f32")
ALL_TNR = dict(layer="tnr", readout="tnr", node="tnr")


def _fp32_stagewise(monkeypatch, case, *args, **kw):
    seen = []
    inner = tgs._tn_families

    def families(*a, **k):
        fam, classes = inner(*a, **k)
        seen.append(classes)
        return fam, classes

    monkeypatch.setattr(tgs, "_tn_families", families)
    rec = tgs._stagewise("fp32_" + case, *args, **kw)
    assert len(seen) == 1
    _assert_fp32_classes(seen[0])
    # judged as fp32 families: against float64 alone, no emulation, no additive bar term
    assert set(rec["tn"].values()) == {"f32"}
    return rec


def test_stages_c01_silu_h128_inputs(cuda_device, fp32_mode, monkeypatch):
    b = make_batch(12, n_atoms=30, n_bonds=34, n_mace=40, seed=101)
    _fp32_stagewise(monkeypatch, "c01_silu_h128", b, 128, 3, "silu", True, cuda_device,
                    inputs=True, expect_tn=L_TNR)  # H = 128: tnr<4, 4>


def test_stages_c02_gelu_h39(cuda_device, fp32_mode, monkeypatch):
    b = make_batch(6, 14, 16, n_mace=7, seed=102)
    _fp32_stagewise(monkeypatch, "c02_gelu_h39", b, 39, 2, "gelu", True, cuda_device,
                    inputs=True, expect_tn=ALL_F32)  # H = 39: no tnr tile divides it


def test_stages_c03_relu_h96_x_in_place(cuda_device, fp32_mode, monkeypatch):
    b = make_batch(10, 24, 26, n_mace=2, seed=103)
    assert b.x.shape[1] == 80
    _fp32_stagewise(monkeypatch, "c03_relu_h96", b, 96, 3, "relu", False, cuda_device,
                    inputs=True, expect_tn=L_TNR)  # H = 96: tnr<4, 4>


def test_stages_c04_cfg2_widths(cuda_device, fp32_mode, monkeypatch):
    # H = 400: tnr<5, 5> on the layer, tnr<5, 4> over [xp | a_D] (848 + 400 columns) and xp; 25
    # column fragments: the widest tiles of the per-step NT variant
    _fp32_stagewise(monkeypatch, "c04_cfg2_32", make_batch(32, seed=104), 400, 4, "relu", False,
                    cuda_device, expect_tn=ALL_TNR)


def test_stages_c06_hub_segments_skip(cuda_device, fp32_mode, monkeypatch):
    b = _hub_batch([150, 3, 70, 300, 5], seed=41)
    _fp32_stagewise(monkeypatch, "c06_hub64_skip1", b, 64, 3, "relu", True, cuda_device,
                    expect_tn=L_TNR)


def test_stages_c08_unpaired_order(cuda_device, fp32_mode, monkeypatch):
    u = _shuffled_pairs(make_batch(8, n_atoms=30, n_bonds=30, n_mace=16, seed=28), seed=5)
    _fp32_stagewise(monkeypatch, "c08_unpaired", u, 64, 3, "gelu", True, cuda_device,
                    expect_tn=L_TNR)
    torch.cuda.synchronize()
    assert native.raise_device_errors(cuda_device) & native.DEVERR_UNPAIRED_SEEN


def test_stages_c09_mean_modes_isolated_nodes(cuda_device, fp32_mode, monkeypatch):
    b = _sparse_batch(6, 40, seed=27)
    _fp32_stagewise(monkeypatch, "c09_mean_mean", b, 64, 2, "silu", True, cuda_device,
                    inputs=True, aggr="mean", pool="mean", expect_tn=L_TNR)


def test_stages_train_mode_model_mask_m1(cuda_device, fp32_mode, monkeypatch):
    kind, H, p, seed = MASK_CASES["m1"]
    assert (H, p) == (64, 0.5)
    rec = _fp32_stagewise(monkeypatch, "mask_m1", mask_batch(kind), H, MASK_D, "sigmoid", True,
                          cuda_device, p_drop=p, expect_tn=L_TNR, mask="model", drop_seed=seed)
    assert rec["key"] == od.forward_key(seed)


# ---------------------------------------------------------------------------------------------
# 6. goldens at the plain bar (the sigmoid case included: 1e-4, not 2e-4)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", golden_cases())
def test_goldens_forward_and_all_gradients_at_the_plain_bar(case, cuda_device, fp32_mode):
    z, meta = load_golden(case)
    m = model_from_golden(z, meta, cuda_device)
    m.eval()
    with torch.no_grad():
        y = m(batch_from_golden(z, meta, cuda_device))
    assert_y_close(y.cpu().numpy(), z["out_y_eval"])

    m = model_from_golden(z, meta, cuda_device, dropout=0.0)
    m.train()
    data = batch_from_golden(z, meta, cuda_device)
    data.x.requires_grad_(True)
    data.edge_attr.requires_grad_(True)
    pred = m(data)
    loss = torch.nn.MSELoss(reduction="sum")(pred, data.y.view_as(pred))
    loss.backward()
    assert abs(loss.item() - float(z["out_loss"])) <= 1e-4 * abs(float(z["out_loss"]))
    worst = ("", 0.0)
    for k, p in m.named_parameters():
        g, ref = p.grad.cpu().numpy().astype(np.float64), np.asarray(z["g_" + k], np.float64)
        err = np.abs(g - ref).max() / (np.abs(ref).max() + 1e-30)
        worst = max(worst, (k, err), key=lambda t: t[1])
    print(f"{case}: largest parameter-gradient error {worst[1]:.3e} ({worst[0]})")
    for k, p in m.named_parameters():
        assert_g_close(p.grad.cpu().numpy(), z["g_" + k], k)  # rtol: the default 1e-4
    assert_g_close(data.x.grad.cpu().numpy(), z["gin_x"], "x")
    if z["gin_edge_attr"].size:
        assert_g_close(data.edge_attr.grad.cpu().numpy(), z["gin_edge_attr"], "edge_attr")


# ---------------------------------------------------------------------------------------------
# 7. the cancelled skip scalar: plain 1e-4 on every tensor, no sum |terms| allowance
# ---------------------------------------------------------------------------------------------
def test_sweep_h1000_d4_skip_scalars_at_plain_bar(cuda_device, fp32_mode, monkeypatch):
    H, D, skip = 1000, 4, True
    b = make_batch(6, n_atoms=30, n_bonds=30, n_mace=768, seed=H + 10 * D + skip)
    monkeypatch.setattr(tgp, "SKIP_COND_U", 0.0)
    _oracle_compare(b, H, D, "relu", skip, cuda_device, seed=H + D)


# ---------------------------------------------------------------------------------------------
# 8. mode plumbing
# ---------------------------------------------------------------------------------------------
def _module(b, H, D, dev, act="silu", seed=0):
    torch.manual_seed(seed)
    m = GNN(b.x.shape[1], b.edge_attr.shape[1], depth=D, hidden_sizes=[H] * D,
            dropout_ps=[0.0] * D, activation_fn=ACT[act], use_learnable_skip=True)
    return m.to(dev).train()


def _profiled_step(m, data):
    lib = native.load()
    lib.cgr_profile_reset()
    lib.cgr_profile_enable(1)
    try:
        m.zero_grad(set_to_none=True)
        torch.nn.MSELoss(reduction="sum")(m(data), data.y).backward()
        torch.cuda.synchronize()
    finally:
        lib.cgr_profile_enable(0)
    classes = set(native.profile_report())
    lib.cgr_profile_reset()
    return classes


def test_switch_selects_the_families_and_back(cuda_device):
    b = make_batch(8, n_atoms=20, n_bonds=22, n_mace=16, seed=7)
    m, data = _module(b, 64, 2, cuda_device), b.to_torch(cuda_device)
    was = config.precision
    try:
        config.precision = "fp32"
        _assert_fp32_classes(_profiled_step(m, data))
        config.precision = "split"
        classes = _profiled_step(m, data)
    finally:
        config.precision = was
    for c in tgs.TN_CLASSES.values():  # H = 64: the split-bf16 e-image TN, plain class names
        assert c in classes and c + "[tnr]" not in classes and c + "[f32]" not in classes
    assert "eimage" in classes


def test_backward_runs_in_its_forwards_mode_whatever_the_switch_says(cuda_device):
    b = make_batch(8, n_atoms=20, n_bonds=22, n_mace=16, seed=7)
    m, data = _module(b, 64, 2, cuda_device), b.to_torch(cuda_device)
    loss_fn = torch.nn.MSELoss(reduction="sum")
    was = config.precision
    grads = {}
    try:
        for flip in (False, True):
            config.precision = "fp32"
            m.zero_grad(set_to_none=True)
            loss = loss_fn(m(data), data.y)
            if flip:
                config.precision = "split"
            loss.backward()
            torch.cuda.synchronize()
            grads[flip] = [p.grad.clone() for p in m.parameters()]
        config.precision = "split"
        m.zero_grad(set_to_none=True)
        loss_fn(m(data), data.y).backward()
        split = [p.grad.clone() for p in m.parameters()]
    finally:
        config.precision = was
    for (k, _), g0, g1 in zip(m.named_parameters(), grads[False], grads[True]):
        assert torch.equal(g0, g1), k
    # ... and that mode is not the default's: some gradient differs from a split-mode step
    assert any(not torch.equal(a, c) for a, c in zip(grads[False], split))


def test_backward_refuses_a_config_of_another_mode(cuda_device):
    lib = native.load()
    b = make_batch(4, n_atoms=12, n_bonds=13, n_mace=8, seed=3)
    m, d = _module(b, 24, 2, cuda_device, act="relu"), b.to_torch(cuda_device)
    params = [p.detach() for p in m.native_parameters()]
    t8 = _cfg_tuple(b.x.shape[1], 14, 24, 2, "relu", True)
    dy = torch.ones(b.num_graphs, device=cuda_device)
    for fwd_mode in (1, 0):
        run = ArenaRun(t8 + (fwd_mode,), d.x, d.edge_index, d.edge_attr, d.batch, d.ptr,
                       b.num_graphs, params)
        assert run.cfg.precision == fwd_mode
        other = make_config(*(t8 + (1 - fwd_mode,)))
        ws = torch.empty(max(lib.cgr_gnn_workspace_bytes(ctypes.byref(c), run.N, run.E, run.B)
                             for c in (run.cfg, other)), dtype=torch.uint8, device=cuda_device)
        grads = [torch.full_like(p, 12345.0) for p in params]
        rc = lib.cgr_gnn_backward(ctypes.byref(other), _param_table(params), ctypes.byref(run.bs),
                                  None, 0, run.flags, native.ptr(run.arena), native.ptr(dy),
                                  _param_table(grads), native.ptr(ws), None,
                                  native.stream_ptr(cuda_device))
        assert rc != 0 and b"precision" in lib.cgr_last_error()
        torch.cuda.synchronize()
        assert all(bool((g == 12345.0).all()) for g in grads)  # nothing was enqueued
        got = run.backward(dy, params)  # the forward's own mode runs
        with pytest.raises(RuntimeError, match="precision"):
            saved, run.cfg = run.cfg, other
            try:
                run.input_grads(dy, params, run.ws)
            finally:
                run.cfg = saved
        run.input_grads(dy, params, run.ws)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(g).all()) for g in got)


def test_switch_reaches_the_nt_kernels(cuda_device):
    # c01's forward: the first layer's pre-activation differs between the modes in some bit
    b = make_batch(12, n_atoms=30, n_bonds=34, n_mace=40, seed=101)
    m, d = _module(b, 128, 3, cuda_device), b.to_torch(cuda_device)
    params = [p.detach() for p in m.native_parameters()]
    t8 = _cfg_tuple(b.x.shape[1], b.edge_attr.shape[1], 128, 3, "silu", True)
    pre = {}
    for mode in (0, 1):
        run = ArenaRun(t8 + (mode,), d.x, d.edge_index, d.edge_attr, d.batch, d.ptr, b.num_graphs,
                       params)
        torch.cuda.synchronize()
        pre[mode] = run.floats("pre", run.E, index=1).clone()
    assert pre[0].shape == pre[1].shape and not torch.equal(pre[0], pre[1])
    assert torch.allclose(pre[0], pre[1], rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------------
# 9. the forward-only path
# ---------------------------------------------------------------------------------------------
def test_predict_equals_training_forward_bitwise_also_with_packed_images(cuda_device, fp32_mode):
    lib = native.load()
    b = make_batch(12, n_atoms=30, n_bonds=34, n_mace=40, seed=101)
    H, D = 128, 3
    m, data = _module(b, H, D, cuda_device), b.to_torch(cuda_device)
    m.eval()
    y_train = m(data)
    assert y_train.requires_grad
    with torch.no_grad():
        y_pred = m(data)
    assert torch.equal(y_pred, y_train.detach())
    # caller-packed images: cgr_gnn_pack_images and cgr_gnn_predict agree on one config's layout
    t9 = resolve_config_tuple(_cfg_tuple(b.x.shape[1], b.edge_attr.shape[1], H, D, "silu", True))
    assert t9[8] == 1
    cfg = make_config(*t9)
    params = [p.detach().contiguous() for p in m.native_parameters()]
    N, E, B = b.x.shape[0], b.edge_index.shape[1], b.num_graphs
    images = torch.empty(lib.cgr_gnn_image_bytes(ctypes.byref(cfg)), dtype=torch.uint8,
                         device=cuda_device)
    arena = torch.empty(lib.cgr_gnn_predict_arena_bytes(ctypes.byref(cfg), N, E, B),
                        dtype=torch.uint8, device=cuda_device)
    y = torch.empty(B, device=cuda_device)
    bs = _batch_struct(data.x, data.edge_index, data.edge_attr, data.batch, data.ptr, B)
    st = native.stream_ptr(cuda_device)
    native.check(lib.cgr_gnn_pack_images(ctypes.byref(cfg), _param_table(params),
                                         native.ptr(images), st))
    native.check(lib.cgr_gnn_predict(ctypes.byref(cfg), _param_table(params), ctypes.byref(bs),
                                     None, 0, None, 0, native.ptr(images), native.ptr(arena),
                                     native.ptr(y), st))
    torch.cuda.synchronize()
    assert torch.equal(y, y_train.detach())


# ---------------------------------------------------------------------------------------------
# 10. a captured step keeps the mode it was captured in and equals the eager steps bitwise
# ---------------------------------------------------------------------------------------------
def test_three_captured_steps_equal_eager_steps_bitwise(cuda_device, fp32_mode):
    from test_gpu_captured_epoch import _eager_epoch, _full

    from cgr_mpnn_3D._amd.captured import CapturedTrainer
    from cgr_mpnn_3D._amd.data import GraphStore
    from cgr_mpnn_3D._amd.loss import MSELoss
    from cgr_mpnn_3D._amd.optim import FusedAdam

    B = 8
    b = make_batch(24, n_atoms=10, n_bonds=12, n_mace=3, seed=22, n_atoms_jitter=3)
    store = GraphStore.from_batch(b, cuda_device)
    batches = [np.arange(8 * i, 8 * i + 8, dtype=np.int64) for i in range(3)]
    sizes = [store.batch_sizes(_full(ids, B)[0]) for ids in batches]
    caps = (max(n for n, _ in sizes) + 40, max(e for _, e in sizes) + 8)
    loss_fn = MSELoss("sum")

    def fresh():
        m = _module(b, 64, 2, cuda_device)
        return m, FusedAdam(m.parameters(), lr=1e-3, amsgrad=True)

    m1, o1 = fresh()
    _, ref_total = _eager_epoch(m1, o1, loss_fn, store, batches, B, caps)
    m2, o2 = fresh()
    tr = CapturedTrainer(m2, o2, loss_fn, store, B, *caps)
    tr.step(batches[0])  # captured under "fp32" ...
    config.precision = "split"  # ... and replayed whatever the switch says (restored by fp32_mode)
    for ids in batches[1:]:
        tr.step(ids)
    assert tr.fallbacks == 0
    torch.cuda.synchronize()
    for (k, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), k
    assert torch.equal(tr.loss_total, ref_total)
    tr.close()
