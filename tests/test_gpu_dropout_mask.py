"""GPU: the train-mode dropout mask, bit for bit against the host model of its hash
(oracle/dropout.py: written from the definitions in csrc/, never from GPU output).

The mask is a pure integer function, keep[r, c] = drop_hash(key, layer, r * H + c) >= thresh, so
every place that evaluates it is held to tolerance zero, at every element of every layer:

* forward: EpLayerSeg (fused, Hp <= 512: m1, m2, m4, m5) and EpLayer::finish4 (unfused: m3);
* backward, through layer_row_apply (bwd_rows.hpp): the top layer's k_layer_bwd_img with the
  e-image (m1, m4) and without it (m3); the fused backward epilogue's interior rows and its
  crossing-segment completion (m1, m3; layers D-2 .. 0), and its unpaired completion (m4);
* the key: k_prep_count (CGR_PREP_SPLIT=1) and its one-workgroup twin in prep_one.hpp, with and
  without a device counter, in cgr_gnn_forward, cgr_gnn_predict, the module and a captured graph.

b3_pack.hip's e-image pass over dpre_l (b3_eimage, layers below the top) reads the finished dpre
and evaluates no mask: no case has to reach it.  Every case uses sigmoid: act(pre) > 0 for the
|pre| < 80 asserted here, so h == 0 exactly where the element was dropped and no element is left
out of any comparison.
"""

import numpy as np
import pytest
import torch

from stagewise_common import (MASK_CASES, MASK_D, TORCH_F32, mask_batch, mask_model,
                              model_masks)
from test_gpu_parity import _cfg_tuple
from test_gpu_stagewise import B3, _np, _stagewise

from cgr_mpnn_3D._amd import native
from cgr_mpnn_3D._amd.debug import ArenaRun
from cgr_mpnn_3D._amd.functional import gnn_predict
from cgr_mpnn_3D.models.GNN import GNN
from oracle import dropout as od
from oracle import stagewise as sw

pytestmark = pytest.mark.gpu

D = MASK_D


class _Case:
    """A mask case on the device: batch, parameters in C-ABI order, config tuple."""

    def __init__(self, case, dev, ps=None):
        kind, self.H, self.p, self.seed = MASK_CASES[case]
        self.b, m = mask_model(case, ps)
        self.ps = [float(q) for q in m.dropout_ps]
        self.m = m.to(dev)
        self.params = [q.detach().contiguous() for q in self.m.native_parameters()]
        self.data = self.b.to_torch(dev)
        self.N, self.E, self.B = self.b.x.shape[0], self.b.edge_index.shape[1], self.b.num_graphs
        self.cfg_t = _cfg_tuple(self.b.x.shape[1], self.b.edge_attr.shape[1], self.H, D, "sigmoid",
                                True)

    def run(self, ps=None, seed=None, training=True, counter=None):
        d = self.data
        return ArenaRun(self.cfg_t, d.x, d.edge_index, d.edge_attr, d.batch, d.ptr, self.B,
                        self.params, dropout_ps=self.ps if ps is None else ps,
                        seed=self.seed if seed is None else seed, training=training,
                        rng_counter=counter)

    def predict(self, ps, seed, training, counter):
        d = self.data
        return gnn_predict(self.cfg_t, d.x, d.edge_index, d.edge_attr, d.batch, d.ptr, self.B, ps,
                           seed, training, self.params, rng_counter=counter)


def _layers(c, run):
    """[(pre_{l+1}, h_{l+1})] over the logical [E, H], rows in dst-sorted order."""
    out = []
    for l in range(D):
        pre, h = _np(run.floats("pre", c.E, index=l + 1)), _np(run.floats("h", c.E, index=l + 1))
        assert np.isfinite(pre).all() and np.abs(pre).max() < 80, (l, np.abs(pre).max())
        out.append((pre, h))
    return out


def _assert_masked_layer(tag, l, pre, h, keep, scale):
    """h != 0 exactly where the model keeps, and h = float32(sigmoid(pre) * scale) there, to the
    stagewise bar of an h stage (no sum: the activation allowance and the product's rounding)."""
    got = h != 0
    if not np.array_equal(got, keep):
        d = np.argwhere(got != keep)
        raise AssertionError(f"{tag}: layer {l} mask differs from the model at {len(d)} of "
                             f"{keep.size} elements, first (row, column) {d[0].tolist()}")
    ks = keep * float(scale)
    st = sw.activate(pre, "sigmoid", ks)
    r, at = sw.rho(h, st)
    rr, _ = sw.rho(sw.activate(pre, "sigmoid", ks, TORCH_F32).ref, st)
    assert r <= sw.bar(rr), (tag, l, r, rr, at)


def _profile_classes(fn):
    lib = native.load()
    lib.cgr_profile_reset()
    lib.cgr_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.cgr_profile_enable(0)
    classes = set(native.profile_report())
    lib.cgr_profile_reset()
    return classes


# ---------------------------------------------------------------------------------------------
# forward, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(MASK_CASES))
def test_forward_mask_equals_model_at_every_element(case, cuda_device):
    c = _Case(case, cuda_device)
    run = c.run()
    torch.cuda.synchronize()
    key = run.rng_key()
    assert key == od.forward_key(c.seed)  # no device counter: the key is the seed
    masks = model_masks(key, c.E, c.H, c.ps)
    for l, (pre, h) in enumerate(_layers(c, run)):
        _assert_masked_layer(case, l, pre, h, masks[l], od.thresh_scale(c.p)[1])
    assert np.isfinite(_np(run.y)).all()
    # the path and layout the case is there for
    status = int(run.ints("status", 1).item())
    assert (status == 4) == (case == "m4"), status
    classes = _profile_classes(c.run)
    fused, unfused = "gemm_nt_layer_seg_fwd" in classes, "gemm_nt_layer_fwd" in classes
    assert (fused, unfused) == ((False, True) if case == "m3" else (True, False)), sorted(classes)
    if case == "m5":  # dst segments over >= 3 of the 64-row tiles
        dst = _np(run.ints("dst_s", c.E))
        assert np.bincount(dst).max() >= 3 * 64 and c.E < 96 * 128
    if case == "m2":
        assert run.Hp == c.H + 1


# ---------------------------------------------------------------------------------------------
# key derivation: seed + Weyl step of the device counter, both bookkeeping forms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_key_follows_counter_forward_and_predict(split, cuda_device, monkeypatch):
    monkeypatch.setenv("CGR_PREP_SPLIT", "1" if split else "0")
    c = _Case("m1", cuda_device)
    # which bookkeeping ran: graph_prep.hip's launches (k_prep_count), or the x-GEMM launch's side
    # workgroup (prep_one.hpp), which has no profile class of its own
    assert ("graph_prep" in _profile_classes(c.run)) == split
    scale = od.thresh_scale(c.p)[1]
    for c0 in (0, 1, 41):
        counter = torch.tensor([c0], dtype=torch.int64, device=cuda_device)
        run = c.run(counter=counter)
        torch.cuda.synchronize()
        key = run.rng_key()
        assert key == od.forward_key(c.seed, c0) != od.forward_key(c.seed)
        assert int(counter.item()) == c0 + 1
        pre, h = _layers(c, run)[0]  # ... and that key is the one the epilogue used
        _assert_masked_layer(f"counter {c0}", 0, pre, h, od.keep_mask(key, 0, c.E, c.H, c.p),
                             scale)
        # cgr_gnn_predict with CGR_TRAIN_DROPOUT: the same rule (its arena is its own; its y is
        # that of a forward keyed with the predicted key)
        counter.fill_(c0)
        y = c.predict(c.ps, c.seed, True, counter)
        torch.cuda.synchronize()
        assert int(counter.item()) == c0 + 1
        assert torch.equal(y, c.run(seed=od.forward_key(c.seed, c0)).y)
        assert torch.equal(y, run.y)
    # no layer drops (p = 0 everywhere, or eval mode): no key wanted, the counter stays
    counter = torch.tensor([7], dtype=torch.int64, device=cuda_device)
    y_eval = c.run(training=False, counter=counter).y
    assert torch.equal(c.run(ps=[0.0] * D, counter=counter).y, y_eval)
    assert torch.equal(c.predict([0.0] * D, c.seed, True, counter), y_eval)
    assert torch.equal(c.predict(c.ps, c.seed, False, counter), y_eval)
    torch.cuda.synchronize()
    assert int(counter.item()) == 7


# ---------------------------------------------------------------------------------------------
# backward: every stage against the oracle fed the model's masks alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,expect_tn", [
    # top layer: k_layer_bwd_img writing the e-image; layers 1, 0: the fused epilogue
    ("m1", B3),
    # H = 516: k_layer_bwd_img without an image, the layer gradient on tnr<4, 4>
    ("m3", dict(layer="tnr", readout="f32", node="f32")),
    # status 4: every row below the top layer through the unpaired completion
    ("m4", B3)])
def test_backward_stages_with_model_masks(case, expect_tn, cuda_device):
    kind, H, p, seed = MASK_CASES[case]
    rec = _stagewise(f"mask_{case}", mask_batch(kind), H, D, "sigmoid", True, cuda_device, p_drop=p,
                     expect_tn=expect_tn, mask="model", drop_seed=seed)
    assert rec["key"] == od.forward_key(seed)
    if case == "m4":
        torch.cuda.synchronize()
        assert native.raise_device_errors(cuda_device) & native.DEVERR_UNPAIRED_SEEN


# ---------------------------------------------------------------------------------------------
# edges of p
# ---------------------------------------------------------------------------------------------
def test_p_one_drops_everything(cuda_device):
    # thresh 0xFFFFFFFF, scale 0: h_{l+1} exactly 0, y finite; every stage and gradient against
    # the oracle with all-zero keep (a layer weight's gradient: exactly 0, its S is 0)
    kind, H, _, seed = MASK_CASES["m1"]
    rec = _stagewise("mask_p1", mask_batch(kind), H, D, "sigmoid", True, cuda_device, p_drop=1.0, expect_tn=B3,
                     mask="model", drop_seed=seed)
    for l in range(D):
        assert not rec["h"][l + 1].any() and not rec["dpre"][l].any()
        assert not rec["grads"][f"convs.{l}.lin.weight"].any()
    assert np.isfinite(rec["y"]).all()


def test_p_tiny_keeps_all_but_hash_zero(cuda_device):
    # p = 1e-12: thresh 1 (clamped up from 0), scale 1.0f: the eval-mode h bit for bit, except
    # where the hash is 0 -- the model says where (almost surely nowhere)
    c = _Case("m1", cuda_device, ps=[1e-12] * D)
    assert od.thresh_scale(1e-12) == (1, np.float32(1.0))
    run, ev = c.run(), c.run(training=False)
    torch.cuda.synchronize()
    assert run.rng_key() == od.forward_key(c.seed)
    masks = model_masks(run.rng_key(), c.E, c.H, c.ps)
    for l, ((_, h), (_, h_eval)) in enumerate(zip(_layers(c, run), _layers(c, ev))):
        dropped = ~masks[l]
        assert np.array_equal((h == 0) & (h_eval != 0), dropped), l
        assert h[~dropped].tobytes() == h_eval[~dropped].tobytes(), l
        if dropped.any():  # later layers see another input
            break
    else:
        assert torch.equal(run.y, ev.y)


def test_mixed_p_masks_one_layer_only(cuda_device):
    # p = [0, 0.5, 0]: only layer 1 is masked, and the key is still written and advanced
    ps = [0.0, 0.5, 0.0]
    c = _Case("m1", cuda_device, ps=ps)
    counter = torch.tensor([3], dtype=torch.int64, device=cuda_device)
    run = c.run(counter=counter)
    torch.cuda.synchronize()
    key = run.rng_key()
    assert key == od.forward_key(c.seed, 3) and int(counter.item()) == 4
    masks = model_masks(key, c.E, c.H, ps)
    assert masks[0] is None and masks[2] is None
    every = np.ones((c.E, c.H), bool)
    for l, (pre, h) in enumerate(_layers(c, run)):
        _assert_masked_layer("mixed", l, pre, h, every if masks[l] is None else masks[l],
                             od.thresh_scale(ps[l])[1])
    assert not masks[1].all()


# ---------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------
def test_module_forward_is_keyed_by_generator_seed_instance_and_counter(cuda_device):
    c = _Case("m1", cuda_device)
    m, s = c.m, 20261
    torch.manual_seed(s)
    seed = od.module_seed(s, m._cgr_instance)
    assert m._cgr_dropout_seed(cuda_device) == seed
    for _ in range(2):  # the second forward uses counter + 1
        counter = m._cgr_rng_counter.clone()
        c0 = int(counter.item())
        y = m(c.data)
        assert y.requires_grad
        run = c.run(seed=seed, counter=counter)
        torch.cuda.synchronize()
        assert torch.equal(y.detach(), run.y)
        assert run.rng_key() == od.forward_key(seed, c0)
        assert int(m._cgr_rng_counter.item()) == int(counter.item()) == c0 + 1
    # a model built after the first: the next construction index, another key
    m2 = GNN(c.b.x.shape[1], c.b.edge_attr.shape[1], depth=D, hidden_sizes=[c.H] * D,
             dropout_ps=c.ps, activation_fn=torch.sigmoid, use_learnable_skip=True)
    assert m2._cgr_instance == m._cgr_instance + 1
    assert m2._cgr_dropout_seed(cuda_device) == od.module_seed(s, m2._cgr_instance) != seed
