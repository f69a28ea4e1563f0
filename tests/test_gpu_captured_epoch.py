"""Captured training over ragged batches (cgr_mpnn_3D/_amd/captured.py): the padded step against
the fp64 oracle on the unpadded batch, CapturedTrainer against the same steps run eagerly
(bitwise: no kernel of the step uses atomics), the eager fallback, predict(), and FusedAdam with
the learning rate as a device tensor (cgr_adam_step_lr_ptr)."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cgr_mpnn_3D._amd.captured import CapturedTrainer
from cgr_mpnn_3D._amd.data import GraphStore
from cgr_mpnn_3D._amd.loss import MSELoss
from cgr_mpnn_3D._amd.optim import FusedAdam
from cgr_mpnn_3D._amd.synth import make_batch
from cgr_mpnn_3D.models.GNN import GNN, global_add_pool, global_max_pool, global_mean_pool
from oracle import collate_numpy as oc
from oracle import dmpnn_numpy as on

pytestmark = pytest.mark.gpu

POOLS = {"add": global_add_pool, "mean": global_mean_pool, "max": global_max_pool}
D, H = 2, 48


def _store_arrays(b):
    src_graph = b.batch[b.edge_index[0]]
    ecount = np.bincount(src_graph, minlength=b.num_graphs)
    edge_ptr = np.concatenate([[0], np.cumsum(ecount)]).astype(np.int64)
    return b.x, b.edge_index, b.edge_attr, b.y, b.ptr, edge_ptr


def _model(F_, dev, pool="add", aggr="add"):
    torch.manual_seed(0)
    m = GNN(F_, 14, depth=D, hidden_sizes=[H] * D, dropout_ps=[0.0] * D, activation_fn=F.silu,
            aggr=aggr, pooling_fn=POOLS[pool])
    return m.to(dev).train()


# -- (a) the padded step against the fp64 oracle on the unpadded batch ---------------------------

@pytest.fixture(scope="module")
def small(cuda_device):
    b = make_batch(12, n_atoms=10, n_bonds=12, n_mace=3, seed=21, n_atoms_jitter=3)
    assert np.diff(b.ptr).min() >= 7 and np.diff(b.ptr).max() <= 13
    return b, GraphStore.from_batch(b, cuda_device)


@pytest.mark.parametrize("pool", ["add", "mean", "max"])
@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_padded_step_matches_oracle_on_unpadded_batch(pool, aggr, small, cuda_device):
    b, store = small
    real = np.arange(10)
    full = np.concatenate([real, [0, 1]])          # two filler slots at weight 0
    w = torch.tensor([1.0] * 10 + [0.0] * 2, device=cuda_device)
    N, E = store.batch_sizes(full)
    N_cap, E_cap = N + 9, E + 28                   # 9 pad nodes, 14 pad pairs: in-degree <= 4
    assert N % 64 and E % 64                       # both boundaries lie inside a 64-row tile
    assert store.fits(full, N_cap, E_cap)
    m = _model(b.x.shape[1], cuda_device, pool, aggr)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    pb = store.collate_padded(full, N_cap, E_cap, weight_dev=w)
    pred = m(pb)
    assert pred.shape == (13,)
    loss = torch.nn.MSELoss(reduction="sum")(pred * pb.mask, pb.y * pb.mask)
    loss.backward()
    torch.cuda.synchronize()
    assert int(pb.info[2]) == 0
    assert bool(torch.isfinite(pred).all())        # fillers and the pad graph included

    u = oc.collate(real, *_store_arrays(b))
    loss_o, y_o, g_o = on.loss_and_grads(sd, u["x"], u["edge_index"], u["edge_attr"], u["batch"],
                                         u["y"], D, "silu", False, num_graphs=10, aggr=aggr,
                                         pool=pool)
    y = pred.detach().cpu().numpy().astype(np.float64)[:10]
    err_y = np.abs(y - y_o)
    print(f"pool={pool} aggr={aggr}: max |dy| {err_y.max():.3e} (|y| max {np.abs(y_o).max():.3e})")
    assert np.all(err_y <= 1e-4 * np.abs(y_o) + 1e-6 * np.abs(y_o).max())
    assert abs(float(loss.detach()) - loss_o) <= 1e-4 * abs(loss_o)
    for k, p in m.named_parameters():
        g = p.grad.cpu().numpy().astype(np.float64)
        err = np.abs(g - g_o[k]).max() / (np.abs(g_o[k]).max() + 1e-30)
        print(f"  {k}: rel err {err:.3e}")
        assert np.isfinite(g).all(), k
        assert err <= 1e-4, f"{k}: rel err {err:.3e}"


# -- (b), (c): CapturedTrainer against eager loops ------------------------------------------------

@pytest.fixture(scope="module")
def epoch(cuda_device):
    b = make_batch(44, n_atoms=10, n_bonds=12, n_mace=3, seed=22, n_atoms_jitter=3)
    store = GraphStore.from_batch(b, cuda_device)
    order = np.argsort(-np.diff(b.ptr), kind="stable")
    rest = np.random.default_rng(3).permutation(order[8:])
    # batch 2 holds the 8 largest graphs; the last batch is short (4 of 8 slots)
    batches = [rest[0:8], rest[8:16], order[:8], rest[16:24], rest[24:32], rest[32:36]]
    return b, store, [np.asarray(x, np.int64) for x in batches]


def _full(ids, B):
    n = len(ids)
    w = np.zeros(B, np.float32)
    w[:n] = 1.0
    return (np.resize(ids, B) if n < B else ids), w


def _eager_epoch(m, opt, loss_fn, store, batches, B, caps, unpadded=()):
    """The reference loop: the same padded batches (or, for the steps in `unpadded`, the plain
    store.collate batch), run eagerly."""
    losses = []
    total = torch.zeros((), device=store.device)
    for i, ids in enumerate(batches):
        opt.zero_grad(set_to_none=True)
        if i in unpadded:
            pb = store.collate(ids)
            loss = loss_fn(m(pb), pb.y)
        else:
            full, w = _full(ids, B)
            pb = store.collate_padded(full, *caps,
                                      weight_dev=torch.from_numpy(w).to(store.device))
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


def test_captured_epoch_equals_eager_padded_epoch(epoch, cuda_device):
    b, store, batches = epoch
    B = 8
    sizes = [store.batch_sizes(_full(ids, B)[0]) for ids in batches]
    caps = (max(n for n, _ in sizes) + 40, max(e for _, e in sizes) + 8)
    assert len({s for s in sizes}) == len(sizes)   # ragged: every batch has its own N, E
    loss_fn = MSELoss("sum")

    m1 = _model(b.x.shape[1], cuda_device)
    o1 = FusedAdam(m1.parameters(), lr=1e-3, amsgrad=True)
    ref_losses, ref_total = _eager_epoch(m1, o1, loss_fn, store, batches, B, caps)

    m2 = _model(b.x.shape[1], cuda_device)
    o2 = FusedAdam(m2.parameters(), lr=1e-3, amsgrad=True)
    tr = CapturedTrainer(m2, o2, loss_fn, store, B, *caps)
    losses = []
    for ids in batches:
        out = tr.step(ids)
        assert out is tr.loss
        losses.append(out.clone())
    assert tr.fallbacks == 0
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(losses, ref_losses)):
        assert torch.equal(x, y), (i, float(x), float(y))
    _assert_same_training_state(m1, o1, m2, o2)
    assert tr.epoch_loss() == float(ref_total)
    assert tr.epoch_loss() == 0.0
    tr.close()


def test_fallback_runs_the_unfitting_batch_eagerly_unpadded(epoch, cuda_device):
    b, store, batches = epoch
    B = 8
    sizes = [store.batch_sizes(_full(ids, B)[0]) for ids in batches]
    others = [s for i, s in enumerate(sizes) if i != 2]
    caps = (max(n for n, _ in others) + 12, max(e for _, e in others) + 8)
    fit = [store.fits(_full(ids, B)[0], *caps) for ids in batches]
    assert fit == [True, True, False, True, True, True]
    loss_fn = MSELoss("sum")

    m1 = _model(b.x.shape[1], cuda_device)
    o1 = FusedAdam(m1.parameters(), lr=1e-3, amsgrad=True)
    _, ref_total = _eager_epoch(m1, o1, loss_fn, store, batches, B, caps, unpadded=(2,))

    m2 = _model(b.x.shape[1], cuda_device)
    o2 = FusedAdam(m2.parameters(), lr=1e-3, amsgrad=True)
    tr = CapturedTrainer(m2, o2, loss_fn, store, B, *caps)
    for ids in batches:
        tr.step(ids)
    assert tr.fallbacks == 1
    torch.cuda.synchronize()
    _assert_same_training_state(m1, o1, m2, o2)
    assert tr.epoch_loss() == float(ref_total)


# -- (d) predict -----------------------------------------------------------------------------------

def test_predict_equals_eval_forward_on_the_plain_batch(epoch, cuda_device):
    b, store, batches = epoch
    B = 8
    m = _model(b.x.shape[1], cuda_device)
    opt = FusedAdam(m.parameters(), lr=1e-2, amsgrad=True)
    tr = CapturedTrainer(m, opt, MSELoss("sum"), store, B)

    def check():
        for ids in (batches[0], batches[5], batches[2]):   # full, short (4 ids), full
            got = tr.predict(ids).clone()
            assert got.shape == (len(ids),)
            assert m.training
            m.eval()
            with torch.no_grad():
                ref = m(store.collate(ids))
            m.train()
            torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)

    check()
    before = tr.predict(batches[0]).clone()
    tr.step(batches[1])                             # the captured predict reads the new weights
    assert not torch.equal(tr.predict(batches[0]), before)
    check()
    assert tr.fallbacks == 0


# -- (e) lr as a device tensor ---------------------------------------------------------------------

SHAPES = [(400, 860), (400,), (400, 400), (1, 400), (1,), (7, 3), (1001,), ()]


def test_fused_adam_tensor_lr_matches_torch_capturable_adam(cuda_device):
    g = torch.Generator().manual_seed(0)
    ps_ref = [torch.randn(s, generator=g).to(cuda_device).requires_grad_() for s in SHAPES]
    ps = [p.detach().clone().requires_grad_() for p in ps_ref]
    lr_ref = torch.tensor(3e-3, device=cuda_device)
    lr = torch.tensor(3e-3, device=cuda_device)
    ref = torch.optim.Adam(ps_ref, lr=lr_ref, capturable=True, amsgrad=True)
    opt = FusedAdam(ps, lr=lr, amsgrad=True)
    for it in range(5):
        for p, q in zip(ps, ps_ref):
            gr = torch.randn(p.shape, generator=g).to(cuda_device) * (1 + it)
            p.grad, q.grad = gr.clone(), gr.clone()
        opt.step()
        ref.step()
        lr.mul_(0.5)                                # in place, as a scheduler does
        lr_ref.mul_(0.5)
    torch.cuda.synchronize()
    assert opt.param_groups[0]["lr"] is lr
    for a, c in zip(ps, ps_ref):
        torch.testing.assert_close(a.detach(), c.detach(), rtol=1e-5, atol=1e-6)
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            torch.testing.assert_close(opt.state[a][k], ref.state[c][k], rtol=1e-5, atol=1e-6)
    with pytest.raises(RuntimeError, match="tensor lr"):
        bad = FusedAdam(ps, lr=torch.tensor(1e-3), amsgrad=True)  # a CPU tensor
        bad.step()


def test_captured_step_follows_exponential_lr_on_a_tensor_lr(epoch, cuda_device):
    b, store, batches = epoch
    B = 8
    caps = store.padded_caps(B)
    caps = (caps[0] + 30, caps[1])
    loss_fn = MSELoss("sum")
    steps = [batches[0], batches[1], batches[3], batches[4]]
    assert all(store.fits(ids, *caps) for ids in steps)

    m1 = _model(b.x.shape[1], cuda_device)
    o1 = FusedAdam(m1.parameters(), lr=2.0 ** -10, amsgrad=True)
    m2 = _model(b.x.shape[1], cuda_device)
    lr = torch.tensor(2.0 ** -10, device=cuda_device)
    o2 = FusedAdam(m2.parameters(), lr=lr, amsgrad=True)
    sched = torch.optim.lr_scheduler.ExponentialLR(o2, gamma=0.5)
    tr = CapturedTrainer(m2, o2, loss_fn, store, B, *caps)
    for k, ids in enumerate(steps):
        o1.param_groups[0]["lr"] = 2.0 ** -(10 + k)  # exact in fp32
        _eager_epoch(m1, o1, loss_fn, store, [ids], B, caps)
        tr.step(ids)
        sched.step()
        assert o2.param_groups[0]["lr"] is lr       # updated in place: the replays see it
        torch.cuda.synchronize()
        assert float(lr) == 2.0 ** -(11 + k)
        _assert_same_training_state(m1, o1, m2, o2)
    assert tr.fallbacks == 0


# -- (f) what it refuses ---------------------------------------------------------------------------

def test_mean_reduction_and_ddp_hook_are_refused(epoch, cuda_device):
    b, store, _ = epoch
    m = _model(b.x.shape[1], cuda_device)
    opt = FusedAdam(m.parameters(), lr=1e-3, amsgrad=True)
    for loss_fn in (MSELoss("mean"), torch.nn.MSELoss(reduction="mean"), MSELoss()):
        with pytest.raises(ValueError, match="sum"):
            CapturedTrainer(m, opt, loss_fn, store, 8)
    m._grad_bucket_hook = lambda flat, buckets, events: None
    with pytest.raises(NotImplementedError, match="DDP"):
        CapturedTrainer(m, opt, MSELoss("sum"), store, 8)
    m._grad_bucket_hook = None
    tr = CapturedTrainer(m, opt, torch.nn.MSELoss(reduction="sum"), store, 8)
    with pytest.raises(ValueError):
        tr.step(np.arange(9))                       # more ids than slots
    with pytest.raises(IndexError):
        tr.step([0, 44])
