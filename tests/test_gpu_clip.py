"""FusedAdam(max_grad_norm=...): global L2 gradient-norm clipping inside the fused step
(cgr_grad_sumsq + cgr_adam_step_clip, csrc/optim.hip) against
``torch.nn.utils.clip_grad_norm_`` followed by ``torch.optim.Adam.step`` on clones.

The optimizer bars are test_gpu_optim.py's (rtol 1e-5, atol 1e-6).  The norm is compared with the
fp64 norm of the same gradients at rtol 1e-5: a block sums 4 squares per thread, a 64-lane tree and
4 wave sums in fp32 (~10 roundings of 2^-24 on non-negative terms), the final sum runs in double
and the square root halves the relative error: a few 1e-7 derived, 1e-5 asserted.
"""

import copy

import numpy as np
import pytest
import torch

from cgr_mpnn_3D._amd.captured import CapturedTrainer
from cgr_mpnn_3D._amd.data import GraphStore
from cgr_mpnn_3D._amd.loss import HuberLoss
from cgr_mpnn_3D._amd.optim import FusedAdam
from cgr_mpnn_3D._amd.synth import make_batch
from cgr_mpnn_3D.models.GNN import GNN

pytestmark = pytest.mark.gpu

# test_gpu_optim.py's list: a 0-dim tensor, 1-element tensors, 1001 elements, 400 x 860
SHAPES = [(400, 860), (400,), (400, 400), (1, 400), (1,), (7, 3), (1001,), ()]
BLOCK = 1024  # elements per block of the step kernel (one float4 per thread, 256 threads)
STATE = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def _tensors(dev, shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(dev).requires_grad_() for s in shapes]


def _norm64(grads):
    """fp64 global L2 norm of the gradients that are not None."""
    return float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads if g is not None)))


def _assert_same(opt, ps, ref, ps_ref, amsgrad=True):
    for a, b in zip(ps, ps_ref):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-5, atol=1e-6)
        sa, sb = opt.state[a], ref.state[b]
        for k in STATE[:3 if amsgrad else 2]:
            torch.testing.assert_close(sa[k], sb[k], rtol=1e-5, atol=1e-6)


@pytest.fixture(scope="module")
def six_steps():
    """The six gradient sets of the clipped-step test (randn * (1 + it), on the host) and their
    fp64 norms; shared by every parametrisation and left unchanged."""
    g = torch.Generator().manual_seed(1)
    grads = [[torch.randn(s, generator=g) * (1 + it) for s in SHAPES] for it in range(6)]
    return grads, [_norm64(gs) for gs in grads]


@pytest.mark.parametrize("amsgrad,wd,maximize", [(True, 0.0, False), (True, 1e-2, False),
                                                 (False, 0.0, False), (True, 0.0, True)])
def test_clipped_steps_match_clip_grad_norm_then_adam(amsgrad, wd, maximize, six_steps,
                                                      cuda_device):
    host_grads, norms = six_steps
    max_norm = 0.5 * (norms[2] + norms[3])  # between the norms of steps 2 and 3
    clipped = [n > max_norm for n in norms]
    assert any(clipped) and not all(clipped), norms
    ps_ref = _tensors(cuda_device, SHAPES, 0)
    ps = [p.detach().clone().requires_grad_() for p in ps_ref]
    ref = torch.optim.Adam(ps_ref, lr=3e-3, weight_decay=wd, amsgrad=amsgrad, maximize=maximize)
    opt = FusedAdam(ps, lr=3e-3, weight_decay=wd, amsgrad=amsgrad, maximize=maximize,
                    max_grad_norm=max_norm)
    assert opt.grad_norm.shape == torch.Size([]) and opt.grad_norm.dtype == torch.float32
    norm_ptr = opt.grad_norm.data_ptr()
    for it in range(6):
        for p, q, gr in zip(ps, ps_ref, host_grads[it]):
            p.grad = gr.to(cuda_device)
            q.grad = gr.to(cuda_device)
        before = [p.grad.clone() for p in ps]
        opt.step()
        torch.nn.utils.clip_grad_norm_(ps_ref, max_norm, norm_type=2.0)
        ref.step()
        got = float(opt.grad_norm)
        print(f"step {it}: norm {got!r} fp64 {norms[it]!r} rel "
              f"{abs(got - norms[it]) / norms[it]:.2e} clipped={clipped[it]}")
        assert abs(got - norms[it]) <= 1e-5 * norms[it]
        assert opt.grad_norm.data_ptr() == norm_ptr  # static storage
        for p, g0 in zip(ps, before):  # p.grad is left unscaled (torch scales it in place)
            assert torch.equal(p.grad, g0)
    assert int(opt.skipped_steps) == 0
    _assert_same(opt, ps, ref, ps_ref, amsgrad)
    for p in ps:
        assert float(opt.state[p]["step"]) == 6.0


def test_many_tensors_odd_offsets_missing_grad_and_block_edges(cuda_device):
    # 70 tiny tensors + one 64 x 64 (> CGR_ADAM_GROUP tensors: several launches of both kernels),
    # a tensor of exactly one block and one of one element more; the gradients are views at odd
    # offsets of one flat buffer (the native backward's bucket layout): the scalar path
    shapes = [(3 + i % 5,) for i in range(70)] + [(64, 64), (BLOCK,), (BLOCK + 1,)]
    ps_ref = _tensors(cuda_device, shapes, 2)
    ps = [p.detach().clone().requires_grad_() for p in ps_ref]
    total = sum(p.numel() for p in ps)
    gen = torch.Generator().manual_seed(4)
    flats = [torch.randn(total + 1, generator=gen) * s for s in (1.0, 3.0, 0.5, 2.0)]
    norms = []
    for it, f in enumerate(flats):  # step 2 leaves ps[5].grad None
        off, parts = 1, []
        for i, p in enumerate(ps):
            parts.append(None if (it == 2 and i == 5) else f[off:off + p.numel()])
            off += p.numel()
        norms.append(_norm64(parts))
    max_norm = 0.5 * (sorted(norms)[1] + sorted(norms)[2])
    ref = torch.optim.Adam(ps_ref, lr=1e-2, amsgrad=True)
    opt = FusedAdam(ps, lr=1e-2, amsgrad=True, max_grad_norm=max_norm)
    for it, f in enumerate(flats):
        flat = f.to(cuda_device)
        off = 1  # every view starts at an odd element of the flat buffer or right after one
        for i, (p, q) in enumerate(zip(ps, ps_ref)):
            n = p.numel()
            p.grad = flat[off:off + n].view(p.shape)
            q.grad = p.grad.clone()
            off += n
            if it == 2 and i == 5:
                p.grad = q.grad = None
        assert any(p.grad is not None and p.grad.data_ptr() % 16 for p in ps)
        opt.step()
        torch.nn.utils.clip_grad_norm_(ps_ref, max_norm, norm_type=2.0)
        ref.step()
        got = float(opt.grad_norm)
        assert abs(got - norms[it]) <= 1e-5 * norms[it], (it, got, norms[it])
    assert sum(n > max_norm for n in norms) == 2
    _assert_same(opt, ps, ref, ps_ref)


def test_two_param_groups_share_one_norm_and_clip_separately(cuda_device):
    shapes_a, shapes_b = [(300, 7), (5,), ()], [(BLOCK + 1,), (33, 3)]
    ra, rb = _tensors(cuda_device, shapes_a, 6), _tensors(cuda_device, shapes_b, 7)
    pa = [p.detach().clone().requires_grad_() for p in ra]
    pb = [p.detach().clone().requires_grad_() for p in rb]
    gen = torch.Generator().manual_seed(8)
    steps = [[torch.randn(p.shape, generator=gen) * s for p in pa + pb] for s in (0.2, 5.0, 1.0)]
    norms = [_norm64(gs) for gs in steps]
    max_norm = 0.5 * (norms[0] + norms[2])
    assert norms[0] < max_norm < norms[2] < norms[1]
    ref = torch.optim.Adam([dict(params=ra), dict(params=rb, lr=3e-3)], lr=1e-2, amsgrad=True)
    opt = FusedAdam([dict(params=pa, max_grad_norm=max_norm), dict(params=pb, lr=3e-3)],
                    lr=1e-2, amsgrad=True)
    assert opt.param_groups[1]["max_grad_norm"] is None
    for gs, n64 in zip(steps, norms):
        for p, q, g in zip(pa + pb, ra + rb, gs):
            p.grad = g.to(cuda_device)
            q.grad = g.to(cuda_device)
        opt.step()
        # torch: the global norm of both groups, applied to the group that clips only
        total = torch.nn.utils.get_total_norm([q.grad for q in ra + rb], norm_type=2.0)
        torch.nn.utils.clip_grads_with_norm_(ra, max_norm, total)
        ref.step()
        assert abs(float(opt.grad_norm) - n64) <= 1e-5 * n64
    _assert_same(opt, pa + pb, ref, ra + rb)


def _run(dev, max_grad_norm, grads, shapes, seed=0, **kw):
    ps = _tensors(dev, shapes, seed)
    opt = FusedAdam(ps, lr=3e-3, amsgrad=True, max_grad_norm=max_grad_norm, **kw)
    norms = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.to(dev)
        opt.step()
        if opt.grad_norm is not None:
            norms.append(opt.grad_norm.clone())
    return ps, opt, norms


def test_same_gradients_give_the_same_bits(six_steps, cuda_device):
    grads, norms64 = six_steps
    a = _run(cuda_device, norms64[1], grads[:3], SHAPES)
    b = _run(cuda_device, norms64[1], grads[:3], SHAPES)
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)
    for p, q in zip(a[0], b[0]):
        assert torch.equal(p, q)
        for k in STATE:
            assert torch.equal(a[1].state[p][k], b[1].state[q][k])


def test_infinite_bound_measures_and_never_clips(six_steps, cuda_device):
    grads, norms64 = six_steps
    ps, opt, norms = _run(cuda_device, float("inf"), grads[:3], SHAPES, weight_decay=1e-2)
    qs, plain, none = _run(cuda_device, None, grads[:3], SHAPES, weight_decay=1e-2)
    assert none == [] and plain.grad_norm is None
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)  # bitwise the unclipped FusedAdam
        for k in STATE + ("step",):
            assert torch.equal(opt.state[p][k], plain.state[q][k])
    for got, n64 in zip(norms, norms64):
        assert abs(float(got) - n64) <= 1e-5 * n64
    assert int(opt.skipped_steps) == 0


def test_non_finite_gradient_skips_the_step(cuda_device):
    shapes = [(40, 9), (BLOCK + 5,), (), (3,)]
    gen = torch.Generator().manual_seed(11)
    steps = [[torch.randn(s, generator=gen) * (1 + it) for s in shapes] for it in range(4)]
    norms = [_norm64(gs) for gs in steps]
    max_norm = 0.5 * (norms[1] + norms[2])
    ps_ref = _tensors(cuda_device, shapes, 12)
    ps = [p.detach().clone().requires_grad_() for p in ps_ref]
    ref = torch.optim.Adam(ps_ref, lr=1e-2, amsgrad=True, weight_decay=1e-3)
    opt = FusedAdam(ps, lr=1e-2, amsgrad=True, weight_decay=1e-3, max_grad_norm=max_norm)

    def both(gs):
        for p, q, g in zip(ps, ps_ref, gs):
            p.grad = g.to(cuda_device)
            q.grad = g.to(cuda_device)
        opt.step()
        torch.nn.utils.clip_grad_norm_(ps_ref, max_norm, norm_type=2.0)
        ref.step()

    both(steps[0])
    both(steps[1])
    saved = [(p.detach().clone(), {k: v.clone() for k, v in opt.state[p].items()}) for p in ps]
    bad = [g.clone() for g in steps[2]]
    bad[1][BLOCK + 4] = float("inf")  # one inf, in the scalar tail of the second block
    for p, g in zip(ps, bad):
        p.grad = g.to(cuda_device)
    opt.step()  # the reference never sees this step
    assert int(opt.skipped_steps) == 1
    assert not bool(torch.isfinite(opt.grad_norm))
    for p, (p0, st0) in zip(ps, saved):
        assert torch.equal(p.detach(), p0)
        for k in STATE + ("step",):
            assert torch.equal(opt.state[p][k], st0[k]), k
    both(steps[2])
    both(steps[3])
    assert int(opt.skipped_steps) == 1
    assert abs(float(opt.grad_norm) - norms[3]) <= 1e-5 * norms[3]
    _assert_same(opt, ps, ref, ps_ref)
    for p in ps:
        assert float(opt.state[p]["step"]) == 4.0


# -- capture ----------------------------------------------------------------------------------------

def test_clipped_training_step_graph_capture(cuda_device):
    """test_gpu_optim.py's captured training step (16 reactions, H = 64, D = 2, dropout 0) with
    clipping active: the replays continue the eager sequence, and grad_norm follows them."""
    b = make_batch(16, n_mace=32, seed=71)
    data = b.to_torch(cuda_device)
    loss_fn = torch.nn.MSELoss(reduction="sum")

    def build(max_norm):
        torch.manual_seed(0)
        m = GNN(b.x.shape[1], 14, depth=2, hidden_sizes=[64] * 2, dropout_ps=[0.0] * 2)
        m = m.to(cuda_device).train()
        return m, FusedAdam(m.parameters(), lr=1e-3, amsgrad=True, max_grad_norm=max_norm)

    def step(m, opt):
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(m(data), data.y)
        loss.backward()
        opt.step()
        return loss.detach()

    # the bound: half the first step's norm, so the early steps at least are clipped
    m0, o0 = build(float("inf"))
    step(m0, o0)
    max_norm = 0.5 * float(o0.grad_norm)
    assert np.isfinite(max_norm) and max_norm > 0

    m1, o1 = build(max_norm)
    eager, eager_norms = [], []
    for _ in range(8):
        eager.append(step(m1, o1).item())
        eager_norms.append(float(o1.grad_norm))
    assert max(eager_norms) > max_norm  # clipping was active

    m2, o2 = build(max_norm)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        warm = [step(m2, o2).item() for _ in range(3)]
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        gl = step(m2, o2)
    replayed, replayed_norms = [], []
    for _ in range(5):
        gr.replay()
        replayed.append(gl.item())
        replayed_norms.append(float(o2.grad_norm))
    assert warm == eager[:3]
    torch.testing.assert_close(torch.tensor(replayed), torch.tensor(eager[3:]), rtol=1e-6,
                               atol=0)
    torch.testing.assert_close(torch.tensor(replayed_norms), torch.tensor(eager_norms[3:]),
                               rtol=1e-6, atol=0)
    for a, c in zip(m1.parameters(), m2.parameters()):
        torch.testing.assert_close(a, c, rtol=1e-6, atol=1e-7)
    assert int(o2.skipped_steps) == 0


def test_captured_trainer_epoch_with_clipping_and_huber(cuda_device):
    b = make_batch(20, n_atoms=10, n_bonds=12, n_mace=3, seed=22, n_atoms_jitter=3)
    store = GraphStore.from_batch(b, cuda_device)
    torch.manual_seed(0)
    m = GNN(b.x.shape[1], 14, depth=2, hidden_sizes=[48] * 2, dropout_ps=[0.0] * 2)
    m = m.to(cuda_device).train()
    before = [p.detach().clone() for p in m.parameters()]
    opt = FusedAdam(m.parameters(), lr=1e-3, amsgrad=True, max_grad_norm=1.0)
    tr = CapturedTrainer(m, opt, HuberLoss("sum"), store, 8)
    for ids in (np.arange(0, 8), np.arange(8, 16), np.arange(16, 20)):  # the last batch is short
        tr.step(ids)
    assert tr.fallbacks == 0
    total = tr.epoch_loss()
    assert np.isfinite(total) and total > 0
    assert np.isfinite(float(opt.grad_norm)) and float(opt.grad_norm) > 0
    assert int(opt.skipped_steps) == 0
    assert any(not torch.equal(p.detach(), q) for p, q in zip(m.parameters(), before))
    tr.close()
