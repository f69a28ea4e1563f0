"""Native L1Loss and HuberLoss (cgr_l1_loss_* / cgr_huber_loss_*, csrc/loss.hip) against
torch.nn.L1Loss / torch.nn.HuberLoss.

Forward: against torch's loss of the same fp32 inputs evaluated in fp64, at relative error
(ceil(n / 256) + 10) 2^-24: one workgroup of 256 threads adds ceil(n / 256) non-negative fp32
terms per thread in a fixed order, then a 6-level wave tree and the 4 wave sums; the remaining
roundings are the term itself and the mean's scale.  Gradients: test_gpu_loss.py's bars (rtol 1e-6,
atol 1e-7).
"""

import math

import pytest
import torch

from cgr_mpnn_3D._amd.loss import HuberLoss, L1Loss

pytestmark = pytest.mark.gpu

NS = [1, 7, 256, 1000, 70001]
KINDS = [("l1", None), ("huber", 0.5), ("huber", 1.0)]


def _pair(kind, delta, reduction):
    if kind == "l1":
        return L1Loss(reduction), torch.nn.L1Loss(reduction=reduction)
    return HuberLoss(reduction, delta=delta), torch.nn.HuberLoss(reduction=reduction, delta=delta)


@pytest.fixture(scope="module")
def inputs():
    """y = 3 randn against t = randn per n (both Huber branches occur), with a few entries where
    y == t exactly (the L1 gradient is 0 there).  Host tensors, shared and left unchanged."""
    out = {}
    for n in NS:
        g = torch.Generator().manual_seed(n)
        y = torch.randn(n, generator=g) * 3
        t = torch.randn(n, generator=g)
        for i in range(1, n, max(2, n // 5)):  # n = 1 keeps its one term
            t[i] = y[i]
        d = (y - t).abs()
        if n >= 256:
            assert bool((d == 0).any()) and bool((d > 1.0).any())
            assert bool(((d > 0) & (d < 0.5)).any())
        out[n] = (y, t)
    return out


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("kind,delta", KINDS)
def test_robust_loss_matches_torch(kind, delta, reduction, n, inputs, cuda_device):
    y0, t0 = inputs[n]
    y = y0.to(cuda_device).requires_grad_(True)
    t = t0.to(cuda_device).requires_grad_(True)
    y2 = y.detach().clone().requires_grad_(True)
    t2 = t.detach().clone().requires_grad_(True)
    ours_fn, ref_fn = _pair(kind, delta, reduction)
    ours = ours_fn(y, t)
    ref = ref_fn(y2, t2)
    ref64 = float(ref_fn(y0.double(), t0.double()))
    assert ours.shape == ref.shape == torch.Size([]) and ours.dtype == torch.float32
    bound = (math.ceil(n / 256) + 10) * 2.0 ** -24
    got = float(ours.detach())
    err = abs(got - ref64) / abs(ref64)
    print(f"{kind} delta={delta} {reduction} n={n}: ours {got!r} fp64 {ref64!r} "
          f"rel err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    (ours * 1.5).backward()
    (ref * 1.5).backward()
    assert torch.allclose(y.grad, y2.grad, rtol=1e-6, atol=1e-7)
    assert torch.allclose(t.grad, t2.grad, rtol=1e-6, atol=1e-7)
    if kind == "l1" and n > 1:
        same = y0 == t0
        assert bool((y.grad.cpu()[same] == 0).all()) and bool((t.grad.cpu()[same] == 0).all())


def test_gradient_only_for_the_side_that_asks(cuda_device):
    y = torch.randn(300, device=cuda_device, requires_grad=True)
    t = torch.randn(300, device=cuda_device)
    HuberLoss("sum", delta=0.7)(y, t).backward()
    d = (y - t).detach()
    torch.testing.assert_close(y.grad, d.clamp(-0.7, 0.7), rtol=1e-6, atol=1e-7)
    assert t.grad is None
    t.requires_grad_(True)
    L1Loss("mean")(y.detach(), t).backward()
    torch.testing.assert_close(t.grad, -torch.sign(d) / 300, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("fn", [L1Loss("sum"), HuberLoss("sum", delta=0.5)],
                         ids=["l1", "huber"])
def test_robust_losses_deterministic_and_capturable(fn, cuda_device):
    y = (torch.randn(256, device=cuda_device) * 2).requires_grad_(True)
    t = torch.randn(256, device=cuda_device)
    a = fn(y, t).item()
    assert all(fn(y, t).item() == a for _ in range(3))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn(y, t).backward()
    torch.cuda.current_stream().wait_stream(s)
    expect = y.grad / 2  # two eager backwards accumulated
    gr = torch.cuda.CUDAGraph()
    y.grad = None
    with torch.cuda.graph(gr):
        loss = fn(y, t)
        loss.backward()
    y.grad.zero_()
    gr.replay()
    torch.cuda.synchronize()
    assert loss.item() == a
    assert torch.equal(y.grad, expect)


def test_robust_losses_reject_mismatch(cuda_device):
    for fn in (L1Loss("sum"), HuberLoss("sum")):
        with pytest.raises(ValueError):
            fn(torch.zeros(4, device=cuda_device), torch.zeros(4, 1, device=cuda_device))
        with pytest.raises(TypeError):
            fn(torch.zeros(4, device=cuda_device, dtype=torch.float64),
               torch.zeros(4, device=cuda_device, dtype=torch.float64))
