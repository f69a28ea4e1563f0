#!/usr/bin/env python3
"""What the mean-variance head costs: a cfg2 eager training step (forward, loss, backward,
FusedAdam) with ``ffn = MeanVarianceHead(H)`` and the native ``GaussianNLLLoss("sum")`` against
the same model with the head and the loss composed in torch on ``GNN.encode`` (two Linears,
softplus, cat, ``torch.nn.GaussianNLLLoss``), and against the fused ``Linear(H, 1)`` + native
``MSELoss("sum")`` step, on the same batch and initial weights.  Steps timed with device events
around each, after a warm-up; the legs alternate in blocks so clock drift hits all of them, and
every leg's median over block medians is printed with the min-max spread over blocks.  The head's
and the loss's own launches are timed alone as well (device events around a run of calls).  No
threshold: the figures go into DESIGN.md section 9.

    python tools/uncertainty_price.py [--config cfg2] [--blocks 5] [--steps 30]
"""

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "cgr-mpnn-3d_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from cgr_mpnn_3D._amd.loss import GaussianNLLLoss, MSELoss  # noqa: E402
from cgr_mpnn_3D._amd.optim import FusedAdam  # noqa: E402
from cgr_mpnn_3D._amd.synth import CONFIGS, make_batch  # noqa: E402
from cgr_mpnn_3D.models.GNN import GNN, MeanVarianceHead  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup-ms", type=float, default=300.0)
    args = ap.parse_args()
    c = CONFIGS[args.config]
    dev = torch.device("cuda:0")
    b = make_batch(c["num_graphs"], c["n_atoms"], c["n_bonds"], c["n_mace"], seed=1)
    D, H = c["depth"], c["hidden"]
    data = b.to_torch(dev)

    def model():
        torch.manual_seed(0)
        return GNN(b.x.shape[1], 14, depth=D, hidden_sizes=[H] * D, dropout_ps=[0.0] * D,
                   use_learnable_skip=c["learnable_skip"]).to(dev).train()

    m_nat, m_tor, m_fus = model(), model(), model()
    m_nat.ffn = MeanVarianceHead(H).to(dev)
    mean, var = torch.nn.Linear(H, 1).to(dev), torch.nn.Linear(H, 1).to(dev)
    mean.load_state_dict(m_nat.ffn.mean.state_dict())
    var.load_state_dict(m_nat.ffn.var.state_dict())
    min_var = m_nat.ffn.min_var
    p_nat = list(m_nat.parameters())
    p_tor = [p for k, p in m_tor.named_parameters() if not k.startswith("ffn.")] + \
        list(mean.parameters()) + list(var.parameters())
    p_fus = list(m_fus.parameters())
    o_nat, o_tor, o_fus = (FusedAdam(p, lr=1e-4) for p in (p_nat, p_tor, p_fus))
    nll_nat, nll_tor, mse = GaussianNLLLoss(reduction="sum"), \
        torch.nn.GaussianNLLLoss(reduction="sum"), MSELoss("sum")

    def finish(loss, params, opt):
        for p, g in zip(params, torch.autograd.grad(loss, params)):
            p.grad = g
        opt.step()

    def native():
        finish(nll_nat(m_nat(data), data.y), p_nat, o_nat)

    def composed():
        g = m_tor.encode(data)
        mu = mean(g).squeeze(-1)
        v = torch.nn.functional.softplus(var(g)).squeeze(-1) + min_var
        finish(nll_tor(mu, data.y, v), p_tor, o_tor)

    def fused():
        finish(mse(m_fus(data), data.y), p_fus, o_fus)

    def timed(fn, reps=1):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        z.record()
        z.synchronize()
        return a.elapsed_time(z) / reps

    legs = (("native", native), ("composed", composed), ("fused", fused))
    for _, fn in legs:  # warm-up: lazy streams, allocator, clocks
        spent = 0.0
        while spent < args.warmup_ms:
            spent += timed(fn)
    med = {name: [] for name, _ in legs}
    for _ in range(args.blocks):
        for name, fn in legs:
            med[name].append(statistics.median(timed(fn) for _ in range(args.steps)))
    out = {"config": args.config, "blocks": args.blocks, "steps_per_block": args.steps}
    for name, v in med.items():
        out[name + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    out["native_over_composed"] = out["native_ms"]["median"] / out["composed_ms"]["median"]
    out["native_over_fused"] = out["native_ms"]["median"] / out["fused_ms"]["median"]

    # the head and the loss alone on the step's own shapes: a run of calls between two events
    # (launch rate included: what an eager step sees)
    with torch.no_grad():
        g = m_nat.encode(data)
    g = g.clone().requires_grad_(True)
    head = m_nat.ffn
    out2 = head(g)
    dout = torch.randn_like(out2)
    leaf = out2.detach().clone().requires_grad_(True)
    loss = nll_nat(leaf, data.y)

    def head_fwd():
        with torch.no_grad():
            head(g)

    def head_bwd():
        torch.autograd.grad(out2, [g] + list(head.parameters()), dout, retain_graph=True)

    def loss_fwd():
        with torch.no_grad():
            nll_nat(leaf, data.y)

    def loss_bwd():
        torch.autograd.grad(loss, [leaf], retain_graph=True)

    for name, fn in (("head_forward_us", head_fwd), ("head_backward_us", head_bwd),
                     ("nll_forward_us", loss_fwd), ("nll_backward_us", loss_bwd)):
        timed(fn, 20)
        out[name] = statistics.median(timed(fn, 50) for _ in range(5)) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
