#!/usr/bin/env python3
"""What the attention readout costs: a cfg2 eager training step (forward, loss, backward,
FusedAdam) through GNN(pooling_fn=AttentionPool(H)) -- the native gated-softmax pool on
GNN.encode_nodes -- against the same step with the readout composed in torch exactly as
INTEGRATION.md section 5 writes it (a gate Linear, max, exp, index_add_, gather, divide,
index_add_ on the same encode_nodes), and against the fused add-pool step, on the same batch and
initial weights.  Steps timed with device events around each, after a warm-up; the legs alternate
in blocks so clock drift hits all of them, and every leg's median over block medians is printed
with the min-max spread over blocks.  The native pool's own launches are timed alone as well
(device events around a run of calls).  No threshold: the figures go into DESIGN.md section 9.

    python tools/attn_pool_price.py [--config cfg2] [--blocks 5] [--steps 30]
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

from cgr_mpnn_3D._amd.optim import FusedAdam  # noqa: E402
from cgr_mpnn_3D._amd.synth import CONFIGS, make_batch  # noqa: E402
from cgr_mpnn_3D.models.GNN import GNN, AttentionPool  # noqa: E402


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
    B = b.num_graphs

    def model(pool=None):
        torch.manual_seed(0)
        kw = {} if pool is None else {"pooling_fn": pool}
        return GNN(b.x.shape[1], 14, depth=D, hidden_sizes=[H] * D, dropout_ps=[0.0] * D,
                   use_learnable_skip=c["learnable_skip"], **kw).to(dev).train()

    m_nat = model(AttentionPool(H))
    m_tor, m_fus = model(), model()
    att = torch.nn.Linear(H, 1).to(dev)
    att.load_state_dict(m_nat.pooling_fn.gate.state_dict())
    p_nat = list(m_nat.parameters())
    p_tor = list(m_tor.parameters()) + list(att.parameters())
    p_fus = list(m_fus.parameters())
    o_nat, o_tor, o_fus = (FusedAdam(p, lr=1e-4) for p in (p_nat, p_tor, p_fus))

    def finish(pred, params, opt):
        loss = ((pred - data.y) ** 2).sum()
        for p, g in zip(params, torch.autograd.grad(loss, params)):
            p.grad = g
        opt.step()

    def native():
        finish(m_nat(data), p_nat, o_nat)

    def composed():  # INTEGRATION.md section 5, line for line
        hn = m_tor.encode_nodes(data)
        s = att(hn).squeeze(-1)
        e = torch.exp(s - s.max().detach())
        w = e / torch.zeros(B, device=e.device).index_add_(0, data.batch, e)[data.batch]
        g = torch.zeros(B, H, device=e.device).index_add_(0, data.batch, w[:, None] * hn)
        finish(m_tor.ffn(g).squeeze(-1), p_tor, o_tor)

    def fused():
        finish(m_fus(data), p_fus, o_fus)

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

    # the pool alone on the step's own shapes: a run of calls between two events (launch rate
    # included: what an eager step sees)
    with torch.no_grad():
        hn = m_nat.encode_nodes(data)
    hn = hn.clone().requires_grad_(True)
    pool = m_nat.pooling_fn
    dg = torch.randn(B, H, device=dev)
    g = pool(hn, data.batch, ptr=data.ptr)
    gate = list(pool.parameters())

    def pool_fwd():
        with torch.no_grad():
            pool(hn, data.batch, ptr=data.ptr)

    def pool_bwd():
        torch.autograd.grad(g, [hn] + gate, dg, retain_graph=True)

    for name, fn in (("pool_forward_us", pool_fwd), ("pool_backward_us", pool_bwd)):
        timed(fn, 20)
        out[name] = statistics.median(timed(fn, 50) for _ in range(5)) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
