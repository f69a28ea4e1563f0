"""The per-step cost of FusedAdam(max_grad_norm=...) at cfg2: bench.py's captured step built twice
in one process (same init, same batch), without and with clipping, replayed in alternating blocks.
Also the eager step both ways.  Prints one JSON line; ``--out PATH`` also writes it to a file
(the record in DESIGN.md §9 is profiles/clip_cost_cfg2.json)."""

import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "cgr-mpnn-3d_amd")):
    sys.path.insert(0, p)

from cgr_mpnn_3D._amd.loss import MSELoss  # noqa: E402
from cgr_mpnn_3D._amd.optim import FusedAdam  # noqa: E402
from cgr_mpnn_3D._amd.synth import CONFIGS, make_batch  # noqa: E402
from cgr_mpnn_3D.models.GNN import GNN  # noqa: E402

BLOCK, ROUNDS, EAGER = 2000, 7, 300


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    c = CONFIGS["cfg2"]
    D, H = c["depth"], c["hidden"]
    b = make_batch(c["num_graphs"], c["n_atoms"], c["n_bonds"], c["n_mace"], seed=1234)
    data = b.to_torch(dev)
    loss_fn = MSELoss(reduction="sum")

    def build(max_grad_norm):
        torch.manual_seed(0)
        m = GNN(b.x.shape[1], 14, depth=D, hidden_sizes=[H] * D, dropout_ps=[0.02] * D,
                use_learnable_skip=c["learnable_skip"]).to(dev).train()
        opt = FusedAdam(m.parameters(), lr=1e-3, amsgrad=True, max_grad_norm=max_grad_norm)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(m(data), data.y)
            loss.backward()
            opt.step()
            return loss

        for _ in range(30):
            step()
        torch.cuda.synchronize()
        return m, opt, step

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            fn()
            if (i + 1) % 50 == 0:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    legs = {"plain": build(None), "clip": build(1.0)}
    nparam = sum(p.numel() for p in legs["clip"][0].parameters())
    eager = {k: [] for k in legs}
    for _ in range(5):
        for k, (_, _, step) in legs.items():
            eager[k].append(timed(step, EAGER))

    replay = {}
    for k, (_, _, step) in legs.items():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        replay[k] = g.replay
        timed(g.replay, 600)  # steady state before any timed block
    captured = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k in legs:
            captured[k].append(timed(replay[k], BLOCK))

    def summary(xs):
        return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs),
                    blocks=[round(x, 5) for x in xs])

    out = dict(config="cfg2", parameters=nparam, block_steps=BLOCK, rounds=ROUNDS,
               captured={k: summary(v) for k, v in captured.items()},
               eager={k: summary(v) for k, v in eager.items()},
               grad_norm=float(legs["clip"][1].grad_norm),
               skipped_steps=int(legs["clip"][1].skipped_steps))
    out["captured_delta_us"] = 1e3 * (out["captured"]["clip"]["median_ms"]
                                      - out["captured"]["plain"]["median_ms"])
    out["eager_delta_us"] = 1e3 * (out["eager"]["clip"]["median_ms"]
                                   - out["eager"]["plain"]["median_ms"])
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
