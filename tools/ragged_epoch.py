"""One training epoch over ragged batches: the eager store.collate loop against CapturedTrainer.

Workload: a synthetic ragged store at cfg2 widths (F 846, Fe 14, H 400, D 4, batch 256); the
epoch's ids are fixed (seeded) and grouped by size within windows, the way a length-bucketed
sampler batches, so the batches differ by well over 10 % in E.  Legs, each with its own model
(same init), FusedAdam(amsgrad) and the native MSELoss("sum"):

  eager            store.collate(ids) -> forward -> loss -> backward -> step, loss accumulated on
                   the device (one sync per epoch)
  eager_item       the same with trainer.py:142-150's loss.item() per batch
  captured_full    CapturedTrainer at store.padded_caps(batch)
  captured_tight   CapturedTrainer at the --quantile of the epoch's batch sizes (plus room for
                   the pad graph); batches above it fall back to the eager step

Timing: a window is --epochs epochs back to back ending in one synchronize (host clock); after
--warmup untimed windows per leg, --repeats windows per leg are taken with the legs alternating,
and the median, min, max and spread ((max - min) / median) are reported.  `--legs eager,eager_item`
needs nothing but GraphStore.collate, so the same script gives the baseline on an older checkout
of the package (--pkg).  Writes one JSON object (--out, default stdout only).
"""

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--n-atoms", type=int, default=30)
    ap.add_argument("--jitter", type=int, default=10)
    ap.add_argument("--n-mace", type=int, default=768)
    ap.add_argument("--hidden", type=int, default=400)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--bucket", type=int, default=512, help="ids are size-sorted within "
                    "windows of this many graphs of the seeded permutation")
    ap.add_argument("--quantile", type=float, default=0.75)
    ap.add_argument("--epochs", type=int, default=10, help="epochs per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--legs", default="eager,eager_item,captured_full,captured_tight")
    ap.add_argument("--pkg", default=os.path.join(REPO, "cgr-mpnn-3d_amd"),
                    help="directory holding the cgr_mpnn_3D package to measure")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.pkg)

    import numpy as np
    import torch

    from cgr_mpnn_3D._amd.data import GraphStore
    from cgr_mpnn_3D._amd.loss import MSELoss
    from cgr_mpnn_3D._amd.optim import FusedAdam
    from cgr_mpnn_3D._amd.synth import make_batch
    from cgr_mpnn_3D.models.GNN import GNN

    if not torch.cuda.is_available():
        raise SystemExit("ragged_epoch: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    legs = [s for s in args.legs.split(",") if s]
    B, D, H = args.batch, args.depth, args.hidden

    b = make_batch(args.graphs, n_atoms=args.n_atoms, n_bonds=args.n_atoms, n_mace=args.n_mace,
                   seed=11, n_atoms_jitter=args.jitter)
    store = GraphStore.from_batch(b, dev)
    F_ = b.x.shape[1]
    perm = np.random.default_rng(5).permutation(args.graphs)
    ncount = np.diff(b.ptr)
    for w0 in range(0, args.graphs, args.bucket):
        win = perm[w0:w0 + args.bucket]
        perm[w0:w0 + args.bucket] = win[np.argsort(ncount[win], kind="stable")]
    batches = [perm[i:i + B] for i in range(0, args.graphs, B)]
    order = np.random.default_rng(6).permutation(len(batches))
    batches = [batches[i] for i in order]
    full = [np.resize(x, B) if len(x) < B else x for x in batches]
    sizes = np.array([store.batch_sizes(x) for x in full])
    n_rxn = sum(len(x) for x in batches)
    del b

    def model_opt():
        torch.manual_seed(0)
        m = GNN(F_, 14, depth=D, hidden_sizes=[H] * D, dropout_ps=[0.0] * D).to(dev).train()
        return m, FusedAdam(m.parameters(), lr=1e-4, amsgrad=True)

    loss_fn = MSELoss("sum")
    runs, extra = {}, {}

    def eager_leg(item):
        m, opt = model_opt()
        total = torch.zeros((), device=dev)

        def epoch():
            for ids in batches:
                pb = store.collate(ids)
                opt.zero_grad(set_to_none=True)
                loss = loss_fn(m(pb), pb.y)
                loss.backward()
                opt.step()
                if item:
                    loss.item()
                else:
                    total.add_(loss.detach())
            if not item:
                total.item()
                total.zero_()
        return epoch

    def captured_leg(caps, name):
        from cgr_mpnn_3D._amd.captured import CapturedTrainer

        m, opt = model_opt()
        tr = CapturedTrainer(m, opt, loss_fn, store, B, *caps)
        fits = [store.fits(x, *caps) for x in full]
        extra[name] = dict(
            node_cap=int(caps[0]), edge_cap=int(caps[1]),
            fallbacks_per_epoch=int(len(fits) - sum(fits)),
            pad_overhead_nodes=round(float(np.mean(
                [caps[0] / n for (n, _), f in zip(sizes, fits) if f] or [1.0])), 4),
            pad_overhead_edges=round(float(np.mean(
                [caps[1] / e for (_, e), f in zip(sizes, fits) if f] or [1.0])), 4))

        def epoch():
            for ids in batches:
                tr.step(ids)
            tr.epoch_loss()
        epoch.trainer = tr
        return epoch

    fns = {}
    for leg in legs:
        if leg in ("eager", "eager_item"):
            fns[leg] = eager_leg(leg == "eager_item")
        elif leg == "captured_full":
            fns[leg] = captured_leg(store.padded_caps(B), leg)
        elif leg == "captured_tight":
            q_n = int(np.quantile(sizes[:, 0], args.quantile))
            q_e = int(np.quantile(sizes[:, 1], args.quantile))
            e_cap = q_e + (q_e & 1)
            # room for a pad graph whose in-degree stays within the bound (pairs <= 2 P) for
            # every batch below the quantile
            need = [n - (-(e_cap - e) // 4) for n, e in sizes if n <= q_n and e <= e_cap]
            n_cap = max([q_n + 2] + [int(v) for v in need])
            fns[leg] = captured_leg((n_cap, e_cap), leg)
        else:
            raise SystemExit(f"unknown leg {leg!r}")

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.epochs):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for leg in legs:
        for _ in range(args.warmup):
            window(fns[leg])
        runs[leg] = []
    for _ in range(args.repeats):
        for leg in legs:                       # alternate the legs: drift hits all of them alike
            runs[leg].append(window(fns[leg]))

    steps = args.epochs * len(batches)
    out = dict(
        workload=dict(graphs=args.graphs, batch=B, batches_per_epoch=len(batches), F=F_, Fe=14,
                      H=H, D=D, n_atoms=args.n_atoms, jitter=args.jitter, bucket=args.bucket,
                      N_min=int(sizes[:, 0].min()), N_max=int(sizes[:, 0].max()),
                      E_min=int(sizes[:, 1].min()), E_max=int(sizes[:, 1].max()),
                      E_max_over_min=round(float(sizes[:, 1].max() / sizes[:, 1].min()), 3),
                      epochs_per_window=args.epochs, warmup_windows=args.warmup,
                      repeats=args.repeats),
        device=torch.cuda.get_device_name(0), legs={})
    for leg in legs:
        t = np.array(runs[leg])
        medn = float(np.median(t))
        rec = dict(ms_per_step=round(medn / steps * 1e3, 4),
                   ms_per_step_min=round(float(t.min()) / steps * 1e3, 4),
                   ms_per_step_max=round(float(t.max()) / steps * 1e3, 4),
                   spread=round(float((t.max() - t.min()) / medn), 4),
                   reactions_per_s=round(args.epochs * n_rxn / medn, 1))
        rec.update(extra.get(leg, {}))
        tr = getattr(fns[leg], "trainer", None)
        if tr is not None:
            windows = args.warmup + args.repeats
            rec["fallbacks_counted"] = tr.fallbacks
            assert tr.fallbacks == rec["fallbacks_per_epoch"] * args.epochs * windows
        out["legs"][leg] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
