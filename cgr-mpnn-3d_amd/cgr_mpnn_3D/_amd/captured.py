"""Captured training over ragged batches: one HIP graph replayed for every batch of an epoch.

The reference's loop (``training/trainer.py:138-150``) collates a batch, runs forward, loss,
backward and the optimizer, and reads ``loss.item()`` -- per batch.  On the MI355X path the device
part of that step is well under a millisecond, so the host's ~40 launches, its allocations and
the ``.item()`` sync dominate.  A captured graph removes them, but it freezes shapes and launch
arguments, and every ``GraphStore.collate(ids)`` batch has its own N and E.

``CapturedTrainer`` closes that gap with fixed-shape collation (``GraphStore.collate_padded``,
``cgr_collate_padded``): the batch is written into static tensors of capacities ``node_cap`` /
``edge_cap`` and the remainder is one pad graph whose loss weight is 0, so it adds an exact 0 to
every gradient.  The graph ids reach the device through one small async copy per
step; nothing else crosses the host/device boundary until ``epoch_loss()``.

    store = GraphStore.from_data_list(train_data, "cuda")
    lr = torch.tensor(1e-3, device="cuda")                       # device lr: the scheduler's
    opt = FusedAdam(model.parameters(), lr=lr, amsgrad=True)     # updates reach the replays
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.95)
    tr = CapturedTrainer(model, opt, MSELoss("sum"), store, batch_size=32)
    for epoch in range(epochs):
        for ids in batches(perm):            # host ints, len(ids) <= batch_size
            tr.step(ids)                     # no sync
        train_loss = tr.epoch_loss() / n_train        # the epoch's one sync
        val = torch.cat([tr.predict(ids).clone() for ids in val_batches])
        sched.step()

A batch that does not fit the capacities (or whose pad graph would exceed the pad-degree bound)
runs the same step eagerly on ``store.collate(ids)`` and is counted in ``fallbacks``.  There is
no non-native path: both forms run the HIP kernels.

The zero-weight slots leave the loss as ``loss_fn(pred * mask, y * mask)``, which needs a ``[B +
1]`` prediction and a loss term that is 0 at (0, 0).  A loss whose class sets ``pads_by_weight``
(``GaussianNLLLoss`` on a ``MeanVarianceHead`` model, ``[B + 1, 2]``) is called as ``loss_fn(pred,
y, weight=mask)`` instead: the native losses skip an element of weight 0.
"""

from __future__ import annotations

import numpy as np
import torch

from . import config as _config


class CapturedTrainer:
    RING = 4  # pinned staging buffers in flight

    def __init__(self, model, optimizer, loss_fn, store, batch_size, node_cap=None,
                 edge_cap=None, max_pad_degree=4):
        if getattr(loss_fn, "reduction", None) != "sum":
            raise ValueError(
                "CapturedTrainer needs a sum-reduction loss (train.py:120's "
                "MSELoss(reduction='sum')): a mean would divide by a count that includes the "
                "filler slots and the pad graph")
        if getattr(model, "_grad_bucket_hook", None) is not None or \
                _config.grad_bucket_hook is not None:
            raise NotImplementedError(
                "CapturedTrainer does not support a gradient-bucket hook (DDP): the collectives "
                "of a data-parallel step are not part of its captured graph")
        self.model, self.optimizer, self.loss_fn, self.store = model, optimizer, loss_fn, store
        self.batch_size = B = int(batch_size)
        caps = store.padded_caps(B)
        self.node_cap = int(node_cap) if node_cap is not None else caps[0]
        self.edge_cap = int(edge_cap) if edge_cap is not None else caps[1]
        self.max_pad_degree = int(max_pad_degree)
        self.fallbacks = 0
        dev = self.device = store.device
        # ids (int64) and slot weights (fp32) travel in one buffer: one H2D copy per step
        self._stage = torch.zeros(12 * B, dtype=torch.uint8, device=dev)
        self._ids = self._stage[:8 * B].view(torch.int64)
        self._w = self._stage[8 * B:].view(torch.float32)
        self._pinned = [torch.zeros(12 * B, dtype=torch.uint8).pin_memory()
                        for _ in range(self.RING)]
        self._pinned_np = [(p[:8 * B].view(torch.int64).numpy(),
                            p[8 * B:].view(torch.float32).numpy()) for p in self._pinned]
        self._events = [None] * self.RING
        self._slot = 0
        self._batch = store.alloc_padded(B, self.node_cap, self.edge_cap)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)  # the last step's loss
        self.loss_total = torch.zeros((), dtype=torch.float32, device=dev)
        self._pred = None  # static [B + 1] (+ the model's trailing dims), shaped at first predict
        self._train_graph = None
        self._predict_graph = None

    # -- staging ---------------------------------------------------------------------------------
    def _full_ids(self, ids):
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        n = int(ids.size)
        if not 1 <= n <= self.batch_size:
            raise ValueError(f"CapturedTrainer: 1 .. {self.batch_size} graph ids per step, "
                             f"got {n}")
        if ids.min() < 0 or ids.max() >= self.store.num_graphs:
            raise IndexError(f"graph id out of range [0, {self.store.num_graphs})")
        # a short batch (the last of an epoch) is filled with repeats at loss weight 0
        return ids, (np.resize(ids, self.batch_size) if n < self.batch_size else ids), n

    def _stage_ids(self, full, n):
        """One async H2D copy of the ids and slot weights through the pinned ring; waits only for
        the copy that last used this ring slot (RING steps ago), never for the device."""
        k = self._slot
        self._slot = (k + 1) % self.RING
        ev = self._events[k]
        if ev is not None:
            ev.synchronize()
        ids_h, w_h = self._pinned_np[k]
        ids_h[:] = full
        w_h[:n] = 1.0
        w_h[n:] = 0.0
        self._stage.copy_(self._pinned[k], non_blocking=True)
        if ev is None:
            ev = self._events[k] = torch.cuda.Event()
        ev.record()

    def _fits(self, full):
        return self.store.fits(full, self.node_cap, self.edge_cap, self.max_pad_degree)

    # -- the step, as captured (also the eager form of a padded step) ----------------------------
    def _collate_static(self):
        return self.store.collate_padded(None, self.node_cap, self.edge_cap, out=self._batch,
                                         ids_dev=self._ids, weight_dev=self._w)

    def _account(self, loss):
        loss = loss.detach()
        self.loss_total += loss
        self.loss.copy_(loss)

    def _padded_step(self):
        b = self._collate_static()
        self.optimizer.zero_grad(set_to_none=True)
        pred = self.model(b)
        if getattr(self.loss_fn, "pads_by_weight", False):
            # (a [B + 1, 2] output, and a term that is not 0 at (0, 0): GaussianNLLLoss)
            loss = self.loss_fn(pred, b.y, weight=b.mask)
        else:
            loss = self.loss_fn(pred * b.mask, b.y * b.mask)
        loss.backward()
        self.optimizer.step()
        self._account(loss)

    def _unpadded_step(self, ids):
        b = self.store.collate(ids)
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.loss_fn(self.model(b), b.y)
        loss.backward()
        self.optimizer.step()
        self._account(loss)

    def _padded_predict(self):
        b = self._collate_static()
        out = self.model(b)
        if self._pred is None:  # the first (eager warm-up) call: [B + 1], or [B + 1, 2] for a
            self._pred = torch.zeros_like(out)  # mean-variance head
        self._pred.copy_(out)

    # -- capture ---------------------------------------------------------------------------------
    def _snapshot(self):
        """What the eager warm-up steps change: parameters, optimizer state, the model's dropout
        counter and the loss accumulators.  Restored in place afterwards (the captured graph must
        see the same tensors), so capturing costs the training run no step."""
        opt = self.optimizer
        params = [p for g in opt.param_groups for p in g["params"]]
        saved_p = [p.detach().clone() for p in params]
        saved_s = {p: {k: v.clone() for k, v in opt.state[p].items() if torch.is_tensor(v)}
                   for p in params if p in opt.state}
        bufs = [self.loss, self.loss_total]
        counter = getattr(self.model, "_cgr_rng_counter", None)
        if counter is not None:
            bufs.append(counter)
        saved_b = [t.clone() for t in bufs]

        def restore():
            with torch.no_grad():
                for p, q in zip(params, saved_p):
                    p.copy_(q)
                for p in params:
                    for k, v in opt.state.get(p, {}).items():
                        if torch.is_tensor(v):
                            old = saved_s.get(p, {}).get(k)
                            v.zero_() if old is None else v.copy_(old)  # fresh state is all 0
                for t, q in zip(bufs, saved_b):
                    t.copy_(q)
        return restore

    def _capture(self, body, warm):
        restore = self._snapshot()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warm):
                body()
            restore()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            body()
        return g

    # -- public ----------------------------------------------------------------------------------
    def step(self, ids):
        """One training step over graphs ``ids`` (host ints, ``len(ids) <= batch_size``).
        Returns the static device tensor holding this step's loss; reads nothing back."""
        ids, full, n = self._full_ids(ids)
        if not self._fits(full):
            self.fallbacks += 1
            self._unpadded_step(ids)
            return self.loss
        self._stage_ids(full, n)
        if self._train_graph is None:
            self._train_graph = self._capture(self._padded_step, warm=2)
        self._train_graph.replay()
        return self.loss

    @torch.no_grad()
    def predict(self, ids):
        """Eval-mode predictions for ``ids`` from a second captured graph (forward only): a view
        of the first ``len(ids)`` rows of a static tensor (``[n]``, or ``[n, 2]`` for a
        mean-variance head), overwritten by the next call."""
        ids, full, n = self._full_ids(ids)
        was_training = self.model.training
        if not self._fits(full):
            self.model.eval()
            try:
                return self.model(self.store.collate(ids))
            finally:
                self.model.train(was_training)
        self._stage_ids(full, n)
        if self._predict_graph is None:
            self.model.eval()
            try:
                self._predict_graph = self._capture(self._padded_predict, warm=1)
            finally:
                self.model.train(was_training)
        self._predict_graph.replay()
        return self._pred[:n]

    def epoch_loss(self) -> float:
        """Sum of the step losses since the last call, then zeroed: the epoch's one sync."""
        v = float(self.loss_total.item())
        self.loss_total.zero_()
        return v

    def close(self):
        """Drop the captured graphs (and their memory pools)."""
        self._train_graph = None
        self._predict_graph = None
