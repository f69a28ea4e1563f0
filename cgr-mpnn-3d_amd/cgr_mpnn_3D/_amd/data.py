"""Device-resident reaction-graph store + on-device collation.

The reference loads every reaction as a PyG ``Data`` (``cgr_mpnn_3D/data/ChemDataset.py:81-94``)
and collates each step's batch on the host with ``torch_geometric.loader.DataLoader``
(``cgr_mpnn_3D/training/trainer.py:105-118``), then copies it to the GPU.  At ~1.4 ms per
training step on one MI355X that host path (collating 256 graphs + a 26 MB H2D copy) would cost
more than the step itself.  Here the whole dataset (T1x: ~10k reactions, ~1 GB fp32 with the
768-wide MACE block) is uploaded once, and each batch is collated by one kernel
(``cgr_collate``) into exactly the ``Batch.from_data_list`` layout ``GNN.forward`` reads.

    store = GraphStore.from_data_list(list_of_pyg_data, device)   # or from_batch(collated)
    for ids in sampler:                                             # host int indices
        batch = store.collate(ids)                                  # device TorchBatch
        loss = loss_fn(model(batch), batch.y)

``collate`` needs the output sizes for allocation; they come from the host copy of the per-graph
node/edge counts, so there is no device sync.  There is no CPU fallback.

``collate_padded`` writes the same batch into tensors of fixed capacities and fills the rest with
one pad graph of loss weight 0 (``cgr_collate_padded``; layout in DESIGN.md §4), so one captured
training step replays over every batch of an epoch (``_amd/captured.py``).
"""

from __future__ import annotations

import numpy as np
import torch

from . import native
from .synth import RxnBatch, TorchBatch


class GraphStore:
    def __init__(self, x, edge_index, edge_attr, y, node_ptr, edge_ptr, device):
        """All arrays in collated (PyG ``Batch``) layout on the host (numpy): x [N, F] float32,
        edge_index [2, E] int64 with global node ids, edge_attr [E, Fe] float32, y [G] float32
        or None, node_ptr / edge_ptr [G+1] int64."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("GraphStore lives on the GPU (no CPU fallback)")
        self.node_ptr_h = np.asarray(node_ptr, dtype=np.int64)
        self.edge_ptr_h = np.asarray(edge_ptr, dtype=np.int64)
        self.num_graphs = int(self.node_ptr_h.shape[0] - 1)
        self.F = int(x.shape[1])
        self.Fe = int(edge_attr.shape[1]) if edge_attr is not None else 0
        self.device = dev
        self.x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
        self.edge_index = torch.from_numpy(
            np.ascontiguousarray(edge_index, dtype=np.int64)).to(dev)
        self.edge_attr = (torch.from_numpy(np.ascontiguousarray(edge_attr, dtype=np.float32))
                          .to(dev) if self.Fe else None)
        self.y = (torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(dev)
                  if y is not None else None)
        self.node_ptr = torch.from_numpy(self.node_ptr_h).to(dev)
        self.edge_ptr = torch.from_numpy(self.edge_ptr_h).to(dev)
        self._ncount = np.diff(self.node_ptr_h)
        self._ecount = np.diff(self.edge_ptr_h)
        self._lib = native.load()

    # -- construction ------------------------------------------------------------------------
    @classmethod
    def from_batch(cls, b: RxnBatch, device):
        """From one collated batch holding the whole dataset (edges grouped by graph, as PyG
        collation leaves them)."""
        src_graph = b.batch[b.edge_index[0]]
        if src_graph.size and np.any(np.diff(src_graph) < 0):
            raise ValueError("edges must be grouped by graph (PyG collation order)")
        ecount = np.bincount(src_graph, minlength=b.num_graphs)
        edge_ptr = np.concatenate([[0], np.cumsum(ecount)]).astype(np.int64)
        return cls(b.x, b.edge_index, b.edge_attr, b.y, b.ptr, edge_ptr, device)

    @classmethod
    def from_data_list(cls, data_list, device):
        """From per-reaction PyG-``Data``-like objects (attributes x, edge_index, edge_attr, y;
        torch tensors or numpy arrays), e.g. ``ChemDataset``'s items."""
        def np_(t):
            if t is None:
                return None
            return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

        xs, eis, eas, ys = [], [], [], []
        nptr, eptr = [0], [0]
        for d in data_list:
            x = np_(d.x).astype(np.float32)
            ei = np_(d.edge_index).astype(np.int64)
            ea = np_(getattr(d, "edge_attr", None))
            xs.append(x)
            eis.append(ei + nptr[-1])
            eas.append(ea.astype(np.float32) if ea is not None
                       else np.zeros((ei.shape[1], 0), np.float32))
            y = np_(getattr(d, "y", None))
            ys.append(np.float32(np.asarray(y).reshape(-1)[0]) if y is not None else np.nan)
            nptr.append(nptr[-1] + x.shape[0])
            eptr.append(eptr[-1] + ei.shape[1])
        y = np.asarray(ys, dtype=np.float32)
        return cls(np.concatenate(xs, 0), np.concatenate(eis, 1), np.concatenate(eas, 0),
                   None if np.isnan(y).all() else y, np.asarray(nptr), np.asarray(eptr), device)

    # -- collation ---------------------------------------------------------------------------
    def batch_sizes(self, ids: np.ndarray) -> tuple[int, int]:
        return int(self._ncount[ids].sum()), int(self._ecount[ids].sum())

    def collate(self, ids, stream=None) -> TorchBatch:
        """Batch of graphs ``ids`` (host ints, any order, repeats allowed) in
        ``Batch.from_data_list`` layout, built on the device by one kernel."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        if ids.size and (ids.min() < 0 or ids.max() >= self.num_graphs):
            raise IndexError(f"graph id out of range [0, {self.num_graphs})")
        B = int(ids.size)
        N, E = self.batch_sizes(ids)
        dev = self.device
        gid = torch.from_numpy(ids).to(dev, non_blocking=False)
        x = torch.empty((N, self.F), dtype=torch.float32, device=dev)
        ei = torch.empty((2, E), dtype=torch.int64, device=dev)
        ea = torch.empty((E, self.Fe), dtype=torch.float32, device=dev)
        bt = torch.empty(N, dtype=torch.int64, device=dev)
        ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
        y = torch.empty(B, dtype=torch.float32, device=dev) if self.y is not None else None
        if B:
            with native.device_guard(dev):
                native.check(self._lib.cgr_collate(
                    native.ptr(gid), B, native.ptr(self.node_ptr), native.ptr(self.edge_ptr),
                    native.ptr(self.x), self.F, native.ptr(self.edge_index),
                    int(self.edge_index.shape[1]), native.ptr(self.edge_attr), self.Fe,
                    native.ptr(self.y), native.ptr(x), native.ptr(ei), E, native.ptr(ea),
                    native.ptr(bt), native.ptr(ptr), native.ptr(y),
                    stream if stream is not None else native.stream_ptr(dev)))
        else:
            ptr.zero_()
        out = TorchBatch(x=x, edge_index=ei, edge_attr=ea, batch=bt, ptr=ptr, y=y)
        out._ids = gid  # keep the id buffer alive until the kernel has run
        return out

    # -- fixed-shape collation (captured training over ragged batches) -----------------------
    def padded_caps(self, batch_size: int) -> tuple[int, int]:
        """Capacities that hold any ``batch_size`` graphs of the store: the sum of the
        ``batch_size`` largest node counts + 2 (the pad graph needs two nodes) and the sum of
        the ``batch_size`` largest edge counts.  Tighter capacities may be passed to
        ``collate_padded``; ``fits`` tells whether a batch goes into them."""
        k = int(batch_size)
        if k < 1:
            raise ValueError("padded_caps: batch_size must be at least 1")
        n = np.sort(self._ncount)[::-1][:k].sum()
        e = np.sort(self._ecount)[::-1][:k].sum()
        # repeats are allowed, so more slots than graphs repeat the largest graph
        if k > self.num_graphs:
            n += (k - self.num_graphs) * self._ncount.max()
            e += (k - self.num_graphs) * self._ecount.max()
        e = int(e)
        return int(n) + 2, e + (e & 1)

    @staticmethod
    def pad_degree_bound(pad_nodes: int, pad_pairs: int) -> int:
        """Bound on the in-degree of a pad node: ``pad_pairs`` reverse pairs laid along the ring
        of ``pad_nodes`` nodes give every node at most ``2 * ceil(pad_pairs / pad_nodes)``
        in-edges."""
        return 2 * -(-int(pad_pairs) // int(pad_nodes))

    def fits(self, ids, node_cap: int, edge_cap: int, max_pad_degree: int = 4) -> bool:
        """Whether ``collate_padded(ids, node_cap, edge_cap)`` gives a batch a model may train
        on, from the host copies of the counts (no device sync): the graphs and a pad graph of
        at least two nodes fit, and no pad node gets more than ``max_pad_degree`` in-edges (the
        pad graph's forward values must stay finite: with sum aggregation they grow per layer
        with the in-degree, and 0 * inf in a weight gradient is NaN; 4 is the valence bound of
        the dataset's molecules, so the pad graph grows like a real one)."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        N, E = self.batch_sizes(ids)
        if N + 2 > node_cap or E > edge_cap or (edge_cap - E) & 1:
            return False
        return self.pad_degree_bound(node_cap - N, (edge_cap - E) // 2) <= max_pad_degree

    def alloc_padded(self, batch_size: int, node_cap: int, edge_cap: int) -> TorchBatch:
        """Static output tensors of ``collate_padded`` (``out=``) for ``batch_size`` slots."""
        B, N, E = int(batch_size), int(node_cap), int(edge_cap)
        if B < 1 or N < 2 or E < 0 or E & 1:
            raise ValueError("collate_padded: batch_size >= 1, node_cap >= 2, edge_cap even")
        dev = self.device
        out = TorchBatch(
            x=torch.empty((N, self.F), dtype=torch.float32, device=dev),
            edge_index=torch.empty((2, E), dtype=torch.int64, device=dev),
            edge_attr=torch.empty((E, self.Fe), dtype=torch.float32, device=dev),
            batch=torch.empty(N, dtype=torch.int64, device=dev),
            ptr=torch.empty(B + 2, dtype=torch.int64, device=dev),
            y=torch.empty(B + 1, dtype=torch.float32, device=dev) if self.y is not None else None)
        out.mask = torch.empty(B + 1, dtype=torch.float32, device=dev)
        out.info = torch.empty(4, dtype=torch.int64, device=dev)
        return out

    def collate_padded(self, ids, node_cap, edge_cap, *, out=None, ids_dev=None,
                       weight_dev=None, stream=None) -> TorchBatch:
        """The batch of ``collate(ids)`` in tensors of fixed shapes ``[node_cap, F]`` /
        ``[2, edge_cap]``, the remainder filled by one pad graph (slot B, loss weight 0; see
        ``cgr_collate_padded`` in include/cgr_mpnn3d.h).  ``ptr`` has B + 2 entries, so
        ``GNN.forward`` sees B + 1 graphs; ``.mask`` [B + 1] holds the slots' loss weights (1 for
        a real slot, 0 for a filler slot and the pad graph), ``.info`` [4] (int64, device) =
        N_real, E_real, status, 0.

        ``out``: tensors from ``alloc_padded`` (or an earlier call) to write into.  ``ids_dev``
        (int64 [B]) / ``weight_dev`` (float32 [B]): the ids and slot weights already on the
        device -- the call then touches no host data and can be captured with frozen arguments
        (``ids`` may be None; the caller checks ``fits`` itself).  Given host ``ids`` only, every
        slot gets weight 1."""
        dev = self.device
        if ids_dev is None:
            ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
            if ids.size and (ids.min() < 0 or ids.max() >= self.num_graphs):
                raise IndexError(f"graph id out of range [0, {self.num_graphs})")
            ids_dev = torch.from_numpy(ids).to(dev)
        elif ids_dev.dtype != torch.int64 or ids_dev.device != dev or \
                not ids_dev.is_contiguous() or ids_dev.dim() != 1:
            raise ValueError("collate_padded: ids_dev must be a contiguous int64 vector on the "
                             "store's device")
        B = int(ids_dev.numel())
        if B < 1:
            raise ValueError("collate_padded: at least one graph id")
        if weight_dev is None:
            weight_dev = torch.ones(B, dtype=torch.float32, device=dev)
        elif weight_dev.dtype != torch.float32 or weight_dev.device != dev or \
                not weight_dev.is_contiguous() or weight_dev.numel() != B:
            raise ValueError("collate_padded: weight_dev must be a contiguous float32 [B] "
                             "vector on the store's device")
        N, E = int(node_cap), int(edge_cap)
        if out is None:
            out = self.alloc_padded(B, N, E)
        elif tuple(out.x.shape) != (N, self.F) or tuple(out.edge_index.shape) != (2, E) or \
                out.ptr.numel() != B + 2 or out.mask.numel() != B + 1 or \
                out.edge_attr.shape[0] != E or out.batch.numel() != N:
            raise ValueError("collate_padded: `out` was allocated for other sizes")
        with native.device_guard(dev):
            native.check(self._lib.cgr_collate_padded(
                native.ptr(ids_dev), native.ptr(weight_dev), B, self.num_graphs,
                native.ptr(self.node_ptr), native.ptr(self.edge_ptr), native.ptr(self.x), self.F,
                native.ptr(self.edge_index), int(self.edge_index.shape[1]),
                native.ptr(self.edge_attr), self.Fe, native.ptr(self.y), N, E,
                native.ptr(out.x), native.ptr(out.edge_index), native.ptr(out.edge_attr),
                native.ptr(out.batch), native.ptr(out.ptr), native.ptr(out.y),
                native.ptr(out.mask), native.ptr(out.info),
                stream if stream is not None else native.stream_ptr(dev)))
        out._ids = (ids_dev, weight_dev)  # alive until the kernel has run
        return out
