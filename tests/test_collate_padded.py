"""Fixed-shape collation (cgr_collate_padded / GraphStore.collate_padded): the batch of
cgr_collate followed by one pad graph, bit-exact against a reference built here from the PyG
collation restatement (oracle/collate_numpy.py) plus the pad layout of include/cgr_mpnn3d.h:

  pad nodes N_real + i (i < P = N_cap - N_real): x = 0, batch = B; ptr[B] = N_real,
  ptr[B+1] = N_cap, y[B] = 0, mask[:B] = slot weights, mask[B] = 0;
  pad pair j < Ep = (E_cap - E_real) / 2: edge E_real+2j = (a -> b), edge E_real+2j+1 = (b -> a),
  a = N_real + j mod P, b = N_real + (j+1) mod P, edge_attr = 0.
"""

import numpy as np
import pytest

from cgr_mpnn_3D._amd.synth import make_batch
from oracle import collate_numpy as oc


def _store_arrays(b):
    src_graph = b.batch[b.edge_index[0]]
    ecount = np.bincount(src_graph, minlength=b.num_graphs)
    edge_ptr = np.concatenate([[0], np.cumsum(ecount)]).astype(np.int64)
    return b.x, b.edge_index, b.edge_attr, b.y, b.ptr, edge_ptr


def pad_edges(N_real, E_real, N_cap, E_cap):
    """[2, E_cap - E_real] pad edge block of the layout above."""
    P, Ep = N_cap - N_real, (E_cap - E_real) // 2
    j = np.arange(Ep, dtype=np.int64)
    a, b = N_real + j % P, N_real + (j + 1) % P
    ei = np.empty((2, 2 * Ep), np.int64)
    ei[0, 0::2], ei[1, 0::2] = a, b
    ei[0, 1::2], ei[1, 1::2] = b, a
    return ei


def padded_reference(ids, weights, arrays, N_cap, E_cap):
    ref = oc.collate(ids, *arrays)
    B = len(ids)
    N_real, E_real = ref["x"].shape[0], ref["edge_index"].shape[1]
    assert N_real + 2 <= N_cap and E_real <= E_cap and (E_cap - E_real) % 2 == 0
    F, Fe = ref["x"].shape[1], ref["edge_attr"].shape[1]
    x = np.zeros((N_cap, F), np.float32)
    x[:N_real] = ref["x"]
    ea = np.zeros((E_cap, Fe), np.float32)
    ea[:E_real] = ref["edge_attr"]
    ei = np.concatenate([ref["edge_index"], pad_edges(N_real, E_real, N_cap, E_cap)], 1)
    batch = np.full(N_cap, B, np.int64)
    batch[:N_real] = ref["batch"]
    return dict(x=x, edge_index=ei, edge_attr=ea, batch=batch,
                ptr=np.concatenate([ref["ptr"], [N_cap]]).astype(np.int64),
                y=np.concatenate([ref["y"], [0]]).astype(np.float32),
                mask=np.concatenate([weights, [0]]).astype(np.float32),
                info=np.array([N_real, E_real, 0, 0], np.int64))


def max_pad_in_degree(N_real, E_real, N_cap, E_cap):
    ei = pad_edges(N_real, E_real, N_cap, E_cap)
    return int(np.bincount(ei[1] - N_real, minlength=1).max()) if ei.size else 0


@pytest.mark.parametrize("P,Ep", [(2, 0), (2, 1), (2, 100), (7, 5), (3, 1), (7, 7), (7, 8),
                                  (7, 9), (5, 23), (64, 130)])
def test_reference_pad_layout_is_paired_in_range_and_degree_bounded(P, Ep):
    from cgr_mpnn_3D._amd.data import GraphStore

    N_real, E_real = 37, 90
    N_cap, E_cap = N_real + P, E_real + 2 * Ep
    ei = pad_edges(N_real, E_real, N_cap, E_cap)
    assert ei.shape == (2, 2 * Ep)
    # reverse pairs: edge 2k+1 is the reverse of edge 2k, no self loop
    assert np.array_equal(ei[0, 0::2], ei[1, 1::2]) and np.array_equal(ei[1, 0::2], ei[0, 1::2])
    assert np.all(ei[0] != ei[1])
    if Ep:
        assert ei.min() >= N_real and ei.max() < N_cap
    # the bound fits() tests, 2 ceil(Ep / P): the ring gives node 0 ceil(Ep/P) out-pairs and node 1
    # ceil(Ep/P) in-pairs; it is attained unless Ep mod P == 1 (the extra pair then adds one
    # in-edge to each of two nodes: one below the bound)
    bound = GraphStore.pad_degree_bound(P, Ep)
    assert bound == 2 * ((Ep + P - 1) // P)
    deg = max_pad_in_degree(N_real, E_real, N_cap, E_cap)
    assert deg == (bound - 1 if Ep % P == 1 else bound)


def _garbage(out):
    """Pre-fill the static outputs, so every element the kernel must write is seen to be."""
    for t in (out.x, out.edge_attr, out.y, out.mask):
        t.fill_(float("nan"))
    for t in (out.edge_index, out.batch, out.ptr, out.info):
        t.fill_(-7)


def _assert_equal(got, ref):
    for k in ("x", "edge_index", "edge_attr", "batch", "ptr", "y", "mask", "info"):
        g = getattr(got, k).cpu().numpy()
        assert g.shape == ref[k].shape, k
        assert np.array_equal(g.view(np.int32) if g.dtype == np.float32 else g,
                              ref[k].view(np.int32) if g.dtype == np.float32 else ref[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("n_mace,fe", [(3, 14), (2, 14), (3, 0), (2, 0)])
def test_device_collate_padded_bit_exact(n_mace, fe, cuda_device):
    import torch

    from cgr_mpnn_3D._amd.data import GraphStore

    b = make_batch(40, n_atoms=9, n_bonds=11, n_mace=n_mace, seed=7, n_atoms_jitter=4)
    if fe == 0:
        b.edge_attr = np.zeros((b.edge_attr.shape[0], 0), np.float32)
    arrays = _store_arrays(b)
    store = GraphStore.from_batch(b, cuda_device)
    rng = np.random.default_rng(0)

    def check(ids, N_cap, E_cap, weights=None):
        ids = np.asarray(ids, np.int64)
        w = np.ones(len(ids), np.float32) if weights is None else weights
        ref = padded_reference(ids, w, arrays, N_cap, E_cap)
        out = store.alloc_padded(len(ids), N_cap, E_cap)
        _garbage(out)
        if weights is None:
            got = store.collate_padded(ids, N_cap, E_cap, out=out)
        else:  # everything already on the device, as a captured step passes it
            got = store.collate_padded(
                None, N_cap, E_cap, out=out, ids_dev=torch.from_numpy(ids).to(cuda_device),
                weight_dev=torch.from_numpy(w).to(cuda_device))
        assert got is out
        _assert_equal(got, ref)
        # the real region is what cgr_collate writes
        plain = store.collate(ids)
        N, E = store.batch_sizes(ids)
        assert torch.equal(got.x[:N], plain.x) and torch.equal(got.batch[:N], plain.batch)
        assert torch.equal(got.edge_index[:, :E], plain.edge_index)
        assert torch.equal(got.edge_attr[:E], plain.edge_attr)
        assert torch.equal(got.ptr[:len(ids) + 1], plain.ptr)
        assert torch.equal(got.y[:len(ids)], plain.y)

    ids = rng.integers(0, 40, size=25)
    N, E = store.batch_sizes(ids)
    check(ids, N + 7, E + 10)                      # random ids
    check(ids, N + 2, E + 4)                       # P == 2 exactly
    check(ids, N + 5, E)                           # Ep == 0
    check(ids, N + 3, E + 2)                       # one pad pair
    check(ids, *store.padded_caps(25))             # the always-sufficient capacities
    short = rng.integers(0, 40, size=10)           # a short batch: filler slots at weight 0
    full = np.resize(short, 16)
    w = np.concatenate([np.ones(10), np.zeros(6)]).astype(np.float32)
    N, E = store.batch_sizes(full)
    check(full, N + 9, E + 12, weights=w)
    rep = np.array([3, 3, 3])                      # repeated ids
    N, E = store.batch_sizes(rep)
    check(rep, N + 4, E + 6)
    one = np.array([39])
    check(one, *store.padded_caps(1))
    # without `out` the tensors are allocated at the capacities
    got = store.collate_padded(ids, 400, 900)
    assert got.x.shape == (400, store.F) and got.edge_index.shape == (2, 900)
    assert got.ptr.numel() == 27 and got.num_graphs == 26
    _assert_equal(got, padded_reference(ids, np.ones(25, np.float32), arrays, 400, 900))


@pytest.mark.gpu
def test_padded_caps_and_fits(cuda_device):
    from cgr_mpnn_3D._amd.data import GraphStore

    b = make_batch(40, n_atoms=9, n_bonds=11, n_mace=2, seed=7, n_atoms_jitter=4)
    store = GraphStore.from_batch(b, cuda_device)
    nc, ec = np.diff(b.ptr), np.diff(_store_arrays(b)[5])
    for k in (1, 8, 40):
        assert store.padded_caps(k) == (int(np.sort(nc)[-k:].sum()) + 2,
                                        int(np.sort(ec)[-k:].sum()))
    ids = np.arange(8)
    N, E = store.batch_sizes(ids)
    assert store.fits(ids, N + 2, E) and store.fits(ids, N + 2, E + 8)
    assert not store.fits(ids, N + 1, E + 8)       # no room for a two-node pad graph
    assert not store.fits(ids, N + 2, E - 2)
    assert not store.fits(ids, N + 2, E + 10)      # 5 pairs on 2 nodes: in-degree 6 > 4
    assert store.fits(ids, N + 2, E + 10, max_pad_degree=6)
    assert store.fits(ids, N + 5, E + 20) and not store.fits(ids, N + 5, E + 22)
    assert not store.fits(ids, N + 5, E + 3)       # an odd remainder cannot be reverse pairs


@pytest.mark.gpu
@pytest.mark.parametrize("short_nodes,short_edges", [(True, False), (False, True), (True, True)])
def test_overflow_sets_status_and_writes_nothing_outside_the_capacities(short_nodes, short_edges,
                                                                        cuda_device):
    """Capacities too small for the ids: info[2] bit 0, and the kernel itself keeps every write
    inside the capacities -- the outputs are allocated larger and the excess holds a canary."""
    import torch

    from cgr_mpnn_3D._amd import native
    from cgr_mpnn_3D._amd.data import GraphStore

    b = make_batch(40, n_atoms=9, n_bonds=11, n_mace=3, seed=7, n_atoms_jitter=4)
    store = GraphStore.from_batch(b, cuda_device)
    ids = np.arange(40)[::-1].copy()
    B = len(ids)
    N, E = store.batch_sizes(ids)
    N_cap = N // 2 + 1 if short_nodes else N + 6
    E_cap = (E // 4) * 2 if short_edges else E + 8
    assert not store.fits(ids, N_cap, E_cap)
    EXTRA, F, Fe = 300, store.F, store.Fe
    dev = cuda_device
    f32 = dict(dtype=torch.float32, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    CF, CI = -12345.0, -987654321
    sizes = dict(x=N_cap * F, ea=E_cap * Fe, y=B + 1, mask=B + 1, ei=2 * E_cap, batch=N_cap,
                 ptr=B + 2, info=4)
    bufs = {k: torch.full((n + EXTRA,), CF if k in ("x", "ea", "y", "mask") else CI,
                          **(f32 if k in ("x", "ea", "y", "mask") else i64))
            for k, n in sizes.items()}
    gid = torch.from_numpy(ids).to(dev)
    w = torch.ones(B, **f32)
    p = native.ptr
    native.check(native.load().cgr_collate_padded(
        p(gid), p(w), B, store.num_graphs, p(store.node_ptr), p(store.edge_ptr), p(store.x), F,
        p(store.edge_index), int(store.edge_index.shape[1]), p(store.edge_attr), Fe, p(store.y),
        N_cap, E_cap, p(bufs["x"]), p(bufs["ei"]), p(bufs["ea"]), p(bufs["batch"]),
        p(bufs["ptr"]), p(bufs["y"]), p(bufs["mask"]), p(bufs["info"]),
        native.stream_ptr(dev)))
    torch.cuda.synchronize()
    info = bufs["info"][:4].cpu().numpy()
    assert info[0] == N and info[1] == E and info[2] & native.PAD_OVERFLOW and info[3] == 0
    for k, n in sizes.items():
        tail = bufs[k][n:]
        assert bool((tail == (CF if tail.dtype == torch.float32 else CI)).all()), k
    # what was written inside stays a valid index space for anything that reads it
    ei = bufs["ei"][:2 * E_cap]
    written = ei[ei != CI]
    assert written.numel() == 0 or (int(written.min()) >= 0 and int(written.max()) < N_cap)
    ptr = bufs["ptr"][:B + 2].cpu().numpy()
    assert ptr.min() >= 0 and ptr.max() <= N_cap


@pytest.mark.gpu
def test_collate_padded_rejects_bad_arguments(cuda_device):
    import torch

    from cgr_mpnn_3D._amd.data import GraphStore

    b = make_batch(6, n_atoms=8, n_bonds=9, n_mace=2, seed=9)
    store = GraphStore.from_batch(b, cuda_device)
    with pytest.raises(IndexError):
        store.collate_padded([0, 6], 100, 200)
    with pytest.raises(ValueError):
        store.collate_padded([0, 1], 100, 201)     # odd edge capacity
    with pytest.raises(ValueError):
        store.collate_padded(None, 100, 200, ids_dev=torch.zeros(2, dtype=torch.int32,
                                                                 device=cuda_device))
    out = store.alloc_padded(3, 100, 200)
    with pytest.raises(ValueError):
        store.collate_padded([0, 1], 100, 200, out=out)  # `out` holds 3 slots
    # an id out of range that reaches the kernel (device ids are not checked on the host) is
    # taken as an empty graph and flagged, not dereferenced
    bad = torch.tensor([1, 77, 2], dtype=torch.int64, device=cuda_device)
    got = store.collate_padded(None, 100, 200, out=out, ids_dev=bad)
    info = got.info.cpu().numpy()
    N, E = store.batch_sizes(np.array([1, 2]))
    assert info[0] == N and info[1] == E and info[2] == 4
