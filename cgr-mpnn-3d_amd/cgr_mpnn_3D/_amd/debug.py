"""Introspection helpers (tests / profiling): run the native forward with a caller-visible arena
and view its saved buffers; every buffer a call writes can also be the caller's own (the arena
contract's tests hand in guarded ones).  Not used by the model itself."""

from __future__ import annotations

import ctypes

import torch

from . import native
from .functional import (_LEVEL_CALLS, LEVEL_FUSED, LEVEL_NODES, LEVEL_POOLED, _batch_struct,
                         _dropout_array, _param_table, make_config)


def _caller_bytes(buf, nbytes, dev):
    """The first `nbytes` bytes of the caller's uint8 buffer `buf` (None: a fresh torch.empty)."""
    if buf is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert buf.dtype == torch.uint8 and buf.dim() == 1 and buf.is_contiguous(), "uint8 [n] buffer"
    assert buf.numel() >= nbytes and buf.device == dev, (buf.numel(), nbytes, buf.device)
    return buf[:nbytes]


class ArenaRun:
    def __init__(self, cfg_tuple, x, edge_index, edge_attr, batch, graph_ptr, num_graphs, params,
                 dropout_ps=None, seed=0, training=False, prepare_backward=True,
                 rng_counter=None, encode=False, g_out=None, nodes=False, n_out=None, arena=None,
                 y=None):
        """rng_counter: optional device int64 tensor [1], the dropout counter the forward reads
        and advances when any layer drops (GNN._cgr_rng_counter's role); None: the key is seed.
        encode: the headless forward (cgr_gnn_encode; the ffn slots of `params` may be None):
        self.g_out [B, H] instead of self.y -- written into `g_out` when the caller passes a
        buffer (any float32 tensor whose storage holds B * H floats from its data pointer) -- and
        backward / input_grads then take dg [B, H].
        nodes: the nodes-level forward (cgr_gnn_encode_nodes; ffn slots may be None, the config's
        pooling takes no part): self.n_out [N, H] -- written into `n_out` when the caller passes a
        buffer holding N * H floats from its data pointer -- and backward / input_grads take
        dn [N, H].
        arena: a caller-owned uint8 device tensor of at least cgr_gnn_arena_bytes, used from its
        data pointer, whatever it holds (None: a fresh torch.empty).  y: likewise the fused
        level's output, a float32 tensor holding B floats from its data pointer."""
        assert not (encode and nodes), "one output level per run"
        lib = native.load()
        self.cfg = make_config(*cfg_tuple)
        self.N, self.E, self.B = int(x.shape[0]), int(edge_index.shape[1]), int(num_graphs)
        self.H = self.cfg.hidden
        self.Hp = (self.H + 3) // 4 * 4
        dev = x.device
        nbytes = lib.cgr_gnn_arena_bytes(ctypes.byref(self.cfg), self.N, self.E, self.B)
        self.arena = _caller_bytes(arena, nbytes, dev)
        self.encode = bool(encode)
        self.nodes = bool(nodes)
        self.level = LEVEL_NODES if nodes else LEVEL_POOLED if encode else LEVEL_FUSED
        self.y = None
        if self.nodes:
            self.n_out = out = n_out if n_out is not None else torch.empty(
                self.N, self.H, dtype=torch.float32, device=dev)
        elif self.encode:
            self.g_out = out = g_out if g_out is not None else torch.empty(
                self.B, self.H, dtype=torch.float32, device=dev)
        else:
            self.y = out = y if y is not None else torch.empty(
                self.B, dtype=torch.float32, device=dev)
        self._keep = (x, edge_index, edge_attr, batch, graph_ptr, params, rng_counter)
        self.bs = _batch_struct(x, edge_index, edge_attr, batch, graph_ptr, self.B)
        self.dropout_ps, self.seed, self.training = dropout_ps, seed, training
        # prepared for the backward (this helper runs it), as a training step's forward is
        self.flags = (native.TRAIN_DROPOUT if training else 0) | (
            native.TRAIN_FOR_BACKWARD if prepare_backward else 0)
        with native.device_guard(dev):
            entry = getattr(lib, _LEVEL_CALLS[self.level][0])
            native.check(entry(
                ctypes.byref(self.cfg), _param_table(params), ctypes.byref(self.bs),
                _dropout_array(dropout_ps, self.cfg.depth), ctypes.c_uint64(seed),
                native.ptr(rng_counter), self.flags, native.ptr(self.arena),
                native.ptr(out), native.stream_ptr(dev)))

    def offset(self, name, index=0):
        lib = native.load()
        return lib.cgr_gnn_arena_offset(ctypes.byref(self.cfg), self.N, self.E, self.B,
                                        name.encode(), index)

    def ints(self, name, count):
        off = self.offset(name)
        assert off >= 0, name
        return self.arena[off:off + 4 * count].view(torch.int32)

    def uint64(self, name, count=1):
        """count 64-bit words of a named buffer ("rng": the dropout key this forward used)."""
        off = self.offset(name)
        assert off >= 0 and off % 8 == 0, name
        return self.arena[off:off + 8 * count].view(torch.int64)

    def rng_key(self):
        """The dropout key in the arena as a Python int in [0, 2^64) (synchronizes)."""
        return int(self.uint64("rng").item()) % 2**64

    def floats(self, name, rows, index=0, cols=None):
        off = self.offset(name, index)
        assert off >= 0, (name, index)
        cols = self.Hp if cols is None else cols
        t = self.arena[off:off + 4 * rows * cols].view(torch.float32).view(rows, cols)
        return t[:, :self.H] if cols == self.Hp else t

    def ws_floats(self, name, rows, index=0):
        """[rows, H] view of a backward-workspace buffer ("dpre" with the layer index, "dpre0",
        "ds": cgr_gnn_workspace_offset) of the last backward(); ws_floats_padded keeps the Hp - H
        pad columns."""
        return self.ws_floats_padded(name, rows, index)[:, :self.H]

    def ws_floats_padded(self, name, rows, index=0):
        lib = native.load()
        off = lib.cgr_gnn_workspace_offset(ctypes.byref(self.cfg), self.N, self.E, self.B,
                                           name.encode(), index)
        assert off >= 0, (name, index)
        return self.ws[off:off + 4 * rows * self.Hp].view(torch.float32).view(rows, self.Hp)

    def backward(self, dy, params, ws=None, grads=None):
        """dy [B] (encode: dg [B, H]; nodes: dn [N, H]) -> the gradient list (encode, nodes: None
        in the ffn slots).  ws: a caller-owned uint8 device tensor of at least
        cgr_gnn_workspace_bytes; grads: the caller's gradient tensors in the parameter table's
        order (None where the parameter is None), e.g. views into one flat buffer; None: fresh
        torch.empty ones."""
        lib = native.load()
        dev = dy.device
        ws = _caller_bytes(ws, lib.cgr_gnn_workspace_bytes(ctypes.byref(self.cfg), self.N, self.E,
                                                           self.B), dev)
        if grads is None:
            grads = [None if p is None else torch.empty_like(p) for p in params]
        assert len(grads) == len(params)
        self.ws = ws
        entry = getattr(lib, _LEVEL_CALLS[self.level][1])
        with native.device_guard(dev):
            native.check(entry(
                ctypes.byref(self.cfg), _param_table(params), ctypes.byref(self.bs),
                _dropout_array(self.dropout_ps, self.cfg.depth), ctypes.c_uint64(self.seed),
                self.flags, native.ptr(self.arena), native.ptr(dy.contiguous()),
                _param_table(grads), native.ptr(ws), None, native.stream_ptr(dev)))
        return grads

    def input_grads(self, dy, params, ws, dx=None, de=None):
        """cgr_gnn_input_grads (encode: cgr_gnn_encode_input_grads, dy = dg; nodes:
        cgr_gnn_encode_nodes_input_grads, dy = dn) on this arena with workspace `ws` ->
        (dx, dedge_attr), written into the caller's `dx` [N, F] / `de` [E, Fe] where given."""
        lib = native.load()
        dev = dy.device
        F_ = self.cfg.num_node_features
        Fe = self.cfg.num_edge_features
        if dx is None:
            dx = torch.empty(self.N, F_, device=dev)
        if not Fe:
            de = None
        elif de is None:
            de = torch.empty(self.E, Fe, device=dev)
        entry = getattr(lib, _LEVEL_CALLS[self.level][2])
        with native.device_guard(dev):
            native.check(entry(
                ctypes.byref(self.cfg), _param_table(params), ctypes.byref(self.bs),
                native.ptr(self.arena), native.ptr(dy.contiguous()), native.ptr(ws),
                native.ptr(dx), native.ptr(de), native.stream_ptr(dev)))
        return dx, de


class PredictRun:
    """The level's forward-only entry (cgr_gnn_predict / _encode_predict / _encode_nodes_predict)
    on a caller-visible predict arena: self.y [B], [B, H] or [N, H] by `level`.
    arena: a caller-owned uint8 device tensor of at least cgr_gnn_predict_arena_bytes (None: a
    fresh torch.empty); images: a uint8 device tensor that cgr_gnn_pack_images filled
    (pack_images), None: the call packs its own into the arena; y: the caller's output buffer."""

    def __init__(self, cfg_tuple, x, edge_index, edge_attr, batch, graph_ptr, num_graphs, params,
                 level=LEVEL_FUSED, arena=None, images=None, y=None, dropout_ps=None, seed=0,
                 training=False, rng_counter=None):
        lib = native.load()
        self.cfg = make_config(*cfg_tuple)
        self.N, self.E, self.B = int(x.shape[0]), int(edge_index.shape[1]), int(num_graphs)
        self.H, self.level = self.cfg.hidden, level
        dev = x.device
        self.arena = _caller_bytes(arena, lib.cgr_gnn_predict_arena_bytes(
            ctypes.byref(self.cfg), self.N, self.E, self.B), dev)
        shape = (self.B, (self.B, self.H), (self.N, self.H))[level]
        self.y = y if y is not None else torch.empty(shape, dtype=torch.float32, device=dev)
        self.images = images
        self._keep = (x, edge_index, edge_attr, batch, graph_ptr, params, rng_counter)
        self.bs = _batch_struct(x, edge_index, edge_attr, batch, graph_ptr, self.B)
        entry = getattr(lib, _LEVEL_CALLS[level][3])
        with native.device_guard(dev):
            native.check(entry(
                ctypes.byref(self.cfg), _param_table(params), ctypes.byref(self.bs),
                _dropout_array(dropout_ps, self.cfg.depth), ctypes.c_uint64(seed),
                native.ptr(rng_counter), native.TRAIN_DROPOUT if training else 0,
                native.ptr(images), native.ptr(self.arena), native.ptr(self.y),
                native.stream_ptr(dev)))

    def status(self):
        """The graph prep's status word (the training arena's offset: the shared prefix)."""
        off = native.load().cgr_gnn_arena_offset(ctypes.byref(self.cfg), self.N, self.E, self.B,
                                                 b"status", 0)
        return int(self.arena[off:off + 4].view(torch.int32).item())


def pack_images(cfg_tuple, params, dev, images=None):
    """cgr_gnn_pack_images of `params` into `images` (a caller-owned uint8 device tensor of at
    least cgr_gnn_image_bytes; None: a fresh torch.empty) -> its first cgr_gnn_image_bytes."""
    lib = native.load()
    cfg = make_config(*cfg_tuple)
    images = _caller_bytes(images, lib.cgr_gnn_image_bytes(ctypes.byref(cfg)), dev)
    with native.device_guard(dev):
        native.check(lib.cgr_gnn_pack_images(ctypes.byref(cfg), _param_table(params),
                                             native.ptr(images), native.stream_ptr(dev)))
    return images
