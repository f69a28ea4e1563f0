"""Shared by tests/test_gpu_arena_contract.py (the kernels), the fp64 stage tests (their poisoned
first run) and tests/test_arena_contract_model.py (what these checks can tell apart, on the CPU).

The contract of every caller-owned buffer of the C ABI (include/cgr_mpnn3d.h): its contents on
entry are arbitrary, and nothing outside the bytes the library reports is written.  Both halves
are checked with bytes alone:

  Guarded       [guard | payload | guard]: the payload starts from a chosen fill, the guards
                from 0xA5; check_guards() finds any write outside the payload.
  fills         "zero" 0x00; "ones" 0xFF (fp32 NaN, bf16 NaN, int32 -1); stale: the bytes a
                finished run of a different case left in its buffer of the same kind.  No fill
                reads as a large positive int32: a stale word misread as an index must stay
                next to its buffer, where the guard absorbs it.
  slack_ranges  the bytes between a named region's logical end and the next 256-byte boundary
                (the layouts round every region up): nobody's, so they keep the fill.
  check_fills   one run per fill: guards, slack, and every output bit-identical across fills.

Everything here works on CPU tensors too; only the runner that fills the buffers needs a GPU.
"""

import ctypes

import numpy as np
import torch

GUARD_BYTES = 64 * 1024  # a multiple of 4096; -1 x any row stride used here stays inside
GUARD_BYTE = 0xA5
ALIGN = 256  # the payload's alignment, and the layouts' region rounding (Bump::take)
FILL_BYTE = {"zero": 0x00, "ones": 0xFF}
FILLS = ("zero", "ones", "stale")


def _as_bytes(a):
    """uint8 numpy view of a tensor's / array's bytes (host copy)."""
    if isinstance(a, torch.Tensor):
        a = a.detach().contiguous().cpu().numpy()
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Guarded:
    """`nbytes` of payload, 256-byte aligned, between two guards of at least GUARD_BYTES of 0xA5
    (the rear guard starts at the payload's last byte + 1).  fill: "zero", "ones", or the stale
    bytes themselves (a tensor or array: tiled or truncated to nbytes)."""

    def __init__(self, nbytes, fill, dev):
        self.nbytes = int(nbytes)
        total = GUARD_BYTES + self.nbytes + GUARD_BYTES + ALIGN
        self.buf = torch.full((total,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        self.lead = GUARD_BYTES + (-(self.buf.data_ptr() + GUARD_BYTES)) % ALIGN
        self.payload = self.buf[self.lead:self.lead + self.nbytes]
        assert self.nbytes == 0 or self.payload.data_ptr() % ALIGN == 0
        if isinstance(fill, str):
            self.fill_name = fill
            self.fill = np.full(self.nbytes, FILL_BYTE[fill], np.uint8)
        else:
            self.fill_name = "stale"
            src = _as_bytes(fill)
            assert src.size > 0, "no stale bytes"
            self.fill = np.resize(src, self.nbytes)  # tiled or truncated
        self.payload.copy_(torch.from_numpy(self.fill).to(dev))

    def floats(self, *shape):
        n = int(np.prod(shape))
        assert 4 * n <= self.nbytes
        return self.payload[:4 * n].view(torch.float32).view(*shape)

    def bytes(self):
        """The payload as it stands, uint8 numpy."""
        return _as_bytes(self.payload)

    def check_guards(self, what="buffer"):
        """Every guard byte still 0xA5; else the first and last changed offset, relative to the
        payload's first byte (negative: in front of it; >= nbytes: past its end)."""
        whole = _as_bytes(self.buf)
        guard = np.ones(whole.size, bool)
        guard[self.lead:self.lead + self.nbytes] = False
        bad = np.flatnonzero(guard & (whole != GUARD_BYTE))
        assert bad.size == 0, (
            f"{what}: {bad.size} guard bytes changed, offsets {int(bad[0]) - self.lead} .. "
            f"{int(bad[-1]) - self.lead} relative to a payload of {self.nbytes} bytes "
            f"({self.fill_name} fill)")

    def check_slack(self, ranges, what="buffer"):
        """ranges: (name, lo, hi) byte ranges of the payload that must still hold the fill."""
        now = self.bytes()
        for name, lo, hi in ranges:
            assert 0 <= lo <= hi <= self.nbytes, (what, name, lo, hi, self.nbytes)
            bad = np.flatnonzero(now[lo:hi] != self.fill[lo:hi])
            assert bad.size == 0, (
                f"{what}: slack after {name} written: {bad.size} bytes, offsets "
                f"{lo + int(bad[0])} .. {lo + int(bad[-1])} of [{lo}, {hi}) "
                f"({self.fill_name} fill)")


# -------------------------------------------------------------------------------------------------
# the named regions of the two layouts, through the host-only offset queries
# -------------------------------------------------------------------------------------------------
ARENA_INTS = ("perm", "src_s", "dst_s", "rev_s", "src_list")  # 4 E bytes each
MAX_DEPTH = 32


def _round_up(n, m):
    return (n + m - 1) // m * m


def named_regions(cfg, N, E, B):
    """{"arena": [(name, offset, logical bytes)], "ws": [...]} of every buffer the offset queries
    know and that exists for this configuration (status, the one unaligned word, left out)."""
    from cgr_mpnn_3D._amd import native

    lib = native.load()
    H, D, Fe = cfg.hidden, cfg.depth, cfg.num_edge_features
    Hp, Fep = _round_up(H, 4), _round_up(Fe, 4)

    def a_off(name, index=0):
        return lib.cgr_gnn_arena_offset(ctypes.byref(cfg), N, E, B, name.encode(), index)

    def w_off(name, index=0):
        return lib.cgr_gnn_workspace_offset(ctypes.byref(cfg), N, E, B, name.encode(), index)

    arena = [("rng", a_off("rng"), 8)]
    arena += [(k, a_off(k), 4 * E) for k in ARENA_INTS]
    arena += [("dst_ptr", a_off("dst_ptr"), 4 * (N + 1)),
              ("src_ptr", a_off("src_ptr"), 4 * (N + 1)), ("graph_ptr", a_off("graph_ptr"), 4 * (B + 1)),
              ("node_graph", a_off("node_graph"), 4 * N), ("e_s", a_off("e_s"), 4 * E * Fep),
              ("P", a_off("P"), 4 * N * Hp), ("Q", a_off("Q"), 4 * N * Hp)]
    for l in range(MAX_DEPTH + 1):
        arena += [(f"h[{l}]", a_off("h", l), 4 * E * Hp), (f"a[{l}]", a_off("a", l), 4 * N * Hp),
                  (f"pre[{l}]", a_off("pre", l), 4 * E * Hp)]
    arena += [("zn", a_off("zn"), 4 * N * Hp), ("hn", a_off("hn"), 4 * N * Hp),
              ("g", a_off("g"), 4 * B * Hp)]
    # dpre: the D layers' buffers back to back, one region
    ws = [("dpre", w_off("dpre", 0), 4 * E * Hp * D), ("dpre0", w_off("dpre0"), 4 * E * Hp),
          ("ds", w_off("ds"), 4 * N * Hp), ("dzn_main", w_off("dzn_main"), 4 * N * Hp)]
    return {"arena": [r for r in arena if r[1] >= 0], "ws": [r for r in ws if r[1] >= 0]}


def slack_ranges(run):
    """{"arena": [(name, lo, hi)], "ws": [...]}: for every named region of `run`'s configuration
    (anything with .cfg, .N, .E, .B) the bytes from its logical end to the next 256-byte boundary
    -- where the next region starts, or the buffer ends.  Empty ranges are left out."""
    out = {}
    for kind, regs in named_regions(run.cfg, run.N, run.E, run.B).items():
        out[kind] = [(name, off + size, _round_up(off + size, ALIGN)) for name, off, size in regs
                     if (off + size) % ALIGN]
    return out


def guarded_run_buffers(cfg_tuple, N, E, B, params, fill, dev):
    """Guarded arena, workspace and flat gradient buffer of one training run, all from `fill`
    ("zero" / "ones"), and the gradient views into the flat buffer per parameter, as
    functional._function_backward lays them out (None where the parameter is None)
    -> ({"arena", "ws", "grads": Guarded}, [gradient views])."""
    from cgr_mpnn_3D._amd import native
    from cgr_mpnn_3D._amd.functional import _grad_views, make_config

    lib, cfg = native.load(), make_config(*cfg_tuple)
    geo, _, total = _grad_views(params, cfg.depth)
    bufs = {"arena": Guarded(lib.cgr_gnn_arena_bytes(ctypes.byref(cfg), N, E, B), fill, dev),
            "ws": Guarded(lib.cgr_gnn_workspace_bytes(ctypes.byref(cfg), N, E, B), fill, dev),
            "grads": Guarded(4 * total, fill, dev)}
    flat = bufs["grads"].floats(total)
    grads = [None if p is None else flat[o:o + int(np.prod(s, dtype=np.int64))].view(s)
             for p, (s, _, o) in zip(params, geo)]
    return bufs, grads


# -------------------------------------------------------------------------------------------------
# records and the three-fill check
# -------------------------------------------------------------------------------------------------
def flat(rec):
    """(name, array) of every array of a record: a dict of arrays, of lists of arrays (None
    entries skipped) and of dicts of arrays."""
    for k, v in rec.items():
        if isinstance(v, (np.ndarray, torch.Tensor)):
            yield k, v
        elif isinstance(v, (list, tuple)):
            for i, t in enumerate(v):
                if t is not None:
                    yield f"{k}[{i}]", t
        elif isinstance(v, dict):
            yield from ((f"{k}.{n}", t) for n, t in v.items() if t is not None)


def diff_report(a, b):
    """None when two records hold the same buffers with the same bytes; else a line naming the
    first differing buffer and element."""
    fa, fb = list(flat(a)), list(flat(b))
    if [k for k, _ in fa] != [k for k, _ in fb]:
        return f"buffers differ: {[k for k, _ in fa]} vs {[k for k, _ in fb]}"
    for (k, u), (_, v) in zip(fa, fb):
        u, v = np.asarray(u), np.asarray(v)
        if u.shape != v.shape or u.dtype != v.dtype:
            return f"{k}: {u.dtype}{u.shape} vs {v.dtype}{v.shape}"
        if u.tobytes() == v.tobytes():
            continue
        ub = u.reshape(-1).view(np.uint8).reshape(u.size, -1)
        vb = v.reshape(-1).view(np.uint8).reshape(v.size, -1)
        bad = np.flatnonzero((ub != vb).any(axis=1))
        at = tuple(int(i) for i in np.unravel_index(bad[0], u.shape)) if u.shape else ()
        return (f"{k}: {bad.size} of {u.size} elements differ, first at {at}: "
                f"{u.reshape(-1)[bad[0]]!r} vs {v.reshape(-1)[bad[0]]!r}")
    return None


def byte_runs(mask):
    """[(lo, hi)] of every maximal run of True in a 1-D bool array."""
    edges = np.flatnonzero(np.diff(np.concatenate([[False], mask, [False]]).astype(np.int8)))
    return [(int(lo), int(hi)) for lo, hi in zip(edges[::2], edges[1::2])]


class Outcome:
    """One run: its Guarded buffers by name, the slack ranges of those that have a layout
    ({buffer name: [(region, lo, hi)]}), and the record of everything it computed."""

    def __init__(self, buffers, record, slack=None):
        self.buffers, self.record, self.slack = buffers, record, slack or {}

    def verify(self, what=""):
        for name, g in self.buffers.items():
            g.check_guards(f"{what}{name}")
        for name, ranges in self.slack.items():
            self.buffers[name].check_slack(ranges, f"{what}{name}")


def check_fills(runner, fills=FILLS, what=""):
    """runner(fill) -> Outcome, once per fill ("zero", "ones", "stale": the runner turns the name
    into Guarded buffers).  Every run's guards and slack intact; every record bit-identical to
    the first fill's.  Returns {fill: Outcome}."""
    outs = {}
    for fill in fills:
        outs[fill] = o = runner(fill)
        o.verify(f"{what} [{fill}] ")
    first = fills[0]
    for fill in fills[1:]:
        d = diff_report(outs[first].record, outs[fill].record)
        assert d is None, f"{what}: result depends on the buffers' contents on entry " \
                          f"({first} vs {fill} fill): {d}"
    return outs
