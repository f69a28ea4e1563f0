"""CPU: what the arena-contract checks (tests/arena_contract_common.py, used on the GPU by
tests/test_gpu_arena_contract.py) can tell apart, and the layout algebra they rest on.

1. The layouts through the host-only size and offset queries, over a fixed-seed sample of
   configurations: which named buffers exist, alignment, no overlap, everything inside the
   reported bytes, sizes monotone in N, E and B.
2. The harness itself on CPU tensors with a fake runner: each planted violation -- a write one
   byte past or before the payload, a write into a slack range, an output that copies a stale
   byte of a region nobody wrote, an output that differs only under the stale fill -- is flagged,
   and a runner that does none of these passes.
"""

import ctypes
import types

import numpy as np
import pytest
import torch

from arena_contract_common import (ALIGN, FILLS, GUARD_BYTE, GUARD_BYTES, Guarded, Outcome,
                                   byte_runs, check_fills, diff_report, named_regions,
                                   slack_ranges)

from cgr_mpnn_3D._amd import native
from cgr_mpnn_3D._amd.functional import make_config

NS = (1, 2, 63, 64, 65, 147, 320)
ES = (2, 4, 62, 64, 66, 322, 1056, 4096, 4098)
HS = (1, 3, 4, 12, 37, 39, 64, 100, 400, 512, 513, 516, 521, 1000)
FS = (0, 1, 80, 85, 118)
FES = (0, 3, 14)
DS = (1, 3, 32)
ACTS = (native.ACT_RELU, native.ACT_SILU)
SAMPLE = 320
MAX_DEPTH = native.MAX_DEPTH


def _sample():
    rng = np.random.default_rng(20264)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]  # noqa: E731
    out = []
    for _ in range(SAMPLE):
        N = pick(NS)
        out.append(dict(N=N, E=pick(ES), B=pick((1, min(N, 7))), H=pick(HS), F=pick(FS),
                        Fe=pick(FES), D=pick(DS), act=pick(ACTS), aggr=pick((0, 1)),
                        pool=pick((0, 1, 2)), skip=pick((0, 1)), prec=pick((0, 1))))
    return out


def _cfg(c):
    return make_config(c["F"], c["Fe"], c["H"], c["D"], c["act"], c["skip"], c["aggr"], c["pool"],
                       c["prec"])


def _sizes(cfg, N, E, B):
    lib, r = native.load(), ctypes.byref(cfg)
    return (lib.cgr_gnn_arena_bytes(r, N, E, B), lib.cgr_gnn_workspace_bytes(r, N, E, B),
            lib.cgr_gnn_predict_arena_bytes(r, N, E, B))


def test_sample_is_large_and_spans_the_value_sets():
    s = _sample()
    assert len(s) >= 300
    for key, values in (("N", NS), ("E", ES), ("H", HS), ("F", FS), ("Fe", FES), ("D", DS),
                        ("act", ACTS), ("pool", (0, 1, 2)), ("aggr", (0, 1)), ("prec", (0, 1))):
        assert {c[key] for c in s} == set(values), key
    assert {c["B"] for c in s} >= {1, 2, 7}


def test_named_buffers_exist_exactly_where_the_config_has_them():
    lib = native.load()
    for c in _sample():
        cfg, dims = _cfg(c), (c["N"], c["E"], c["B"])

        def off(name, index=0):
            return lib.cgr_gnn_arena_offset(ctypes.byref(cfg), *dims, name.encode(), index)

        relu = c["act"] == native.ACT_RELU
        for name in ("status", "rng", "perm", "src_s", "dst_s", "rev_s", "src_list", "dst_ptr",
                     "src_ptr", "graph_ptr", "node_graph", "P", "Q", "hn", "g"):
            assert off(name) >= 0, (c, name)
        assert (off("e_s") >= 0) == (c["Fe"] > 0), c
        assert (off("zn") >= 0) == (not relu), c
        for l in range(MAX_DEPTH + 2):
            assert (off("h", l) >= 0) == (l <= c["D"]), (c, l)
            assert (off("a", l) >= 0) == (l <= c["D"]), (c, l)
            assert (off("pre", l) >= 0) == (l <= c["D"] and not relu), (c, l)
        assert off("h", -1) == -1 and off("no_such_buffer") == -1

        def woff(name, index=0):
            return lib.cgr_gnn_workspace_offset(ctypes.byref(cfg), *dims, name.encode(), index)

        for l in range(MAX_DEPTH + 1):
            assert (woff("dpre", l) >= 0) == (l < c["D"]), (c, l)
        assert woff("dpre0") >= 0 and woff("ds") >= 0 and woff("dzn_main") >= 0
        assert woff("dzn") == -1 and woff("Gs") == -1 and woff("dm") == -1


def test_named_regions_are_aligned_disjoint_and_inside_the_reported_bytes():
    lib = native.load()
    for c in _sample():
        cfg, dims = _cfg(c), (c["N"], c["E"], c["B"])
        arena_bytes, ws_bytes, predict_bytes = _sizes(cfg, *dims)
        assert arena_bytes > 0 and ws_bytes > 0 and predict_bytes > 0, c
        regs = named_regions(cfg, *dims)
        status = lib.cgr_gnn_arena_offset(ctypes.byref(cfg), *dims, b"status", 0)
        for kind, total in (("arena", arena_bytes), ("ws", ws_bytes)):
            rs = sorted(regs[kind], key=lambda r: r[1])
            if kind == "arena":
                assert 0 <= status and status + 4 <= rs[0][1], c  # in the zero block, in front
            for name, o, size in rs:
                assert o % ALIGN == 0, (c, kind, name, o)
                assert o + size <= total, (c, kind, name, o, size, total)
            for (n0, o0, s0), (n1, o1, _) in zip(rs, rs[1:]):
                assert o0 + s0 <= o1, (c, kind, n0, n1)
        # the predict arena holds the prefix the two layouts share (bookkeeping .. Q)
        prefix = [r for r in regs["arena"] if "[" not in r[0] and r[0] not in ("zn", "hn", "g")]
        assert {r[0] for r in prefix} >= {"rng", "perm", "graph_ptr", "node_graph", "P", "Q"}
        assert max(o + s for _, o, s in prefix) <= predict_bytes, c


def test_sizes_are_monotone_in_nodes_edges_and_graphs():
    for c in _sample():
        cfg = _cfg(c)
        walks = ([(N, c["E"], c["B"]) for N in NS if N >= c["B"]],
                 [(c["N"], E, c["B"]) for E in ES],
                 [(c["N"], c["E"], B) for B in range(1, min(c["N"], 7) + 1)])
        for walk in walks:
            sizes = [_sizes(cfg, *dims) for dims in walk]
            for (d0, s0), (d1, s1) in zip(zip(walk, sizes), zip(walk[1:], sizes[1:])):
                assert all(a <= b for a, b in zip(s0, s1)), (c, d0, s0, d1, s1)


def test_slack_ranges_are_the_rounding_of_each_logical_size():
    c = dict(N=65, E=66, B=2, H=37, F=5, Fe=3, D=2, act=native.ACT_SILU, aggr=0, pool=2, skip=1,
             prec=0)
    run = types.SimpleNamespace(cfg=_cfg(c), N=65, E=66, B=2)
    regs = named_regions(run.cfg, 65, 66, 2)
    sl = slack_ranges(run)
    by = {k: {n: (lo, hi) for n, lo, hi in v} for k, v in sl.items()}
    off = {k: {n: (o, s) for n, o, s in v} for k, v in regs.items()}
    assert set(off["arena"]) >= {"rng", "perm", "src_s", "dst_s", "rev_s", "src_list", "dst_ptr",
                                 "src_ptr", "graph_ptr", "node_graph", "e_s", "P", "Q", "h[0]",
                                 "h[2]", "a[2]", "pre[2]", "zn", "hn", "g"}
    assert "h[3]" not in off["arena"] and set(off["ws"]) == {"dpre", "dpre0", "ds", "dzn_main"}
    o = off["arena"]["perm"][0]
    assert by["arena"]["perm"] == (o + 264, o + 512)  # 4 E = 264
    o = off["arena"]["rng"][0]
    assert by["arena"]["rng"] == (o + 8, o + 256)
    o = off["arena"]["e_s"][0]
    assert by["arena"]["e_s"] == (o + 4 * 66 * 4, o + 1280)  # Fep = 4
    o = off["arena"]["hn"][0]
    assert by["arena"]["hn"] == (o + 4 * 65 * 40, o + 10496)  # Hp = 40
    o = off["ws"]["dpre"][0]
    assert by["ws"]["dpre"] == (o + 2 * 4 * 66 * 40, o + 21248)
    for kind in sl:
        for name, lo, hi in sl[kind]:
            assert lo < hi and hi % ALIGN == 0 and hi - lo < ALIGN, (kind, name)


# -------------------------------------------------------------------------------------------------
# Guarded, diff_report
# -------------------------------------------------------------------------------------------------
def test_guarded_layout_and_fills():
    assert GUARD_BYTES == 64 * 1024 and GUARD_BYTES % 4096 == 0 and GUARD_BYTE == 0xA5
    assert FILLS == ("zero", "ones", "stale")
    for n in (0, 1, 8, 1000):
        for fill, byte in (("zero", 0x00), ("ones", 0xFF)):
            g = Guarded(n, fill, "cpu")
            assert g.payload.numel() == n and g.lead >= GUARD_BYTES
            assert g.buf.numel() - g.lead - n >= GUARD_BYTES
            assert n == 0 or g.payload.data_ptr() % ALIGN == 0
            assert (g.bytes() == byte).all()
            assert (g.buf[:g.lead] == GUARD_BYTE).all() and (g.buf[g.lead + n:] == GUARD_BYTE).all()
            g.check_guards()
    ones = Guarded(16, "ones", "cpu")
    assert torch.isnan(ones.floats(4)).all()  # fp32 NaN
    assert (ones.payload.view(torch.int32) == -1).all()  # int32 -1
    assert torch.isnan(ones.payload.view(torch.bfloat16).float()).all()  # bf16 NaN
    stale = np.arange(1, 11, dtype=np.uint8)
    assert Guarded(25, stale, "cpu").bytes().tolist() == (list(range(1, 11)) * 3)[:25]  # tiled
    assert Guarded(4, torch.from_numpy(stale), "cpu").bytes().tolist() == [1, 2, 3, 4]  # truncated
    f = Guarded(8, np.array([1.0, 2.0, 3.0], np.float32), "cpu")  # any dtype: its bytes
    assert f.floats(2).tolist() == [1.0, 2.0]


def test_diff_report_names_the_first_differing_buffer_and_element():
    a = {"y": np.zeros(3, np.float32), "h": [np.zeros((2, 3), np.float32), None],
         "grads": {"w": np.ones(4, np.float32)}}
    b = {"y": np.zeros(3, np.float32), "h": [np.zeros((2, 3), np.float32), None],
         "grads": {"w": np.ones(4, np.float32)}}
    assert diff_report(a, b) is None
    b["h"][0][1, 2] = np.float32("nan")
    b["grads"]["w"][0] = 2
    r = diff_report(a, b)
    assert r.startswith("h[0]: 1 of 6 elements differ, first at (1, 2)"), r
    a["h"][0][1, 2] = np.float32("nan")  # equal bytes: NaN == NaN here
    assert diff_report(a, b).startswith("grads.w: 1 of 4")
    a["y"] = -a["y"]  # -0.0 and 0.0 differ in bytes
    assert diff_report(a, b).startswith("y: 3 of 3")
    del b["grads"]
    assert diff_report(a, b).startswith("buffers differ")


def test_byte_runs():
    m = np.array([1, 1, 0, 0, 1, 0, 1], bool)
    assert byte_runs(m) == [(0, 2), (4, 5), (6, 7)]
    assert byte_runs(np.zeros(4, bool)) == [] and byte_runs(np.ones(3, bool)) == [(0, 3)]


# -------------------------------------------------------------------------------------------------
# the harness on CPU tensors with a fake runner
# -------------------------------------------------------------------------------------------------
# the fake library's arena: region "a" [0, 100), slack [100, 256); region "b" [256, 656), slack
# [656, 768); region "unused" [768, 868) that this level never writes, slack [868, 1024)
ARENA = 1024
SLACK = [("a", 100, 256), ("b", 656, 768), ("unused", 868, 1024)]
STALE = ((np.arange(4096) * 7) % 251 + 2).astype(np.uint8)  # no byte 0x00, 0x01 or 0xFF


def _fake_runner(fault=None):
    """a = x + 1 (100 bytes), b = 3 a tiled (100 floats), out = sum(b); `fault` plants one
    violation of the contract."""
    x = np.arange(100, dtype=np.uint8)

    def runner(fill):
        arena = Guarded(ARENA, STALE if fill == "stale" else fill, "cpu")
        out = Guarded(4, STALE[100:] if fill == "stale" else fill, "cpu")
        entry = arena.bytes()  # what the buffer held when the call began
        p = arena.payload
        p[0:100] = torch.from_numpy(x + 1)
        b = p[256:656].view(torch.float32)
        b[:] = 3.0 * p[0:100].float()
        y = b.sum()
        if fault == "past_end":
            arena.buf[arena.lead + ARENA] = 0
        elif fault == "before_start":
            arena.buf[arena.lead - 1] = 0
        elif fault == "out_past_end":
            out.buf[out.lead + 4] = 1
        elif fault == "slack":
            p[100] = 9
        elif fault == "last_slack_byte":
            p[1023] = 9
        elif fault == "reads_unwritten":  # one byte of the region no kernel of this level wrote
            y = y + float(entry[800])
        elif fault == "stale_only":  # the same under 0x00 and 0xFF, different under a stale word
            word = int(entry[768:772].view(np.int32)[0])
            y = y + (0.0 if word in (0, -1) else 1.0)
        out.floats(1)[0] = y
        rec = {"out": out.floats(1).numpy().copy(), "a": p[0:100].numpy().copy(),
               "b": b.numpy().copy()}
        return Outcome({"arena": arena, "out": out}, rec, {"arena": SLACK})

    return runner


def test_a_clean_runner_passes():
    outs = check_fills(_fake_runner(), what="clean")
    assert set(outs) == set(FILLS)
    assert outs["stale"].buffers["arena"].bytes()[768:868].tolist() == STALE[768:868].tolist()


@pytest.mark.parametrize("fault,message", [
    ("past_end", r"arena: 1 guard bytes changed, offsets 1024 \.\. 1024"),
    ("before_start", r"arena: 1 guard bytes changed, offsets -1 \.\. -1"),
    ("out_past_end", r"out: 1 guard bytes changed, offsets 4 \.\. 4"),
    ("slack", r"arena: slack after a written: 1 bytes, offsets 100 \.\. 100"),
    ("last_slack_byte", r"arena: slack after unused written: 1 bytes, offsets 1023 \.\. 1023"),
    ("reads_unwritten", r"depends on the buffers' contents on entry \(zero vs ones fill\): out"),
    ("stale_only", r"depends on the buffers' contents on entry \(zero vs stale fill\): out"),
])
def test_each_planted_violation_is_flagged(fault, message):
    with pytest.raises(AssertionError, match=message):
        check_fills(_fake_runner(fault), what="planted")


def test_stale_only_violation_passes_the_two_constant_fills():
    # why the third fill is there: 0x00 and 0xFF alone do not see this one
    check_fills(_fake_runner("stale_only"), fills=("zero", "ones"), what="two fills")
