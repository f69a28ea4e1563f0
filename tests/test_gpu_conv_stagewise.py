"""GPU: the standalone DMPNNConv (csrc/conv.hip) and the bare segment sum (cgr_segment_sum), stage
by stage against float64 (oracle/stagewise.conv_stages), as tests/test_gpu_stagewise.py judges
the model's stages: rho = max (|got - ref|)+ / (u S) <= max(8, 4 rho_ref), rho_ref torch fp32 on
the CPU for the same stage from the same inputs.

The conv is the only user of the LDS-staged fp32 NT GEMM with the pair-order loader
(LdGatherDiff<true>) and an unpadded output (EpStore, ld = H), of the LDS-staged fp32 TN at any H
(the 80-wide tile shapes, Kout <= 16), and of k_add_rows / k_conv_dh.  The C ABI is called
directly so that the NULL-gradient branches, which autograd never takes, are reached.

Every case also asserts that
* a second run reproduces every output bit for bit (the first run's scratch holds NaN bit
  patterns, the second's what the first left there: no output depends on the scratch's content);
* every output sits inside a larger sentinel-filled buffer whose bytes outside the logical
  [rows, width] region are unchanged afterwards, as are guard bytes either side of the scratch.
"""

import numpy as np
import pytest
import torch

from stagewise_common import CONV_CASES, TORCH_F32, conv_inputs, failures, write_report

from cgr_mpnn_3D._amd import native
from oracle import stagewise as sw

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e33  # finite, no kernel's output
GUARD = 64  # floats either side of an output (keeps the logical region 16-byte aligned)
SCRATCH_GUARD = 1024  # bytes either side of the scratch


class Guarded:
    """A [rows, ld] fp32 output whose first `width` columns are logical, inside a sentinel-filled
    buffer: GUARD floats, `offset` floats (a deliberately misaligned start), the rows, GUARD."""

    def __init__(self, rows, width, dev, ld=None, offset=0):
        ld = width if ld is None else ld
        self.rows, self.width, self.ld = rows, width, ld
        self.lo = GUARD + offset
        self.flat = torch.full((self.lo + rows * ld + GUARD,), SENTINEL, dtype=torch.float32,
                               device=dev)
        self.t = self.flat[self.lo:self.lo + rows * ld].view(rows, ld)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def read(self):
        """The logical region; asserts every other byte of the buffer still holds the sentinel."""
        flat = self.flat.cpu().numpy()
        inside = np.zeros(flat.shape, bool)
        body = inside[self.lo:self.lo + self.rows * self.ld].reshape(self.rows, self.ld)
        body[:, :self.width] = True
        want = np.float32(SENTINEL).view(np.uint32)
        touched = np.flatnonzero((flat.view(np.uint32) != want) & ~inside)
        assert touched.size == 0, f"writes outside the logical region at floats {touched[:8]}"
        out = flat[self.lo:self.lo + self.rows * self.ld].reshape(self.rows, self.ld)
        return out[:, :self.width].copy()


class Scratch:
    def __init__(self, nbytes, dev):
        self.n = nbytes
        self.buf = torch.full((nbytes + 2 * SCRATCH_GUARD,), 0xFF, dtype=torch.uint8, device=dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + SCRATCH_GUARD

    def check_guards(self):
        b = self.buf.cpu().numpy()
        assert (b[:SCRATCH_GUARD] == 0xFF).all() and (b[SCRATCH_GUARD + self.n:] == 0xFF).all(), \
            "writes outside the scratch"


def _conv_abi(i, dev, scratch=None):
    """One forward + backward through the C ABI; {a, out, grad_h, grad_weight, grad_bias}."""
    lib = native.load()
    E, H = i["h"].shape
    N = i["N"]
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    ei, h, w, b, ga, go = (up(i[k]) for k in ("edge_index", "h", "weight", "bias", "grad_a",
                                               "grad_out"))
    if scratch is None:
        scratch = Scratch(lib.cgr_dmpnn_conv_scratch_bytes(N, E, H), dev)
    assert scratch.ptr % 16 == 0
    out = dict(a=Guarded(N, H, dev), out=Guarded(E, H, dev), grad_h=Guarded(E, H, dev),
               grad_weight=Guarded(H, H, dev), grad_bias=Guarded(1, H, dev))
    aggr = 1 if i["mean"] else 0
    st = native.stream_ptr(dev)
    with native.device_guard(dev):
        native.check(lib.cgr_dmpnn_conv_forward(native.ptr(ei), N, E, native.ptr(h), H,
                                                native.ptr(w), native.ptr(b), out["a"].ptr,
                                                out["out"].ptr, scratch.ptr, aggr, st))
        native.check(lib.cgr_dmpnn_conv_backward(native.ptr(ei), N, E, native.ptr(h), H,
                                                 native.ptr(w), native.ptr(ga), native.ptr(go),
                                                 out["grad_h"].ptr, out["grad_weight"].ptr,
                                                 out["grad_bias"].ptr, scratch.ptr, aggr, st))
    torch.cuda.synchronize()
    got = {k: g.read() for k, g in out.items()}
    got["grad_bias"] = got["grad_bias"][0]
    scratch.check_guards()
    return got, scratch


def _record(i, got):
    rec = dict(edge_index=i["edge_index"], N=i["N"], h=i["h"], weight=i["weight"], bias=i["bias"],
               grad_a=i["grad_a"], grad_out=i["grad_out"], inv_deg=None, **got)
    if i["mean"]:
        rec["inv_deg"] = 1.0 / np.maximum(np.bincount(i["edge_index"][1], minlength=i["N"]), 1)
    return rec


def _judge(case, rec):
    rows = sw.conv_judge(rec, TORCH_F32)
    write_report(case, rows)
    for r in rows:
        print(f"{case:>22s} {r['stage']:<12s} rho {r['rho']:9.2f}  rho_ref {r['rho_ref']:7.2f}  "
              f"bar {r['bar']:7.2f}  at {r['argmax']}")
    bad = failures(rows)
    assert not bad, f"{case}:\n" + "\n".join(bad)


@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_conv_abi_every_stage(case, cuda_device):
    i = conv_inputs(case)
    got, scratch = _conv_abi(i, cuda_device)
    again, _ = _conv_abi(i, cuda_device, scratch)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), f"{case}: {k} differs between two runs"
    _judge("conv_" + case, _record(i, got))


@pytest.mark.parametrize("case", ["h100", "sparse_mean_h45"])
def test_conv_module_every_stage(case, cuda_device):
    """The same stages through the public DMPNNConv module and autograd (the Python plumbing:
    the inferred node count, the aggregation argument, the order of the returned gradients)."""
    from cgr_mpnn_3D.models.GNN import DMPNNConv

    i = dict(conv_inputs(case))
    H = i["h"].shape[1]
    i["N"] = int(i["edge_index"][1].max()) + 1  # what the module infers, as PyG does
    i["grad_a"] = np.ascontiguousarray(i["grad_a"][:i["N"]])

    def run():
        conv = DMPNNConv(H, aggr="mean" if i["mean"] else "add")
        with torch.no_grad():
            conv.lin.weight.copy_(torch.from_numpy(i["weight"]))
            conv.lin.bias.copy_(torch.from_numpy(i["bias"]))
        conv = conv.to(cuda_device)
        h = torch.from_numpy(i["h"]).to(cuda_device).requires_grad_(True)
        a, out = conv(torch.from_numpy(i["edge_index"]).to(cuda_device), h)
        ((a * torch.from_numpy(i["grad_a"]).to(cuda_device)).sum()
         + (out * torch.from_numpy(i["grad_out"]).to(cuda_device)).sum()).backward()
        torch.cuda.synchronize()
        assert a.shape == (i["N"], H)
        return {k: t.detach().cpu().numpy().copy() for k, t in
                dict(a=a, out=out, grad_h=h.grad, grad_weight=conv.lin.weight.grad,
                     grad_bias=conv.lin.bias.grad).items()}

    got, again = run(), run()
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), f"{case}: {k} differs between two runs"
    _judge("conv_module_" + case, _record(i, got))


# ---------------------------------------------------------------------------------------------
# cgr_segment_sum
# ---------------------------------------------------------------------------------------------
def _segments(nseg, rng, lengths=(0, 1, 2, 3, 4), long=(300, 300)):
    """Segment lengths cycling through `lengths` in a shuffled order, `long` ones mixed in."""
    n = np.asarray([lengths[j % len(lengths)] for j in range(nseg)], np.int64)
    rng.shuffle(n)
    n[rng.choice(nseg, len(long), replace=False)] = long
    ptr = np.zeros(nseg + 1, np.int32)
    ptr[1:] = np.cumsum(n)
    return ptr


# name: (segments, width, ld, pointer offset in floats, all segments empty)
SEGSUM_LAYOUTS = {
    "w64_ld64": (300, 64, 64, 0, False),  # the float4 kernel, an even item count
    "w64_ld80": (300, 64, 80, 0, False),
    "w64_offset4": (300, 64, 64, 1, False),  # the scalar kernel although width % 4 == 0
    "w3": (300, 3, 3, 0, False),
    "odd_items": (301, 12, 12, 0, False),  # 903 float4 items: the last thread's second is past
    "all_empty": (300, 64, 64, 0, True),  # a zero-row `vals`
}


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("layout", sorted(SEGSUM_LAYOUTS))
def test_segment_sum_abi(layout, gather, cuda_device):
    import zlib

    lib = native.load()
    nseg, width, ld, offset, empty = SEGSUM_LAYOUTS[layout]
    rng = np.random.default_rng(zlib.crc32(layout.encode()) + gather)
    ptr = np.zeros(nseg + 1, np.int32) if empty else _segments(nseg, rng)
    total = int(ptr[-1])
    assert empty or {0, 1, 2, 3, 4, 300} <= set(np.diff(ptr).tolist())
    rows = 0 if empty else total + 17  # (gather: more rows than are summed)
    vals = rng.standard_normal((rows, ld)).astype(np.float32)
    idx = rng.permutation(rows)[:total].astype(np.int32) if gather else None
    src = idx.astype(np.int64) if gather else np.arange(total)
    seg_of = np.repeat(np.arange(nseg), np.diff(ptr))

    # `vals` at the same pointer offset as the output, inside a larger allocation (a zero-row
    # view of it for the empty case: the ABI wants a non-NULL pointer)
    vbuf = torch.zeros(GUARD + offset + rows * ld + GUARD, device=cuda_device)
    vbuf[GUARD + offset:GUARD + offset + rows * ld].view(rows, ld).copy_(torch.from_numpy(vals))
    vptr = vbuf.data_ptr() + 4 * (GUARD + offset)
    dp = torch.from_numpy(ptr).to(cuda_device)
    di = torch.from_numpy(idx).to(cuda_device) if gather else None
    assert vptr % 16 == 4 * offset

    def run():
        out = Guarded(nseg, width, cuda_device, ld=ld, offset=offset)
        with native.device_guard(cuda_device):
            native.check(lib.cgr_segment_sum(vptr, ld, native.ptr(di), native.ptr(dp),
                                             nseg, width, out.ptr, ld,
                                             native.stream_ptr(cuda_device)))
        torch.cuda.synchronize()
        return out.read()  # asserts: no write past `width`, none outside the rows

    got, again = run(), run()
    assert got.tobytes() == again.tobytes()
    if empty:
        assert not got.any()
    row = sw.segsum_judge(got, vals[src, :width], seg_of, nseg, TORCH_F32)
    case = f"segsum_{layout}_{'gather' if gather else 'plain'}"
    write_report(case, [row])
    print(f"{case:>28s} rho {row['rho']:7.2f}  rho_ref {row['rho_ref']:6.2f}  bar {row['bar']:6.2f}")
    bad = failures([row])
    assert not bad, "\n".join(bad)
