"""Process-wide switches of the native path."""

import os
import sys

# strict: after every forward, read the graph-prep status word (one device->host sync) and raise
# on out-of-range edge indices / unsorted batch vectors, and check the reference's
# N' = max(dst) + 1 == num_nodes contract (GNN.py:106 fails with RuntimeError otherwise).
strict = os.environ.get("CGR_STRICT", "0") not in ("", "0", "false", "False")

# Called as hook(flat, buckets, events) after every native backward is enqueued (before the
# per-parameter views are handed to autograd): flat = the fp32 gradient buffer, buckets = its
# (start, end) ranges in the order the backward finishes them, events = their ready events (or
# None; see functional.grad_layout and ddp.GradAllReduce).  cgr_mpnn_3D._amd.ddp installs the
# RCCL all-reduce here.
grad_bucket_hook = None

# precision: the arithmetic of the GNN kernels (enum cgr_precision, include/cgr_mpnn3d.h).
#   "split"  the default: split-bf16 NT GEMMs accumulating in the matrix core's running sum, the
#            two-piece e-image TN for the weight gradients (H <= 512)
#   "fp32"   fp32-faithful: every NT k step summed on its own and folded in with one fp32 add,
#            every weight gradient on an fp32 TN family (slower, §9)
# Initialised from CGR_PRECISION; any other value raises ValueError, here and at assignment.  A
# config tuple without a ninth element takes the value current when the call is made
# (functional.make_config); a captured graph keeps the mode it was captured in.
PRECISIONS = ("split", "fp32")  # index = enum cgr_precision


def precision_code(value=None) -> int:
    """enum cgr_precision of `value` ("split" / "fp32"); None: the process switch."""
    return PRECISIONS.index(_checked(precision if value is None else value))


def _checked(value):
    if not isinstance(value, str) or value not in PRECISIONS:
        raise ValueError(f"cgr_mpnn_3D: precision must be one of {PRECISIONS}, got {value!r}")
    return value


precision = _checked(os.environ.get("CGR_PRECISION") or "split")


class _Config(sys.modules[__name__].__class__):
    """This module with a validated `precision` attribute."""

    def __setattr__(self, name, value):
        if name == "precision":
            _checked(value)
        super().__setattr__(name, value)


sys.modules[__name__].__class__ = _Config
