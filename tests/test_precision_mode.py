"""CPU: the precision switch (config.precision / CGR_PRECISION -> cgr_gnn_config.precision, ABI 9)
through the Python layer and the library's host-side queries, and the arithmetic fact the GPU
tests of the mode (tests/test_gpu_precision.py) rest on: the default mode's weight-gradient
arithmetic, evaluated with exact accumulation, is outside the plain fp32-class bar that the
"fp32" mode is held to, while an honest fp32 product is inside it."""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from stagewise_common import TORCH_F32

from cgr_mpnn_3D._amd import config, functional, native
from oracle import stagewise as sw

N2, E2, B2 = 7680, 15360, 256  # cfg2's batch, as tests/test_abi.py sizes it


@pytest.fixture
def restore_precision():
    was = config.precision
    yield
    config.precision = was


def _cfg(precision, F=846, Fe=14, H=400, D=4, act=0, skip=0):
    return native.CgrGnnConfig(F, Fe, H, D, act, skip, 0, 0, precision)


def test_switch_parsing_and_make_config(restore_precision):
    assert config.PRECISIONS == ("split", "fp32")
    assert (native.PRECISION_SPLIT, native.PRECISION_FP32) == (0, 1)
    config.precision = "split"
    assert functional.make_config(10, 2, 8, 1, 0, False).precision == 0
    assert native.CgrGnnConfig(10, 2, 8, 1, 0, 0).precision == 0  # six positional arguments
    config.precision = "fp32"
    assert config.precision_code() == 1
    assert functional.make_config(10, 2, 8, 1, 0, False).precision == 1
    # an explicit argument wins over the switch, either way
    assert functional.make_config(10, 2, 8, 1, 0, False, precision=0).precision == 0
    config.precision = "split"
    assert functional.make_config(10, 2, 8, 1, 0, False, 0, 0, 1).precision == 1
    # a tuple of eight follows the switch as it stands at the call; a ninth element is kept
    t8 = (10, 2, 8, 1, 0, False, 0, 0)
    assert functional.resolve_config_tuple(t8) == t8 + (0,)
    config.precision = "fp32"
    assert functional.resolve_config_tuple(t8) == t8 + (1,)
    assert functional.resolve_config_tuple(t8 + (0,)) == t8 + (0,)
    assert functional.make_config(*functional.resolve_config_tuple(t8)).precision == 1
    for bad in ("bf16", "FP32", "", 1, None):
        with pytest.raises(ValueError):
            config.precision = bad
        assert config.precision == "fp32"  # a refused assignment changes nothing
    with pytest.raises(ValueError):
        config.precision_code("double")


@pytest.mark.parametrize("value, ok", [("fp32", True), ("split", True), ("", True),
                                       ("exact", False)])
def test_environment_variable_initialises_the_switch(value, ok):
    env = dict(os.environ, CGR_PRECISION=value, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, "-c",
                        "from cgr_mpnn_3D._amd import config; print(config.precision)"],
                       env=env, capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip() == (value or "split")
    else:
        assert r.returncode != 0 and "ValueError" in r.stderr and "exact" in r.stderr


def test_unknown_precision_is_rejected_with_message():
    lib = native.load()
    assert lib.cgr_abi_version() == 9 == native.ABI_VERSION
    assert lib.cgr_gnn_num_params(ctypes.byref(_cfg(1))) == 6 + 8
    for bad in (2, -1):
        c = _cfg(bad)
        assert lib.cgr_gnn_num_params(ctypes.byref(c)) == -1
        assert b"precision" in lib.cgr_last_error()
        assert lib.cgr_gnn_arena_bytes(ctypes.byref(c), N2, E2, B2) == -1
        assert lib.cgr_gnn_workspace_bytes(ctypes.byref(c), N2, E2, B2) == -1
        assert lib.cgr_gnn_predict_arena_bytes(ctypes.byref(c), N2, E2, B2) == -1
        assert lib.cgr_gnn_image_bytes(ctypes.byref(c)) == -1


@pytest.mark.parametrize("shape", [dict(), dict(H=128, act=1, skip=1), dict(H=37, F=85, D=2),
                                   dict(H=528, D=2), dict(H=1000, skip=1)])
def test_size_and_offset_queries_answer_in_both_modes(shape):
    lib = native.load()
    sizes = {}
    for mode in (0, 1):
        c = _cfg(mode, **shape)
        a = lib.cgr_gnn_arena_bytes(ctypes.byref(c), N2, E2, B2)
        w = lib.cgr_gnn_workspace_bytes(ctypes.byref(c), N2, E2, B2)
        p = lib.cgr_gnn_predict_arena_bytes(ctypes.byref(c), N2, E2, B2)
        im = lib.cgr_gnn_image_bytes(ctypes.byref(c))
        assert min(a, w, p, im) > 0
        assert p < a
        Hp = (c.hidden + 3) // 4 * 4
        for name, idx in [("h", 0), ("h", c.depth), ("a", c.depth), ("hn", 0), ("perm", 0),
                          ("P", 0), ("g", 0)]:
            off = lib.cgr_gnn_arena_offset(ctypes.byref(c), N2, E2, B2, name.encode(), idx)
            assert 0 <= off < a and off % 256 == 0, (mode, name, idx)
        offs = [lib.cgr_gnn_workspace_offset(ctypes.byref(c), N2, E2, B2, n.encode(), i)
                for n, i in (("dpre", 0), ("dpre", c.depth - 1), ("dpre0", 0), ("ds", 0))]
        assert all(0 <= o and o % 256 == 0 for o in offs) and len(set(offs)) == 3 + (c.depth > 1)
        assert max(offs[:3]) + E2 * Hp * 4 <= w and offs[3] + N2 * Hp * 4 <= w
        assert offs[1] - offs[0] == (c.depth - 1) * E2 * Hp * 4
        assert lib.cgr_gnn_workspace_offset(ctypes.byref(c), N2, E2, B2, b"Gs", 0) == -1
        sizes[mode] = (a, w, p, im)
    # the modes pack their weight images in tilings of their own and "fp32" has no e-images, so
    # the byte counts differ; the fp32 activations both hold set a common floor
    Hp, D = (c.hidden + 3) // 4 * 4, c.depth
    for a, w, p, im in sizes.values():
        assert a > (D + 1) * (E2 + N2) * Hp * 4 and w > (D + 2) * E2 * Hp * 4
        assert p > 3 * E2 * Hp * 4 and im >= 3 * D * c.hidden * c.hidden * 2


# ---------------------------------------------------------------------------------------------
# The bars tell the modes apart.  (R, n, k) are weight-gradient shapes of the GPU cases: rows
# summed over, gradient-side width, operand width.  The operands are drawn in this order from one
# generator, so the figures are reproducible: rho of the emulation 131.9 / 61.7 / 42.6 / 36.6
# against bars 19.3 / 19.1 / 11.2 / 16.1 (the bars move a little with the BLAS summation order
# behind rho_ref; the test prints what it measured).
# ---------------------------------------------------------------------------------------------
TN_SHAPES = [(84, 37, 122), (192, 37, 37), (816, 128, 128), (960, 400, 400)]


@pytest.fixture(scope="module")
def tn_operands():
    rng = np.random.default_rng(0)
    out = []
    for R, n, k in TN_SHAPES:
        a = rng.standard_normal((R, n)) * 10.0 ** rng.uniform(-2.0, 1.0, (R, 1))
        b = rng.standard_normal((R, k))
        out.append((a.astype(np.float32), b.astype(np.float32)))
    return out


@pytest.mark.parametrize("i", range(len(TN_SHAPES)), ids=[str(s) for s in TN_SHAPES])
def test_default_mode_weight_gradient_arithmetic_is_outside_the_plain_bar(i, tn_operands):
    a, b = tn_operands[i]
    st = sw.tn(a, b)  # float64, S = |a|^T |b|
    rho_ref = sw.rho(sw.tn(a, b, ops=TORCH_F32).ref, st)[0]
    bar = sw.bar(rho_ref)
    rho_em = sw.rho(sw.tn_emulated(a, b), st)[0]
    print(f"{TN_SHAPES[i]}: rho(emulation) {rho_em:.1f}  rho_ref {rho_ref:.2f}  bar {bar:.1f}")
    assert rho_ref <= bar  # torch fp32 itself is inside
    assert rho_em > bar  # two-piece operands, three products: outside, even summed exactly
