"""CPU: the host model of the dropout mask (oracle/dropout.py), which
tests/test_gpu_dropout_mask.py holds every evaluation site of the mask to, bit for bit.

* statistical quality of the hash at fixed seeds: keep fraction, neighbour / cross-layer /
  cross-key correlations as z-scores, every |z| <= 4.5 (DESIGN.md §4 records the measured worst);
* the index's high half (idx >= 2^32: E * H elements no test shape reaches on the device);
* thresh_scale at the edges of p;
* mutation power: five wrong masks at the GPU cases' shapes each differ from the model in >= 1 %
  of the elements while passing the drop-rate check (|rate - p| < 0.01) that used to be the
  suite's only independent statement about the mask.
"""

import itertools

import numpy as np
import pytest

from stagewise_common import MASK_CASES, MASK_D, mask_batch
from oracle import dropout as od

Z_BAR = 4.5
E_Q, H_Q = 512, 64
LAYERS = (0, 1, 2, 3)
PS = (0.02, 0.25, 0.5, 0.9)
SEEDS = (0, 1, 1234567, 2**62 - 1, od.module_seed(0, 1))


# ---------------------------------------------------------------------------------------------
# known answers of the integer pieces (python ints, independent of the numpy arithmetic)
# ---------------------------------------------------------------------------------------------
def _mix32_int(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = x * 0x7FEB352D & 0xFFFFFFFF
    x ^= x >> 15
    x = x * 0x846CA68B & 0xFFFFFFFF
    x ^= x >> 16
    return x


def _hash_int(key, layer, idx):
    k = _mix32_int((key & 0xFFFFFFFF) ^ _mix32_int((key >> 32) + layer * 0x9E3779B9))
    x = ((idx & 0xFFFFFFFF) * 0x9E3779B1 + k) & 0xFFFFFFFF
    x ^= ((idx >> 32) * 0x85EBCA77) & 0xFFFFFFFF
    return _mix32_int(x)


def test_numpy_hash_equals_python_int_arithmetic():
    assert int(od.mix32(0)) == 0 and int(od.mix32(1)) == _mix32_int(1) != 1
    rng = np.random.default_rng(1)
    for key in (0, 1, 2**32, 2**64 - 1, od.module_seed(3, 2)):
        for layer in (0, 1, 5):
            idx = np.concatenate([np.arange(5, dtype=np.uint64),
                                  rng.integers(0, 2**63, 20, dtype=np.uint64)])
            got = od.drop_hash(key, layer, idx)
            assert got.dtype == np.uint32
            assert [int(g) for g in got] == [_hash_int(key, layer, int(i)) for i in idx]


def test_forward_key_and_module_seed():
    assert od.forward_key(5) == 5
    assert od.forward_key(5, 0) == 5 + od.KEY_STEP
    assert od.forward_key(2**64 - 1, 41) == (2**64 - 1 + od.KEY_STEP * 42) % 2**64
    assert od.forward_key(7, 2**64 - 1) == 7  # counter + 1 wraps to 0
    assert od.module_seed(0, 1) == 0xBF58476D1CE4E5B9 % 2**62
    assert od.module_seed(1234, 2) == (1234 * 0x9E3779B97F4A7C15 + 2 * 0xBF58476D1CE4E5B9) % 2**62
    assert od.module_seed(0, 1) != od.module_seed(0, 2)


# ---------------------------------------------------------------------------------------------
# statistical quality
# ---------------------------------------------------------------------------------------------
def _corr_z(a, b, q):
    """z of the sample correlation of two keep arrays of n Bernoulli(q) pairs: sum of
    (a - q)(b - q) has variance n (q (1 - q))^2 when the two are independent."""
    a, b = a.ravel().astype(np.float64) - q, b.ravel().astype(np.float64) - q
    return float((a * b).sum() / (q * (1.0 - q) * np.sqrt(a.size)))


def _z_scores(seed, p):
    q = 1.0 - od.thresh_scale(p)[0] / 2.0**32  # the exact keep probability of a uniform hash
    K = [od.keep_mask(seed, l, E_Q, H_Q, p) for l in LAYERS]
    K2 = [od.keep_mask(od.forward_key(seed, 0), l, E_Q, H_Q, p) for l in LAYERS]
    n = E_Q * H_Q
    z = {}
    for l, k in zip(LAYERS, K):
        z[f"frac l{l}"] = float((k.mean() - q) / np.sqrt(q * (1.0 - q) / n))
        z[f"col lag1 l{l}"] = _corr_z(k[:, :-1], k[:, 1:], q)
        z[f"row lag1 l{l}"] = _corr_z(k[:-1], k[1:], q)
        z[f"col lag4 l{l}"] = _corr_z(k[:, :-4], k[:, 4:], q)
        z[f"key vs next key l{l}"] = _corr_z(k, K2[l], q)
    for i, j in itertools.combinations(range(len(LAYERS)), 2):
        z[f"layers {LAYERS[i]},{LAYERS[j]}"] = _corr_z(K[i], K[j], q)
    return z


def test_keep_fractions_and_correlations_at_the_noise_floor():
    worst = (0.0, None)
    for seed in SEEDS:
        for p in PS:
            for name, v in _z_scores(seed, p).items():
                if abs(v) > worst[0]:
                    worst = (abs(v), (seed, p, name))
    print(f"worst |z| {worst[0]:.2f} at seed, p, statistic = {worst[1]}")
    assert worst[0] <= Z_BAR, worst


ROW_SIGMA_MEASURED, COL_SIGMA_MEASURED = 4.00, 3.19


def test_per_row_and_per_column_keep_counts_at_p_half():
    # p = 0.5 only: at p = 0.02 a row's 64 draws are far from normal.  The model's own worst row
    # and column over the 5 seeds x 4 layers are 4.00 and 3.18 sigma (16 of a row's 64, 36 of a
    # column's 512 off the mean; 10,240 rows make ~3.9 sigma the expected worst); the bar is that
    # plus 1 sigma, there to catch a change of the model that makes rows or columns lopsided.
    worst_r = worst_c = 0.0
    for seed in SEEDS:
        for l in LAYERS:
            k = od.keep_mask(seed, l, E_Q, H_Q, 0.5)
            worst_r = max(worst_r, np.abs(k.sum(1) - H_Q / 2).max() / np.sqrt(H_Q / 4))
            worst_c = max(worst_c, np.abs(k.sum(0) - E_Q / 2).max() / np.sqrt(E_Q / 4))
    print(f"worst row {worst_r:.2f} sigma, worst column {worst_c:.2f} sigma")
    assert worst_r <= ROW_SIGMA_MEASURED + 1.0 and worst_c <= COL_SIGMA_MEASURED + 1.0


# ---------------------------------------------------------------------------------------------
# index above 2^32, thresh_scale edges
# ---------------------------------------------------------------------------------------------
def test_index_high_half_enters_the_hash():
    # E * H >= 2^32 needs a 16 GB h: this branch of drop_hash is covered by the model only
    for key, layer in ((0, 0), (2**40 + 3, 2), (od.module_seed(0, 1), 1)):
        for i in (0, 1, 63, 2**31 - 1, 2**32 - 2, 123456789):
            a, b, c = (int(od.drop_hash(key, layer, np.uint64(j))) for j in (i, i + 2**32, i + 1))
            assert a != b and a != c and b != c, (key, layer, i)
    # bijective in the low 32 index bits for a fixed key and high half
    idx = np.arange(1 << 16, dtype=np.uint64)
    for hi in (0, 5):
        assert np.unique(od.drop_hash(9, 1, idx + np.uint64(hi << 32))).size == idx.size


def test_thresh_scale_edges():
    one = np.float32(1.0)
    assert od.thresh_scale(0.0) == (0, one)
    assert od.thresh_scale(-0.25) == (0, one)
    t, s = od.thresh_scale(1e-12)
    assert t == 1 and s == one and s.dtype == np.float32  # floor(p 2^32) = 0 is clamped to 1
    assert od.thresh_scale(0.5) == (2**31, np.float32(2.0))
    p = np.float32(0.999999)
    t, s = od.thresh_scale(p)
    assert t == int(float(p) * 2.0**32) and 1 <= t < 2**32 - 1
    assert s == np.float32(1.0 / (1.0 - float(p))) and np.isfinite(s)
    assert od.thresh_scale(1.0) == (0xFFFFFFFF, np.float32(0.0))
    assert od.thresh_scale(1.5) == (0xFFFFFFFF, np.float32(0.0))
    # p is the float32 the C ABI carries: 0.1 and float32(0.1) give the same constants
    assert od.thresh_scale(0.1) == od.thresh_scale(np.float32(0.1))
    assert od.thresh_scale(0.1)[0] == int(float(np.float32(0.1)) * 2.0**32)
    # no dropout: every element kept
    assert od.keep_mask(3, 0, 5, 7, 0.0).all()


# ---------------------------------------------------------------------------------------------
# mutation power at the GPU cases' shapes
# ---------------------------------------------------------------------------------------------
def _idx(E, H, ld=None, group=False):
    c = np.arange(H, dtype=np.uint64)
    if group:
        c = c & ~np.uint64(3)
    return np.arange(E, dtype=np.uint64)[:, None] * np.uint64(H if ld is None else ld) + c[None, :]


def _mutants(key, l, E, H, p):
    t = np.uint32(od.thresh_scale(p)[0])
    Hp = (H + 3) // 4 * 4
    return {
        "a: layer ignored in the key": od.drop_hash(key, 0, _idx(E, H)) >= t,
        "b: index r * Hp + c": od.drop_hash(key, l, _idx(E, H, ld=Hp)) >= t,
        "c: one decision per float4": od.drop_hash(key, l, _idx(E, H, group=True)) >= t,
        "d: low 32 bits of the key": od.drop_hash(key & 0xFFFFFFFF, l, _idx(E, H)) >= t,
        "e: layer + 1": od.drop_hash(key, l + 1, _idx(E, H)) >= t,
    }


# the GPU case at whose shape each mutation can differ: (b) needs Hp != H, (d) a seed >= 2^32,
# (a) a layer above 0
@pytest.mark.parametrize("mut,case", [("a", "m1"), ("b", "m2"), ("c", "m1"), ("c", "m2"),
                                      ("d", "m1"), ("d", "m3"), ("e", "m1"), ("e", "m5"),
                                      ("a", "m5"), ("c", "m3"), ("e", "m4")])
def test_wrong_masks_differ_from_the_model_and_pass_the_old_rate_check(mut, case):
    kind, H, p, seed = MASK_CASES[case]
    E = mask_batch(kind).edge_index.shape[1]
    key = od.forward_key(seed)
    for l in range(MASK_D):
        if mut == "a" and l == 0:
            continue  # the mutation is the model at layer 0
        model = od.keep_mask(key, l, E, H, p)
        (name, wrong), = ((k, v) for k, v in _mutants(key, l, E, H, p).items() if k[0] == mut)
        differ = (wrong != model).mean()
        rate = 1.0 - wrong.mean()
        print(f"{case} layer {l} {name}: differs in {differ:.4f}, drop rate {rate:.4f}")
        assert differ >= 0.01, (name, case, l, differ)  # the bit-for-bit comparison sees it
        assert abs(rate - p) < 0.01, (name, case, l, rate)  # the drop-rate check did not


def test_mutations_that_cannot_differ_at_a_shape_do_not():
    # why (b) runs at m2 and (d) at m1 / m3: elsewhere the wrong mask is the right one
    kind, H, p, seed = MASK_CASES["m1"]
    mm = _mutants(seed, 1, 640, H, p)
    assert np.array_equal(mm["b: index r * Hp + c"], od.keep_mask(seed, 1, 640, H, p))
    kind, H, p, seed = MASK_CASES["m4"]
    assert seed < 2**32
    mm = _mutants(seed, 1, 640, H, p)
    assert np.array_equal(mm["d: low 32 bits of the key"], od.keep_mask(seed, 1, 640, H, p))
