"""Host model of the train-mode dropout mask: the integer hash of csrc/common.hpp, the threshold
and scale of csrc/gnn_fwd.hip's dropout_consts, the key derivation of csrc/graph_prep.hip's
k_prep_count (and its twin in prep_one.hpp) and the module's key base (GNN._cgr_dropout_seed), in
numpy uint32 / uint64 arithmetic.  Written from those definitions, never from GPU output: the mask
is a pure integer function, so tests/test_gpu_dropout_mask.py compares it with tolerance zero.

    keep[r, c] of layer l  =  drop_hash(key, l, r * H + c) >= thresh(p_l)

r the edge row in dst-sorted order, c the logical column (H, not the padded row length), l the
0-based conv layer whose output is h_{l+1}.
"""

import numpy as np

_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF
KEY_STEP = 0xD1B54A32D192ED03  # Weyl step of the device counter (k_prep_count)


def mix32(x):
    """Wellons' lowbias32 finaliser over uint32 (arrays or scalars), arithmetic mod 2^32."""
    x = np.asarray(x, np.uint64) & np.uint64(_M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(_M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(_M32)
    x = x ^ (x >> np.uint64(16))
    return x.astype(np.uint32)


def layer_key(key, layer):
    """The 32-bit per-(key, layer) constant of drop_hash."""
    key = int(key) & _M64
    hi = ((key >> 32) + (int(layer) & _M32) * 0x9E3779B9) & _M32
    return int(mix32((key & _M32) ^ int(mix32(hi))))


def drop_hash(key, layer, idx):
    """uint32 hash of element index idx (uint64, array or scalar) under the 64-bit key."""
    idx = np.asarray(idx, np.uint64)
    lo, hi = idx & np.uint64(_M32), idx >> np.uint64(32)
    x = (lo * np.uint64(0x9E3779B1) + np.uint64(layer_key(key, layer))) & np.uint64(_M32)
    x = x ^ ((hi * np.uint64(0x85EBCA77)) & np.uint64(_M32))
    return mix32(x)


def thresh_scale(p):
    """(thresh, scale) of one layer: keep iff hash >= thresh, kept values times scale (float32).
    thresh 0 means no dropout.  p is the float32 the C ABI takes, widened to double."""
    p = float(np.float32(p))
    if p <= 0.0:
        return 0, np.float32(1.0)
    if p >= 1.0:
        return _M32, np.float32(0.0)
    t = min(p * 4294967296.0, 4294967295.0)
    return max(int(t), 1), np.float32(1.0 / (1.0 - p))


def forward_key(seed, counter=None):
    """The key one forward writes to the arena: seed when there is no device counter, else
    seed + KEY_STEP * (counter + 1) mod 2^64 (the forward then leaves counter + 1 behind)."""
    seed = int(seed) & _M64
    if counter is None:
        return seed
    return (seed + KEY_STEP * ((int(counter) + 1) & _M64)) & _M64


def module_seed(generator_seed, instance):
    """GNN._cgr_dropout_seed: the device generator's seed mixed with the model's construction
    index."""
    return (int(generator_seed) * 0x9E3779B97F4A7C15 + int(instance) * 0xBF58476D1CE4E5B9) % 2**62


def keep_mask(key, layer, E, H, p):
    """bool [E, H], rows in dst-sorted edge order: True where layer `layer` keeps the element."""
    thresh, _ = thresh_scale(p)
    if thresh == 0:
        return np.ones((E, H), bool)
    idx = (np.arange(E, dtype=np.uint64)[:, None] * np.uint64(H)
           + np.arange(H, dtype=np.uint64)[None, :])
    return drop_hash(key, layer, idx) >= np.uint32(thresh)
