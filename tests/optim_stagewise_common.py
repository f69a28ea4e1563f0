"""Shared by tests/test_gpu_optim_stagewise.py (the kernels) and tests/test_optim_model.py (what
those cases can tell apart, on the CPU): the tensor sizes, the per-element inputs and the
hyper-parameter cases of the fused Adam step's stage tests (oracle/adam.py)."""

import zlib

import numpy as np

from oracle import adam as oa

# Every table holds these sizes: the block edge (1,024 elements), the float4 tail (numel % 4 of
# 0 .. 3 behind full float4 groups and on their own), one, two and three blocks, and tiny tensors
# right behind multi-block ones (k_adam's first_block search).  15,379 elements.
SIZES = (3 * 1024 + 1, 1, 2048, 2, 1025, 3, 2049, 4, 1024, 5, 2047, 7, 1020, 1021, 1023, 1027)
EXTRA = (1, 2, 3, 4, 5, 7)  # the tensors past the sixteenth of a longer table
LR = float(np.float32(3e-3))  # a float: the host double and the device word hold the same value


def table_sizes(n):
    """The sizes of a table of n live tensors (n = 1: the four-block tensor alone)."""
    return list(SIZES[:n]) + [EXTRA[i % len(EXTRA)] for i in range(max(0, n - len(SIZES)))]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def make_inputs(name, sizes, zero_state=False, g_decades=(-12.0, 2.0)):
    """dict(p, g, m, v, vmax) of flat fp32 arrays over sum(sizes) elements, seeded by the name:
    p = randn 10^U(-3, 1); g = randn 10^U(g_decades), every 17th exactly 0; m like g,
    v = (randn 10^U(-12, 2))^2, vmax = v 10^U(-0.5, 0.5), every 23rd element a parameter that
    never had a gradient (m = v = vmax = 0); zero_state: the state of a first step."""
    n = int(sum(sizes))
    r = _rng(name)
    f = np.float32

    def wide(lo, hi):
        return r.standard_normal(n) * 10.0 ** r.uniform(lo, hi, n)

    p = wide(-3.0, 1.0).astype(f)
    g = wide(*g_decades).astype(f)
    g[::17] = 0.0
    m = wide(-12.0, 2.0).astype(f)
    v = (wide(-12.0, 2.0) ** 2).astype(f)
    vmax = (v.astype(np.float64) * 10.0 ** r.uniform(-0.5, 0.5, n)).astype(f)
    for a in (m, v, vmax):
        a[::23] = 0.0
        if zero_state:
            a[:] = 0.0
    return dict(p=p, g=g, m=m, v=v, vmax=vmax)


def split(flat, sizes):
    """The per-tensor views of a flat array."""
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return [flat[a:b] for a, b in zip(offs[:-1], offs[1:])]


def per_element(words, sizes):
    """One value per tensor -> one per element."""
    return np.repeat(np.asarray(words, np.float64), sizes)


H = oa.Hyper
SETTINGS = {
    "ams": H(),
    "ams_wd": H(wd=1e-2),
    "plain_wd_eps1e-3": H(wd=1e-2, eps=1e-3, amsgrad=False),
    "ams_max_wd": H(wd=1e-2, maximize=True),
    "ams_b0_b05": H(b1=0.0, b2=0.5),
    "ams_b08_b095": H(b1=0.8, b2=0.95),
}
# name: (setting, t before the step)
HYPER_CASES = {f"{s}_t{t}": (s, t) for s in ("ams", "ams_wd", "plain_wd_eps1e-3", "ams_max_wd",
                                             "ams_b0_b05") for t in (0, 1, 9)}
HYPER_CASES["ams_b08_b095_t999"] = ("ams_b08_b095", 999)
HYPER_CASES["ams_wd_t99999"] = ("ams_wd", 99999)
MIXED_STEPS = (0, 1, 9, 999)  # the tensors of the mixed table, in turn
# clipped cases: (setting, t); max_norm = CLIP_FRACTION x the float64 norm
CLIP_CASES = {"clip_ams_wd": ("ams_wd", 1), "clip_ams_max_wd": ("ams_max_wd", 9)}
CLIP_FRACTION = 0.3


def hyper_case(name):
    """-> dict(name, sizes, before, words (t per tensor), t (per element), h, lr)."""
    s, t = HYPER_CASES[name]
    sizes = table_sizes(len(SIZES))
    return dict(name=name, sizes=sizes, before=make_inputs(name, sizes, zero_state=(t == 0)),
                words=[float(t)] * len(sizes), t=per_element([t] * len(sizes), sizes),
                h=SETTINGS[s], lr=LR, max_norm=None)


def mixed_case():
    sizes = table_sizes(len(SIZES))
    words = [float(MIXED_STEPS[i % len(MIXED_STEPS)]) for i in range(len(sizes))]
    return dict(name="mixed_steps", sizes=sizes, before=make_inputs("mixed_steps", sizes),
                words=words, t=per_element(words, sizes), h=SETTINGS["ams_wd"], lr=LR,
                max_norm=None)


def clip_case(name):
    s, t = CLIP_CASES[name]
    sizes = table_sizes(len(SIZES))
    before = make_inputs(name, sizes)
    return dict(name=name, sizes=sizes, before=before, words=[float(t)] * len(sizes),
                t=per_element([t] * len(sizes), sizes), h=SETTINGS[s], lr=LR,
                max_norm=CLIP_FRACTION * oa.norm64([before["g"]]))


def all_cases():
    """Every single-step case judged stage by stage, GPU and CPU alike."""
    return ([hyper_case(n) for n in HYPER_CASES] + [mixed_case()]
            + [clip_case(n) for n in CLIP_CASES])


# the norm's own cases: name: (live tensors, gradient moved by one float, unit scale)
NORM_CASES = {
    "norm_aligned": (16, False, False),
    "norm_odd": (16, True, False),
    "norm_65": (65, False, False),
    "norm_65_odd": (65, True, False),
    # one tensor of 1,027 unit-scale elements: its last partial (3 elements) and its tail element
    # weigh ~1e-3 of the sum, where a gradient of nine decades hides them behind its largest terms
    "norm_unit_1027_odd": (None, True, True),
}


def norm_case(name):
    """-> (sizes, [gradient per tensor], [vec4 per tensor]): g = randn 10^U(-6, 3) (every square
    a normal fp32 number), or plain randn."""
    n, odd, unit = NORM_CASES[name]
    sizes = [1027] if n is None else table_sizes(n)
    r = _rng(name)
    tot = int(sum(sizes))
    g = r.standard_normal(tot)
    if not unit:
        g = g * 10.0 ** r.uniform(-6.0, 3.0, tot)
    g = g.astype(np.float32)
    assert (g.astype(np.float64) ** 2 >= 2.0 ** -126).all()
    return sizes, split(g, sizes), [not odd] * len(sizes)
