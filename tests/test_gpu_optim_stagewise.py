"""GPU: the fused Adam / AMSGrad step (csrc/optim.hip), every stage of one step per element
against float64 (oracle/adam.py), as tests/test_gpu_stagewise.py judges the model's stages:
rho = |got - ref| / (u S) <= max(8, 4 rho_ref), rho_ref torch fp32 on the CPU for the same stage
from the same inputs.  Every intermediate of the update is an output of the kernel,
so the m and v stages are judged from the step's inputs and the p stage from the kernel's own
stored m' and v' / vmax'; max_exp_avg_sq and the step word are exact.
tests/test_optim_model.py shows on the CPU what these cases tell apart.

The C ABI is called with hand-built CgrAdamTensor tables, so every pointer is chosen here (two
tests go through FusedAdam, on the same kind of storage).  Each of the six arrays of a table
(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, step) lives in one flat buffer between two 64 KiB
guards of 0xA5 (tests/arena_contract_common.py) with a gap of 4 to 7 sentinel floats in front of,
between and behind the tensors.  After every step the guards, the gaps and the whole gradient
buffer are unchanged bit for bit, as are the param, state and step word of every entry the step
skips.

The norm of a clipped step is held to the relative bar derived from the kernels' summation
structure, oracle/adam.py NORM_BAR = 7u + 1e-12: 11 (float4 path) or 12 (scalar path) roundings
deep on non-negative terms -- the square, two adds or the four-fmaf chain, six butterfly levels,
two levels over the four wave sums -- so at most (1 + u)^12 - 1 on a block partial; the partials
are added in double; the square root halves it, 6u, and the rounding to float adds u.
"""

import ctypes

import numpy as np
import pytest
import torch

import optim_stagewise_common as oc
from arena_contract_common import Guarded
from stagewise_common import failures, write_report

from cgr_mpnn_3D._amd import native
from cgr_mpnn_3D._amd.optim import FusedAdam
from oracle import adam as oa

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e33)  # finite, no step's output
KEYS = ("p", "g", "m", "v", "vmax")
ADAM_GROUP = 32  # CGR_ADAM_GROUP (include/cgr_mpnn3d.h): tensors per launch
ALIGNED = dict.fromkeys(KEYS, 0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _layout(sizes, shift):
    """(first float of every tensor, floats in all): every tensor starts `shift` floats behind a
    16-byte boundary, 4 to 7 sentinel floats lie in front of, between and behind the tensors."""
    starts, off = [], 4
    for n in sizes:
        starts.append(off + shift)
        off = (off + shift + n + 3) // 4 * 4 + 4
    return starts, off


class Table:
    """A CgrAdamTensor table over guarded storage.

    sizes: the floats of every entry's storage; kinds: "live", "nograd" (a NULL gradient) or
    "empty" (numel 0) per entry; before: dict(p, g, m, v, vmax) of flat fp32 arrays over
    sum(sizes) elements; words: the step count per entry; shifts: floats by which each array's
    tensors are moved off their 16-byte boundary."""

    def __init__(self, dev, sizes, before, words, h, shifts=ALIGNED, kinds=None, null_vmax=False):
        self.dev, self.sizes, self.h = dev, list(sizes), h
        self.kinds = list(kinds) if kinds else ["live"] * len(sizes)
        self.before = {k: np.array(before[k], np.float32) for k in KEYS}
        if not h.amsgrad:  # never read, never written: NaN that would spoil anything it entered
            self.before["vmax"][:] = np.nan
        self.words = np.asarray(words, np.float32)
        self.G, self.starts, self.images = {}, {}, {}
        for k in KEYS:
            self.starts[k], total = _layout(self.sizes, shifts[k])
            img = np.full(total, np.nan if (k == "vmax" and not h.amsgrad) else SENTINEL,
                          np.float32)
            for s, n, a in zip(self.starts[k], self.sizes, oc.split(self.before[k], self.sizes)):
                img[s:s + n] = a
            self._upload(k, img)
        self.starts["step"] = [4 + 4 * i for i in range(len(self.sizes))]
        img = np.full(4 + 4 * len(self.sizes), SENTINEL, np.float32)
        img[self.starts["step"]] = self.words
        self._upload("step", img)
        self.live = np.repeat([kd == "live" for kd in self.kinds], self.sizes)
        self.t = oc.per_element(self.words, self.sizes)
        self.tab = (native.CgrAdamTensor * len(self.sizes))()
        for i, (n, kd) in enumerate(zip(self.sizes, self.kinds)):
            ptr = {k: self.G[k].payload.data_ptr() + 4 * self.starts[k][i] for k in self.G}
            assert all(ptr[k] % 16 == 4 * shifts[k] for k in KEYS)
            self.tab[i] = native.CgrAdamTensor(
                ptr["p"], None if kd == "nograd" else ptr["g"], ptr["m"], ptr["v"],
                None if null_vmax else ptr["vmax"], ptr["step"], 0 if kd == "empty" else n)

    def _upload(self, k, img):
        self.images[k] = img
        self.G[k] = Guarded(img.nbytes, img.view(np.uint8), self.dev)

    def __len__(self):
        return len(self.sizes)

    def view(self, k, i):
        """Entry i of array k as a torch view of the guarded storage (the step word 0-dim)."""
        flat = self.G[k].payload.view(torch.float32)
        s = self.starts[k][i]
        return flat[s] if k == "step" else flat[s:s + self.sizes[i]]

    def set_grad(self, g):
        """New gradients in place (the gaps keep their sentinel)."""
        self.before["g"] = np.array(g, np.float32)
        img = self.images["g"]
        for s, n, a in zip(self.starts["g"], self.sizes, oc.split(self.before["g"], self.sizes)):
            img[s:s + n] = a
        self.G["g"].fill = img.view(np.uint8).copy()
        self.G["g"].payload.copy_(torch.from_numpy(self.G["g"].fill).to(self.dev))

    def read(self, what=""):
        """dict(p, m, v, vmax: flat fp32 over every entry; words) as the storage stands.  Asserts
        every guard and gap intact and the gradient buffer unchanged, bit for bit."""
        torch.cuda.synchronize()
        out = {}
        for k, g in self.G.items():
            g.check_guards(f"{what} {k}")
            now = g.bytes().view(np.float32)
            if k == "step":
                data = np.zeros(now.size, bool)
                data[self.starts[k]] = True
                out["words"] = now[self.starts[k]].copy()
            else:
                data = np.zeros(now.size, bool)
                for s, n in zip(self.starts[k], self.sizes):
                    data[s:s + n] = True
                out[k] = now[data].copy()
            if k == "g":
                data[:] = False  # nothing of the gradient buffer may change
            bad = np.flatnonzero((_bits(now) != _bits(self.images[k])) & ~data)
            assert bad.size == 0, (f"{what}: {bad.size} floats of the {k} buffer outside the "
                                   f"tensors changed, first at float {int(bad[0])}")
        del out["g"]
        return out

    def advance(self, after):
        """The step's outputs become the next step's inputs."""
        for k in ("p", "m", "v", "vmax"):
            self.before[k] = after[k]
        self.words = after["words"]
        self.t = oc.per_element(self.words, self.sizes)


class Clip:
    """The device words of a clipped step; the partials hold exactly `capacity` floats between
    guards, from NaN."""

    def __init__(self, dev, capacity):
        self.capacity = capacity
        self.partials = Guarded(4 * capacity, "ones", dev)
        self.norm = torch.full((), float("nan"), dtype=torch.float32, device=dev)
        self.gate = torch.full((1,), 7, dtype=torch.int32, device=dev)
        self.skipped = torch.zeros((), dtype=torch.int64, device=dev)

    def struct(self, num_partials, max_norm):
        return native.CgrAdamClip(self.partials.payload.data_ptr(), num_partials,
                                  self.norm.data_ptr(), self.gate.data_ptr(),
                                  self.skipped.data_ptr(), float(max_norm))


def _args(h):
    return (float(h.b1), float(h.b2), float(h.eps), float(h.wd), int(h.amsgrad), int(h.maximize))


def _lr_word(dev, lr):
    return torch.tensor([lr], dtype=torch.float32, device=dev)


def _step(T, lr=oc.LR, entry="host", max_norm=None, clip=None):
    """One step of table T through cgr_adam_step ("host"), cgr_adam_step_lr_ptr ("ptr") or
    cgr_grad_sumsq + cgr_adam_step_clip ("clip": the lr in a device word)
    -> (what T.read() returns, the Clip or None)."""
    lib, dev = native.load(), T.dev
    st = native.stream_ptr(dev)
    word = _lr_word(dev, lr)
    with native.device_guard(dev):
        if entry == "host":
            native.check(lib.cgr_adam_step(T.tab, len(T), lr, *_args(T.h), st))
        elif entry == "ptr":
            native.check(lib.cgr_adam_step_lr_ptr(T.tab, len(T), word.data_ptr(), *_args(T.h),
                                                  st))
        else:
            need = int(lib.cgr_grad_sumsq_partials(T.tab, len(T)))
            assert need == sum(-(-n // oa.BLOCK) for n, kd in zip(T.sizes, T.kinds)
                               if kd == "live")
            clip = clip or Clip(dev, need)
            assert clip.capacity == need
            native.check(lib.cgr_grad_sumsq(T.tab, len(T), clip.partials.payload.data_ptr(), need,
                                            st))
            c = clip.struct(need, max_norm)
            native.check(lib.cgr_adam_step_clip(T.tab, len(T), 0.0, word.data_ptr(), *_args(T.h),
                                                ctypes.byref(c), st))
    after = T.read(entry)
    if clip is not None:
        clip.partials.check_guards("partials")
    return after, clip


def _same_bits(a, b, keys=("p", "m", "v", "vmax", "words"), where=None, what=""):
    for k in keys:
        x, y = _bits(a[k]), _bits(b[k])
        if where is not None and k != "words":
            x, y = x[where], y[where]
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} elements, first at {int(bad[0])}"


def _judge(case, T, after, lr=oc.LR, norm=None, max_norm=None, grads=None):
    """Every stage of T's live entries inside its bar, the skipped entries untouched, the step
    words advanced by exactly one; the rows go to stage_errors.json."""
    live = T.live
    sel = lambda d: {k: a[live] for k, a in d.items() if k != "words"}  # noqa: E731
    rows, exact = oa.judge(sel(T.before), sel(after), T.t[live], T.h, lr, norm=norm,
                           max_norm=max_norm)
    if norm is not None:
        rows.append(oa.norm_row(norm, grads))
    for r in rows:
        print(f"{case} {r['stage']}: rho {r['rho']:.3f} rho_ref {r['rho_ref']:.3f} "
              f"bar {r['bar']:.2f} at {r['argmax']}")
    write_report(case, rows)
    assert not exact, (case, exact)
    assert not failures(rows), (case, failures(rows))
    entry_live = np.array([kd == "live" for kd in T.kinds])
    assert (after["words"] == T.words + entry_live).all(), (case, after["words"], T.words)
    if not live.all():
        before = dict(T.before, words=T.words)
        _same_bits(before, after, keys=("p", "m", "v", "vmax"), where=~live,
                   what=f"{case}: a skipped entry")
    return rows


def _live_grads(T):
    return [g for g, kd in zip(oc.split(T.before["g"], T.sizes), T.kinds) if kd == "live"]


def _table(dev, c, **kw):
    return Table(dev, c["sizes"], c["before"], c["words"], c["h"], **kw)


# -------------------------------------------------------------------------------------------------
# hyper-parameters, step words, layouts
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.HYPER_CASES))
def test_hyper_parameter_cases(name, cuda_device):
    c = oc.hyper_case(name)
    # one case hands the kernel a NULL max_exp_avg_sq: without amsgrad it is never dereferenced
    T = _table(cuda_device, c, null_vmax=(name == "plain_wd_eps1e-3_t9"))
    after, _ = _step(T, entry="host")
    _judge(name, T, after)
    if c["h"].amsgrad and T.before["v"].any():  # both branches of the maximum are taken
        assert (T.before["vmax"] > after["v"]).any() and (T.before["vmax"] < after["v"]).any()
    if not c["h"].amsgrad:
        assert np.isnan(after["vmax"]).all()


def test_mixed_step_words_in_one_launch(cuda_device):
    c = oc.mixed_case()
    assert len(c["sizes"]) <= ADAM_GROUP and len(set(c["words"])) == len(oc.MIXED_STEPS)
    T = _table(cuda_device, c)
    after, _ = _step(T, entry="host")
    _judge(c["name"], T, after)  # every tensor by its own t


LAYOUTS = [("aligned", ALIGNED)] + [(f"{k}_moved", dict(ALIGNED, **{k: 1})) for k in KEYS] \
    + [("all_moved", dict.fromkeys(KEYS, 1))]


@pytest.mark.parametrize("name", ["ams_wd_t1", "plain_wd_eps1e-3_t1", "ams_max_wd_t0"])
def test_layouts_give_the_same_bits(name, cuda_device):
    """k_adam takes its float4 path only when every pointer it reads is 16-byte aligned, and the
    scalar path otherwise and for the last numel % 4 elements; both call the same adam_elem."""
    c = oc.hyper_case(name)
    first = None
    for lname, shifts in LAYOUTS:
        T = _table(cuda_device, c, shifts=shifts)
        after, _ = _step(T, entry="host")
        _judge(f"{name}/{lname}", T, after)
        if first is None:
            first = after
        _same_bits(first, after, what=f"{name}: aligned vs {lname}")


def test_clipped_layouts_stay_inside_the_bars(cuda_device):
    c = oc.clip_case("clip_ams_wd")
    for lname, shifts in (LAYOUTS[0], LAYOUTS[2], LAYOUTS[-1]):  # aligned, g moved, all moved
        T = _table(cuda_device, c, shifts=shifts)
        after, clip = _step(T, entry="clip", max_norm=c["max_norm"])
        _judge(f"clip_ams_wd/{lname}", T, after, norm=float(clip.norm), max_norm=c["max_norm"],
               grads=_live_grads(T))


# -------------------------------------------------------------------------------------------------
# table shapes: one, two and three launches, skipped entries in between
# -------------------------------------------------------------------------------------------------
def _shaped(n_live):
    """(sizes, kinds): the live sizes with a NULL-gradient entry behind every third live one and
    a numel-0 entry (5 floats of storage) behind every fifth."""
    sizes, kinds = [], []
    for i, n in enumerate(oc.table_sizes(n_live)):
        sizes.append(n)
        kinds.append("live")
        if i % 3 == 2:
            sizes.append(6)
            kinds.append("nograd")
        if i % 5 == 4:
            sizes.append(5)
            kinds.append("empty")
    return sizes, kinds


@pytest.mark.parametrize("n_live", [1, 31, 32, 33, 65])
def test_table_shapes(n_live, cuda_device):
    sizes, kinds = _shaped(n_live)
    assert kinds.count("live") == n_live and sum(sizes) < 20000
    h = oc.SETTINGS["ams_wd"]
    before = oc.make_inputs(f"shape{n_live}", sizes)
    words = [float(oc.MIXED_STEPS[i % 4]) for i in range(len(sizes))]
    lib = native.load()
    T = Table(cuda_device, sizes, before, words, h, kinds=kinds)
    want = sum(-(-n // oa.BLOCK) for n, kd in zip(sizes, kinds) if kd == "live")
    assert lib.cgr_grad_sumsq_partials(T.tab, len(T)) == want
    after, _ = _step(T, entry="host")
    _judge(f"shape{n_live}", T, after)
    # and clipped: the partials of the second and third launch land behind the first's
    T = Table(cuda_device, sizes, before, words, h, kinds=kinds)
    max_norm = oc.CLIP_FRACTION * oa.norm64(_live_grads(T))
    after, clip = _step(T, entry="clip", max_norm=max_norm)
    assert int(clip.skipped) == 0 and int(clip.gate) == 0
    _judge(f"shape{n_live}/clip", T, after, norm=float(clip.norm), max_norm=max_norm,
           grads=_live_grads(T))


# -------------------------------------------------------------------------------------------------
# the three entries read the same lr
# -------------------------------------------------------------------------------------------------
def test_lr_paths_give_the_same_bits(cuda_device):
    c = oc.hyper_case("ams_wd_t1")
    assert float(np.float32(oc.LR)) == oc.LR
    outs = []
    for entry in ("host", "ptr", "clip"):
        T = _table(cuda_device, c)
        # a bound above the norm: coef is exactly 1 and g * 1 = g
        after, clip = _step(T, entry=entry, max_norm=1e30)
        if clip is not None:
            assert int(clip.gate) == 0 and float(clip.norm) < 1e30
        outs.append(after)
    _judge("lr_paths", T, outs[0])
    _same_bits(outs[0], outs[1], what="cgr_adam_step vs cgr_adam_step_lr_ptr")
    _same_bits(outs[0], outs[2], what="cgr_adam_step vs cgr_adam_step_clip, bound above the norm")


# -------------------------------------------------------------------------------------------------
# clipping and the norm
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.CLIP_CASES))
def test_clipped_step(name, cuda_device):
    c = oc.clip_case(name)
    T = _table(cuda_device, c)
    after, clip = _step(T, entry="clip", max_norm=c["max_norm"])
    norm = float(clip.norm)
    assert oa.clip_coef(norm, c["max_norm"]) < 0.31
    assert int(clip.skipped) == 0 and int(clip.gate) == 0
    _judge(name, T, after, norm=norm, max_norm=c["max_norm"], grads=_live_grads(T))


@pytest.mark.parametrize("name", list(oc.NORM_CASES))
def test_norm_inside_its_derived_bar(name, cuda_device):
    sizes, grads, vec4 = oc.norm_case(name)
    before = oc.make_inputs(name, sizes)
    before["g"] = np.concatenate(grads)
    T = Table(cuda_device, sizes, before, [1.0] * len(sizes), oc.SETTINGS["ams"],
              shifts=dict(ALIGNED, g=0 if vec4[0] else 1))
    after, clip = _step(T, entry="clip", max_norm=float("inf"))  # measures, never clips
    norm = float(clip.norm)
    rep, _ = oa.norm_replica(grads, vec4)
    print(f"{name}: norm {norm!r}, host replica {float(rep)!r}, fp64 {oa.norm64(grads)!r}")
    _judge(name, T, after, norm=norm, max_norm=float("inf"), grads=grads)


def test_norm_exact_cases(cuda_device):
    h = oc.SETTINGS["ams"]
    f = np.float32
    # all-zero gradients: norm 0, coef 1, the step proceeds -- the bits of the unclipped step
    sizes = [5, 1025]
    before = oc.make_inputs("zero_grads", sizes)
    before["g"][:] = 0.0
    T = Table(cuda_device, sizes, before, [3.0, 3.0], h)
    after, clip = _step(T, entry="clip", max_norm=1.0)
    assert float(clip.norm) == 0.0 and int(clip.gate) == 0 and int(clip.skipped) == 0
    _judge("zero_grads", T, after, norm=0.0, max_norm=1.0, grads=_live_grads(T))
    U = Table(cuda_device, sizes, before, [3.0, 3.0], h)
    plain, _ = _step(U, entry="host")
    _same_bits(plain, after, what="zero gradients: clipped vs unclipped step")
    for g, want in [([3.0], 3.0), ([3.0, 4.0], 5.0)]:
        for shift in (0, 1):
            before = oc.make_inputs("exact", [len(g)])
            before["g"] = np.array(g, f)
            T = Table(cuda_device, [len(g)], before, [0.0], h, shifts=dict(ALIGNED, g=shift))
            _, clip = _step(T, entry="clip", max_norm=float("inf"))
            assert float(clip.norm) == want, (g, shift, float(clip.norm))
    # two one-element tensors: two partials, added in double
    before = oc.make_inputs("exact2", [1, 1])
    before["g"] = np.array([3.0, 4.0], f)
    T = Table(cuda_device, [1, 1], before, [0.0, 0.0], h)
    _, clip = _step(T, entry="clip", max_norm=float("inf"))
    assert float(clip.norm) == 5.0


# -------------------------------------------------------------------------------------------------
# skipped steps across launches and groups
# -------------------------------------------------------------------------------------------------
BAD = {"inf": float("inf"), "1e20": 1e20}  # 1e20 is finite; its square is not, in fp32


@pytest.mark.parametrize("bad", list(BAD))
def test_skipped_step_spans_every_launch(bad, cuda_device):
    """One bad gradient in a tensor of the third launch: the first launch finalises the norm and
    sets the gate, the second and third (C.partials == nullptr) only read it."""
    sizes = oc.table_sizes(65)
    h = oc.SETTINGS["ams_wd"]
    before = oc.make_inputs(f"skip_{bad}", sizes)
    good = before["g"].copy()
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert 64 // ADAM_GROUP == 2
    before["g"][offs[64]] = BAD[bad]
    T = Table(cuda_device, sizes, before, [2.0] * 65, h)
    max_norm = oc.CLIP_FRACTION * oa.norm64(oc.split(good, sizes))
    after, clip = _step(T, entry="clip", max_norm=max_norm)
    assert int(clip.skipped) == 1 and int(clip.gate) == 1
    assert np.isinf(float(clip.norm))
    _same_bits(dict(T.before, words=T.words), after, what=f"a skipped step ({bad})")
    # the next, finite step on the same storage and the same clip words
    T.set_grad(good)
    after, clip = _step(T, entry="clip", max_norm=max_norm, clip=clip)
    assert int(clip.skipped) == 1 and int(clip.gate) == 0
    _judge(f"after_skip_{bad}", T, after, norm=float(clip.norm), max_norm=max_norm,
           grads=_live_grads(T))


def _class_setup(dev, T, groups, **kw):
    """FusedAdam over torch views of T's guarded storage (params, gradients and pre-set state),
    `groups` lists of entry indices -> (optimizer, [params])."""
    ps = []
    for i in range(len(T)):
        p = T.view("p", i).requires_grad_()
        p.grad = T.view("g", i)
        ps.append(p)
    opt = FusedAdam([dict(params=[ps[i] for i in idx]) for idx in groups], lr=oc.LR,
                    betas=(T.h.b1, T.h.b2), eps=T.h.eps, weight_decay=T.h.wd,
                    amsgrad=T.h.amsgrad, maximize=T.h.maximize, **kw)
    for i, p in enumerate(ps):
        opt.state[p] = dict(step=T.view("step", i), exp_avg=T.view("m", i),
                            exp_avg_sq=T.view("v", i), max_exp_avg_sq=T.view("vmax", i))
    return opt, ps


def _assert_state_in_place(opt, ps, T):
    for i, p in enumerate(ps):  # the class kept the guarded storage (no copy was made)
        st = opt.state[p]
        for k, key in (("m", "exp_avg"), ("v", "exp_avg_sq"), ("vmax", "max_exp_avg_sq"),
                       ("step", "step")):
            assert st[key].data_ptr() == T.view(k, i).data_ptr()


@pytest.mark.parametrize("bad", list(BAD))
def test_skipped_step_spans_both_param_groups(bad, cuda_device):
    sizes = oc.table_sizes(16)
    h = oc.SETTINGS["ams_wd"]
    before = oc.make_inputs(f"groups_{bad}", sizes)
    good = before["g"].copy()
    offs = np.concatenate([[0], np.cumsum(sizes)])
    before["g"][offs[12] + 7] = BAD[bad]  # a tensor of the second group
    T = Table(cuda_device, sizes, before, [4.0] * 16, h)
    max_norm = oc.CLIP_FRACTION * oa.norm64([good])
    opt, ps = _class_setup(cuda_device, T, [list(range(9)), list(range(9, 16))],
                           max_grad_norm=max_norm)
    opt.step()
    _assert_state_in_place(opt, ps, T)
    after = T.read("skipped")
    assert int(opt.skipped_steps) == 1 and np.isinf(float(opt.grad_norm))
    _same_bits(dict(T.before, words=T.words), after, what=f"a skipped step ({bad})")
    T.set_grad(good)
    opt.step()
    after = T.read("after the skip")
    assert int(opt.skipped_steps) == 1
    _judge(f"groups_after_skip_{bad}", T, after, norm=float(opt.grad_norm), max_norm=max_norm,
           grads=[good])


# -------------------------------------------------------------------------------------------------
# a trajectory through the class
# -------------------------------------------------------------------------------------------------
def _trajectory(dev, judge):
    sizes = oc.table_sizes(16)
    h = oc.SETTINGS["ams_wd"]
    before = oc.make_inputs("trajectory", sizes, zero_state=True)
    grads = [before["g"]] + [oc.make_inputs(f"trajectory{it}", sizes)["g"] for it in range(1, 5)]
    norms = [oa.norm64([g]) for g in grads]
    max_norm = float(np.median(norms))  # some steps are clipped, some are not
    T = Table(dev, sizes, before, [0.0] * 16, h)
    opt, ps = _class_setup(dev, T, [list(range(16))], max_grad_norm=max_norm)
    outs, clipped = [], 0
    for it, g in enumerate(grads):
        if it:
            T.set_grad(g)
        opt.step()
        after = T.read(f"step {it + 1}")
        norm = float(opt.grad_norm)
        clipped += oa.clip_coef(norm, max_norm) < 1.0
        if judge:
            _judge(f"trajectory/step{it + 1}", T, after, norm=norm, max_norm=max_norm, grads=[g])
        assert (after["words"] == it + 1).all()
        T.advance(after)
        outs.append(dict(after, norm=np.float32(norm)))
    assert 0 < clipped < 5 and int(opt.skipped_steps) == 0
    _assert_state_in_place(opt, ps, T)
    return outs


def test_trajectory_of_five_steps_through_the_class(cuda_device):
    a = _trajectory(cuda_device, judge=True)
    b = _trajectory(cuda_device, judge=False)  # fresh objects, the same bits
    for it, (x, y) in enumerate(zip(a, b)):
        _same_bits(x, y, what=f"two runs, step {it + 1}")
        assert _bits(x["norm"]) == _bits(y["norm"])
