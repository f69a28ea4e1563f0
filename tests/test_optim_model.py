"""CPU: what the fused Adam step's stage tests (tests/test_gpu_optim_stagewise.py) can tell
apart -- the counterpart of tests/test_stagewise_refs.py and tests/test_dropout_model.py.

* the float64 stages of oracle/adam.py, chained, are torch.optim.Adam (float64, foreach=False);
* at every GPU case's inputs the torch fp32 stand-in and a numpy fp32 replica of the kernel's
  adam_elem sit inside every stage's bar;
* every named variant of the update, applied to that replica, is over the bar of exactly the
  stages it belongs to, in exactly the cases where it differs from the update (VISIBLE below);
* the comparison the older optimizer tests make (six steps of randn (1 + it) gradients from a
  zero state, rtol 1e-5 / atol 1e-6) sees the denominator's eps only in an element whose first
  gradient happens to be below 3e-5;
* the host replica of the norm kernels sits inside the derived norm bar, and a dropped partial
  or a tail element counted twice does not.
"""

import numpy as np
import pytest
import torch

import optim_stagewise_common as oc
from oracle import adam as oa
from stagewise_common import failures

BETAS = [(0.9, 0.999), (0.8, 0.95), (0.0, 0.5)]


# -------------------------------------------------------------------------------------------------
# the model is torch's Adam
# -------------------------------------------------------------------------------------------------
def _close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max(),
                               err_msg=what)


def _torch_adam(p, state, h, lr):
    q = torch.from_numpy(p.copy()).requires_grad_()
    opt = torch.optim.Adam([q], lr=lr, betas=(h.b1, h.b2), eps=h.eps, weight_decay=h.wd,
                           amsgrad=h.amsgrad, maximize=h.maximize, foreach=False)
    if state is not None:
        opt.state[q] = dict(step=torch.tensor(float(state["t"])),
                            exp_avg=torch.from_numpy(state["m"].copy()),
                            exp_avg_sq=torch.from_numpy(state["v"].copy()))
        if h.amsgrad:
            opt.state[q]["max_exp_avg_sq"] = torch.from_numpy(state["vmax"].copy())
    return q, opt


def _compare(q, opt, mine, t, h, what):
    st = opt.state[q]
    _close(mine["p"], q.detach().numpy(), f"{what}: param")
    _close(mine["m"], st["exp_avg"].numpy(), f"{what}: exp_avg")
    _close(mine["v"], st["exp_avg_sq"].numpy(), f"{what}: exp_avg_sq")
    if h.amsgrad:
        _close(mine["vmax"], st["max_exp_avg_sq"].numpy(), f"{what}: max_exp_avg_sq")
    assert float(st["step"]) == t


@pytest.mark.parametrize("betas", BETAS)
@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("amsgrad", [True, False])
def test_chained_stages_are_torch_adam_in_float64(amsgrad, wd, maximize, betas):
    h = oa.Hyper(b1=betas[0], b2=betas[1], wd=wd, amsgrad=amsgrad, maximize=maximize)
    r = np.random.default_rng(5)
    n, lr = 257, 3e-3
    p0 = r.standard_normal(n)
    grads = [r.standard_normal(n) * (1 + it % 3) for it in range(5)]
    # five steps from a zero state (the constants stay doubles: cast=False)
    q, opt = _torch_adam(p0, None, h, lr)
    mine = dict(p=p0, m=np.zeros(n), v=np.zeros(n), vmax=np.zeros(n))
    for it, g in enumerate(grads):
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        mine = oa.step64(mine["p"], g, mine["m"], mine["v"], mine["vmax"], it, h, lr, cast=False)
        _compare(q, opt, mine, it + 1, h, f"step {it + 1}")
    # one step from a loaded state with vmax above and below v'
    v = r.standard_normal(n) ** 2
    state = dict(t=7, m=r.standard_normal(n), v=v, vmax=v * 10.0 ** r.uniform(-0.5, 0.5, n))
    q, opt = _torch_adam(p0, state, h, lr)
    q.grad = torch.from_numpy(grads[0].copy())
    opt.step()
    mine = oa.step64(p0, grads[0], state["m"], state["v"], state["vmax"], 7, h, lr, cast=False)
    if amsgrad:
        above = state["vmax"] > mine["v"]
        assert above.any() and not above.all()
    _compare(q, opt, mine, 8, h, "loaded state")


@pytest.mark.parametrize("maximize,wd", [(False, 0.0), (True, 1e-2)])
def test_clipped_composition_is_clip_grad_norm_then_step(maximize, wd):
    h = oa.Hyper(wd=wd, maximize=maximize)
    r = np.random.default_rng(6)
    sizes, lr = [130, 1, 77], 1e-2
    ps = [r.standard_normal(n) for n in sizes]
    gs = [r.standard_normal(n) * 3.0 for n in sizes]
    norm = oa.norm64(gs)
    for frac in (0.3, 2.0):  # clipped; a bound above the norm: coef = 1
        max_norm = float(np.float32(frac * norm))  # a float: clip_coef's cast changes nothing
        qs = [torch.from_numpy(p.copy()).requires_grad_() for p in ps]
        opt = torch.optim.Adam(qs, lr=lr, weight_decay=wd, amsgrad=True, maximize=maximize,
                               foreach=False)
        for q_, g in zip(qs, gs):
            q_.grad = torch.from_numpy(g.copy())
        total = torch.nn.utils.clip_grad_norm_(qs, max_norm, norm_type=2.0)
        assert abs(float(total) - norm) <= 1e-12 * norm
        opt.step()
        coef = oa.clip_coef(norm, max_norm)
        assert (coef < 1.0) == (frac < 1.0)
        for q_, p, g in zip(qs, ps, gs):
            z = np.zeros_like(p)
            mine = oa.step64(p, g, z, z, z, 0, h, lr, coef=coef, cast=False)
            _compare(q_, opt, mine, 1, h, f"max_norm {frac} x norm")


# -------------------------------------------------------------------------------------------------
# the stand-in and the replica pass, every variant fails, at the GPU cases' inputs
# -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    """Every GPU case with the norm and coefficient the replica of the norm kernels gives it."""
    out = []
    for c in oc.all_cases():
        c = dict(c, norm=None, coef32=None)
        if c["max_norm"] is not None:
            grads = oc.split(c["before"]["g"], c["sizes"])
            c["norm"], _ = oa.norm_replica(grads, [True] * len(grads))
            c["coef32"] = oa.replica_coef(c["norm"], c["max_norm"])
            assert c["coef32"] < 1.0
        out.append(c)
    return out


def _replica(c, variant=None):
    b = c["before"]
    return oa.replica_step(b["p"], b["g"], b["m"], b["v"], b["vmax"], c["t"], c["h"], c["lr"],
                           coef=c["coef32"], variant=variant)


def _judge(c, after):
    return oa.judge(c["before"], after, c["t"], c["h"], c["lr"], norm=c["norm"],
                    max_norm=c["max_norm"])


def test_case_list_holds_what_the_variants_need(cases):
    ts = {int(w) for c in cases for w in c["words"]}
    assert {0, 1, 9, 999, 99999} <= ts
    assert len({tuple(c["words"]) for c in cases if len(set(c["words"])) > 1}) == 1  # mixed
    for c in cases:
        assert sum(c["sizes"]) < 20000
        b = c["before"]
        assert (b["g"][::17] == 0).all() and (b["m"][::23] == 0).all()
        if c["h"].amsgrad and b["v"].any():  # a state with vmax above and below v'
            v1 = _replica(c)["v"]
            assert (b["vmax"] > v1).any() and (b["vmax"] < v1).any(), c["name"]


def test_replica_and_standin_sit_inside_every_bar(cases):
    worst = {}
    for c in cases:
        b, h = c["before"], c["h"]
        rep = _replica(c)
        rows, exact = _judge(c, rep)
        assert not exact and not failures(rows), (c["name"], exact, failures(rows))
        for r in rows:
            w = worst.setdefault(r["stage"], [0.0, 0.0])
            w[0], w[1] = max(w[0], r["rho"]), max(w[1], r["rho_ref"])
        # the stand-in as an implementation: each stage from the previous stage's stored result
        m1 = oa.standin_m(b["p"], b["g"], b["m"], h, c["coef32"])
        v1 = oa.standin_v(b["p"], b["g"], b["v"], h, c["coef32"])
        vm1 = np.maximum(b["vmax"], v1) if h.amsgrad else b["vmax"]
        p1 = oa.standin_p(b["p"], m1, v1, vm1, c["t"], h, c["lr"])
        rows, exact = _judge(c, dict(p=p1, m=m1, v=v1, vmax=vm1))
        assert not exact and not failures(rows), (c["name"], exact, failures(rows))
        for r in rows:
            assert r["rho"] == r["rho_ref"]
    # measured: the replica's rho max 3.34 (m), 6.07 (v, a clipped case), 4.08 (p)
    print({k: (round(a, 2), round(b_, 2)) for k, (a, b_) in worst.items()})


def _bc(h, t):
    return 1.0 - h.b1 ** t, 1.0 - h.b2 ** t


# where a variant differs from the update at all: the cases that can tell it apart
VISIBLE = {
    "eps_omitted": lambda c: True,
    "eps_in_sqrt": lambda c: True,
    # sqrt(bc2) == 1 in double from b2^(t+1) < 2^-53 on: invisible at t = 999 (b2 = 0.95) and at
    # t = 99,999
    "eps_before_bc2": lambda c: any(_bc(c["h"], w + 1)[1] != 1.0 for w in c["words"]),
    # from a zero state vmax' == v'
    "v_for_vmax": lambda c: c["h"].amsgrad and bool(c["before"]["vmax"].any()),
    "bc_at_t": lambda c: any(_bc(c["h"], w) != _bc(c["h"], w + 1) for w in c["words"]),
    "wd_before_maximize": lambda c: c["h"].maximize and c["h"].wd != 0,
    "clip_after_wd": lambda c: c["max_norm"] is not None and c["h"].wd != 0,
    "decoupled_decay": lambda c: c["h"].wd != 0,
    "shared_step": lambda c: len(set(c["words"])) > 1,
}


@pytest.mark.parametrize("variant", sorted(oa.VARIANTS))
def test_every_variant_is_over_the_bar_of_its_own_stages_only(variant, cases):
    own = set(oa.VARIANTS[variant])
    seen, where = set(), []
    for c in cases:
        rows, exact = _judge(c, _replica(c, variant))
        got = oa.flagged(rows)
        assert not exact, (c["name"], exact)
        assert got <= own, f"{variant} at {c['name']}: flagged {got}, its stages are {own}"
        if VISIBLE[variant](c):
            assert got, f"{variant} differs from the update at {c['name']} and no stage sees it"
            where.append(c["name"])
            worst = {r["stage"]: r["rho"] for r in rows if r["stage"][5:] in got}
            print(f"{variant} at {c['name']}: {worst}")
        else:
            assert not got, f"{variant} at {c['name']}: flagged {got} where it is the update"
        seen |= got
    assert seen == own, f"{variant}: only {seen} of {own} flagged in any case"
    names = {c["name"] for c in cases}
    if variant == "bc_at_t":  # the placement of the bias correction is invisible at large t
        assert "ams_wd_t99999" in names - set(where) and "ams_wd_t1" in where
    if variant == "v_for_vmax":  # and vmax from a zero state
        assert not any(n.endswith("_t0") for n in where) and "ams_t1" in where


# -------------------------------------------------------------------------------------------------
# the old bar, replayed
# -------------------------------------------------------------------------------------------------
OLD_SHAPES = [(400, 860), (400,), (400, 400), (1, 400), (1,), (7, 3), (1001,), ()]
P_VARIANTS = ("eps_omitted", "eps_in_sqrt", "eps_before_bc2", "v_for_vmax", "bc_at_t")


def test_old_six_step_comparison_hardly_sees_eps():
    """tests/test_gpu_optim.py's recipe (amsgrad, wd 0, lr 3e-3, six steps of randn (1 + it)
    from a zero state over its SHAPES) in float64, every variant of the parameter stage against
    the update at that test's rtol 1e-5 / atol 1e-6.  At wd = 0 the moments do not depend on the
    parameter, so they are computed once and only the parameter is carried per variant; the
    weight-decay variants are the update itself there.  The numbers are that test's own (CPU
    generators, seeds 0 and 1, its skipped gradient at step 3).  Measured, elements of 505,824
    over the tolerance: eps_omitted 2, eps_in_sqrt 664, eps_before_bc2 78, v_for_vmax 53,
    bc_at_t all.  Only the robust fact is asserted."""
    h, lr = oa.Hyper(), 3e-3
    c = oa.consts(h)
    n = sum(int(np.prod(s)) for s in OLD_SHAPES)
    # that test's own numbers: both of its generators are CPU generators
    gen = torch.Generator().manual_seed(0)
    p0 = np.concatenate([torch.randn(s, generator=gen).double().numpy().reshape(-1)
                         for s in OLD_SHAPES])
    gen = torch.Generator().manual_seed(1)
    p = {k: p0 for k in (None,) + P_VARIANTS}
    m = v = vmax = np.zeros(n)
    sizes = [int(np.prod(s)) for s in OLD_SHAPES]
    third = np.repeat(np.arange(len(sizes)) == 2, sizes)  # its gradient is None at step 3
    t = np.zeros(n)
    for it in range(6):
        g = np.concatenate([(torch.randn(s, generator=gen) * (1 + it)).double().numpy().reshape(-1)
                            for s in OLD_SHAPES])
        live = ~third if it == 3 else np.ones(n, bool)
        m1 = np.where(live, oa.m_stage(p[None], g, m, h, c).ref, m)
        v1 = np.where(live, oa.v_stage(p[None], g, v, h, c).ref, v)
        vmax1 = np.maximum(vmax, v1)
        for k in p:
            with np.errstate(all="ignore"):
                p[k] = np.where(live, oa.p_stage(p[k], m1, v1, vmax1, t, h, c, lr, variant=k).ref,
                                p[k])
        m, v, vmax, t = m1, v1, vmax1, t + live
        g0 = g if it == 0 else g0
    over = {}
    for k in P_VARIANTS:
        bad = ~(np.abs(p[k] - p[None]) <= 1e-6 + 1e-5 * np.abs(p[None]))
        over[k] = int(bad.sum())
        if k == "eps_omitted":
            seen_eps = np.abs(g0[bad])
    print(f"elements of {n} over rtol 1e-5 / atol 1e-6 after six steps: {over}; eps_omitted at "
          f"first gradients of {seen_eps}")
    assert (vmax == v).mean() > 0.9  # growing gradients: vmax is v almost everywhere
    # From a zero state the first update is lr g / (|g| + eps) against lr sign(g): apart by more
    # than atol only where |g| < lr eps / atol = 3e-5, 2.4e-5 of a normal draw; every later
    # denominator holds a gradient of order 1.  That comparison sees eps in such elements alone
    # (two of this draw's 505,824) and in none of the rest.
    assert (seen_eps < lr * h.eps / 1e-6).all()
    assert over["eps_omitted"] < 1e-4 * n


# -------------------------------------------------------------------------------------------------
# the norm
# -------------------------------------------------------------------------------------------------
def _rel(got, grads):
    ref = oa.norm64(grads)
    return abs(float(got) - ref) / ref


def test_norm_replica_inside_the_derived_bar_and_broken_sums_outside():
    assert 7.0 * oa.U < oa.NORM_BAR < 8.0 * oa.U
    caught = {"drop_last_partial": [], "double_tail": []}
    for name in oc.NORM_CASES:
        sizes, grads, vec4 = oc.norm_case(name)
        got, parts = oa.norm_replica(grads, vec4)
        assert parts.size == sum(-(-n // oa.BLOCK) for n in sizes)
        rel = _rel(got, grads)
        print(f"{name}: replica {float(got)!r} rel {rel:.2e} of bar {oa.NORM_BAR:.2e}")
        assert rel <= oa.NORM_BAR, (name, rel)
        row = oa.norm_row(got, grads)
        assert row["rho"] <= row["bar"]
        for variant in caught:
            bad, _ = oa.norm_replica(grads, vec4, variant)
            if _rel(bad, grads) > oa.NORM_BAR:
                caught[variant].append(name)
    print(caught)
    for variant, names in caught.items():
        assert "norm_unit_1027_odd" in names, (variant, names)


def test_norm_replica_exact_cases():
    f = np.float32
    for grads, want in [([np.zeros(5, f), np.zeros(1025, f)], 0.0), ([np.array([3.0], f)], 3.0),
                        ([np.array([3.0, 4.0], f)], 5.0),
                        ([np.array([3.0], f), np.array([4.0], f)], 5.0)]:
        for al in (True, False):
            got, _ = oa.norm_replica(grads, [al] * len(grads))
            assert float(got) == want
            assert oa.norm_row(got, grads)["rho"] == 0.0
    got, _ = oa.norm_replica([np.full(3, 1e20, f)], [True])  # the squares overflow in fp32
    assert np.isinf(got)
    assert oa.norm_row(got, [np.full(3, 1e20, f)])["rho"] == np.inf
