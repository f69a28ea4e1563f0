"""CPU: the per-stage float64 references (oracle/stagewise.py) are the oracle, step by step; their
bars are attainable by an honest fp32 implementation and are missed by a subtly wrong one.

* chain consistency: the stage functions fed their own outputs reproduce oracle/dmpnn_numpy.py's
  predictions and every gradient to 1e-12;
* the reference passes its own bars: a stand-in kernel (numpy fp32; split-bf16 weight gradients
  as the two-piece emulation rounded to fp32) meets the bars tests/test_gpu_stagewise.py holds
  the HIP kernels to, at that file's shapes;
* the activation allowance tol_act holds for torch fp32 over |z| from 1e-30 to 250;
* sensitivity: four one-element kernel bugs each exceed their stage's bar -- and only that
  stage's -- while one of them passes the end-to-end bars of tests/test_gpu_parity.py;
* the same three for the standalone DMPNNConv's stages (conv_stages): torch float64 autograd of
  the reference conv to 1e-12, the fp32 stand-in at tests/test_gpu_conv_stagewise.py's shapes,
  and one-element bugs that exceed their own stage's bar only.
"""

import numpy as np
import pytest
import torch

from conftest import ACT_NAMES
from stagewise_common import (CONV_CASES, TORCH_F32, _ACT, conv_inputs, failures, mixed_dy,
                              random_params)
from test_gpu_parity import (_hub_batch, _shuffled_pairs, _sparse_batch, assert_g_close,
                             assert_y_close)

from cgr_mpnn_3D._amd.synth import make_batch
from oracle import dmpnn_numpy as on
from oracle import stagewise as sw


def _cfg(b, H, D, act, skip=True, aggr="add", pool="add"):
    return dict(F=b.x.shape[1], Fe=b.edge_attr.shape[1], H=H, D=D, act=act, skip=skip, aggr=aggr,
                pool=pool, batched=True)


def _setup(b, H, D, act, skip=True, aggr="add", pool="add", seed=0):
    cfg = _cfg(b, H, D, act, skip, aggr, pool)
    p = random_params(np.random.default_rng(seed), cfg["F"], cfg["Fe"], H, D)
    return cfg, p, mixed_dy(b.num_graphs)


def _chain(b, cfg, p, dy, **kw):
    return sw.run_chain(p, cfg, b.x, b.edge_index, b.edge_attr, b.batch, b.num_graphs, dy, **kw)


# ---------------------------------------------------------------------------------------------
# chain consistency
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,aggr,pool,drop", [("silu", "add", "add", False),
                                                ("relu", "mean", "mean", False),
                                                ("gelu", "add", "max", True)])
def test_stage_chain_reproduces_the_oracle(act, aggr, pool, drop):
    b = make_batch(6, 14, 16, n_mace=7, seed=3, n_atoms_jitter=4)
    H, D = 37, 3
    cfg, p, dy = _setup(b, H, D, act, True, aggr, pool)
    E = b.edge_index.shape[1]
    masks, ps, keep = None, None, None
    if drop:
        rng = np.random.default_rng(7)
        ps = [0.25, 0.0, 0.1]
        masks = [(rng.random((E, H)) >= q).astype(np.float64) for q in ps]
        keep = [m / (1.0 - q) if q > 0 else None for m, q in zip(masks, ps)]
    rec = _chain(b, cfg, p, dy, keep=keep, inputs=True)
    y, cache = on.forward(p, b.x, b.edge_index, b.edge_attr, b.batch, D, act, True, b.num_graphs,
                          dropout_masks=masks, dropout_ps=ps, aggr=aggr, pool=pool)
    gin = {}
    g = on.backward(p, cache, dy, gin)

    def close(got, ref, name):
        err = np.abs(np.asarray(got) - ref).max() / (np.abs(ref).max() + 1e-300)
        assert err <= 1e-12, (name, err)

    perm = rec["perm"]
    close(rec["y"], y, "y")
    for l in range(D + 1):
        close(rec["h"][l], cache["hs"][l][perm], f"h{l}")
    close(rec["a"][D], cache["s"], "a_D")
    close(rec["hn"], cache["hnode"], "hn")
    close(rec["g"], cache["g"], "g")
    assert set(rec["grads"]) == set(g)
    for k in g:
        close(rec["grads"][k], g[k], k)
    close(rec["dx"], gin["x"], "dx")
    close(rec["de"], gin["edge_attr"], "de")
    # and every stage of that record is its own reference: rho == 0 against itself
    for name, got, st, emu, _ in sw.stages(rec, p, cfg):
        assert sw.rho(got, st)[0] == 0.0, name


# ---------------------------------------------------------------------------------------------
# the reference passes its own bars (the shapes of tests/test_gpu_stagewise.py)
# ---------------------------------------------------------------------------------------------
def _case_batches():
    c1 = lambda: make_batch(12, n_atoms=30, n_bonds=34, n_mace=40, seed=101)  # noqa: E731
    cases = {
        "c01": (c1, 128, 3, "silu", True, {}, "b3"),
        "c02": (lambda: make_batch(6, 14, 16, n_mace=7, seed=102), 37, 2, "gelu", True, {}, "b3"),
        "c02_h39": (lambda: make_batch(6, 14, 16, n_mace=7, seed=102), 39, 2, "gelu", True, {},
                    "b3"),
        "c03": (lambda: make_batch(10, 24, 26, n_mace=2, seed=103), 96, 3, "relu", False, {},
                "b3"),
        "c05": (lambda: make_batch(8, n_atoms=20, n_bonds=22, n_mace=16, seed=105), 528, 2, "silu",
                False, {}, "f32"),
        "c06": (lambda: _hub_batch([150, 3, 70, 300, 5], seed=41), 64, 3, "relu", True, {}, "b3"),
        "c08": (lambda: _shuffled_pairs(make_batch(8, n_atoms=30, n_bonds=30, n_mace=16, seed=28),
                                        seed=5), 64, 3, "gelu", True, {}, "b3"),
        "c09_mean": (lambda: _sparse_batch(6, 40, seed=27), 64, 2, "silu", True,
                     dict(aggr="mean", pool="mean"), "b3"),
        "c09_max": (lambda: _sparse_batch(6, 40, seed=29), 64, 2, "silu", False,
                    dict(pool="max"), "b3"),
        "c11": (c1, 128, 3, "silu", True, dict(p_drop=0.02), "b3"),
        # H > 512: the fp32 TN kernels (both families are judged as fp32)
        "c12": (lambda: make_batch(7, 21, 23, n_mace=40, seed=112), 1000, 2, "silu", True, {},
                "f32"),
        "c13": (lambda: make_batch(7, 21, 23, n_mace=7, seed=113), 515, 2, "gelu", True, {},
                "f32"),
        "c14": (lambda: make_batch(7, 21, 23, n_mace=2, seed=114), 521, 3, "relu", False, {},
                "f32"),
        "c15": (lambda: _hub_batch([150, 3, 70, 300, 5], seed=43), 520, 2, "relu", True, {},
                "f32"),
        "c16": (lambda: _sparse_batch(6, 40, seed=31), 516, 2, "silu", True,
                dict(aggr="mean", pool="mean", p_drop=0.02), "f32"),
        "c17": (lambda: _shuffled_pairs(make_batch(6, 21, 23, n_mace=2, seed=115), seed=5), 560,
                2, "gelu", True, {}, "f32"),
    }
    for act in ACT_NAMES:
        cases["c10_" + act] = (c1, 128, 3, act, True, dict(scales=[1e-3, 1, 10, 100]), "b3")
    return cases


CASES = _case_batches()


@pytest.mark.parametrize("case", sorted(CASES))
def test_fp32_stand_in_meets_the_bars(case):
    mk, H, D, act, skip, opt, fam = CASES[case]
    b = mk()
    opt = dict(opt)
    scales, p_drop = opt.pop("scales", None), opt.pop("p_drop", 0.0)
    if scales is not None:
        import dataclasses
        s = np.asarray(scales, np.float32)[np.arange(b.x.shape[0]) % len(scales), None]
        b = dataclasses.replace(b, x=(b.x * s).astype(np.float32))
    cfg, p, dy = _setup(b, H, D, act, skip, **opt)
    keep = None
    if p_drop:
        rng = np.random.default_rng(11)
        keep = [(rng.random((b.edge_index.shape[1], H)) >= p_drop) / (1.0 - p_drop)
                for _ in range(D)]
    rec = _chain(b, cfg, p, dy, ops=sw.F32, keep=keep, tn_family=fam, inputs=True)
    rows = sw.judge(rec, p, cfg, TORCH_F32)
    assert len(rows) >= 20 and all(np.isfinite(r["rho_ref"]) for r in rows)
    bad = failures(rows)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------
# activations: tol_act covers torch fp32's forward and autograd derivative
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACT_NAMES)
def test_activation_allowance_covers_torch_fp32(act):
    mag = 10.0 ** np.linspace(-30.0, np.log10(250.0), 14000)
    pts = np.array([0.0, 20.0, 9.0, 17.0, 88.0, 104.0])
    pts = np.concatenate([pts, np.nextafter(np.float32(20.0), np.float32([0.0, 40.0]))])
    z32 = np.concatenate([mag, -mag, pts, -pts]).astype(np.float32)
    z = z32.astype(np.float64)
    t = torch.from_numpy(z32).clone().requires_grad_(True)
    y = _ACT[act](t)
    y.sum().backward()
    f64, d64 = on.act_fwd(z, act), on.act_grad(z, act)
    assert np.isfinite(f64).all() and np.isfinite(d64).all()
    tol = sw.tol_act(z)
    rf = np.abs(y.detach().numpy() - f64) / tol
    rd = np.abs(t.grad.numpy() - d64) / tol
    print(f"{act}: forward {rf.max():.3f} tol at z={z[rf.argmax()]:.6g}, derivative "
          f"{rd.max():.3f} tol at z={z[rd.argmax()]:.6g}")
    assert rf.max() <= 1.0 and rd.max() <= 1.0


# ---------------------------------------------------------------------------------------------
# split arithmetic
# ---------------------------------------------------------------------------------------------
def test_split_pieces_are_exact_remainders():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(4096) * 10.0 ** rng.uniform(-6, 6, 4096)).astype(np.float32)
    p = sw.split_pieces(x, 3)
    for q in p:  # bf16: the low 16 bits are zero
        assert not (q.view(np.uint32) & 0xFFFF).any()
    x8 = x.astype(np.float64)
    assert np.all(np.abs(x8 - p[0]) <= 2.0 ** -8 * np.abs(x8))
    assert np.all(np.abs(x8 - p[0] - p[1].astype(np.float64)) <= 2.0 ** -16 * np.abs(x8))
    r = x8 - sum(q.astype(np.float64) for q in p)
    assert np.all(np.abs(r) <= 2.0 ** -24 * np.abs(x8))
    # the three-piece six-product NT form is fp32-class, the two-piece TN form 2^-16-class
    a, b = rng.standard_normal((40, 300)), rng.standard_normal((300, 50))
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    ref = a32.astype(np.float64) @ b32.astype(np.float64)
    S = np.abs(a32).astype(np.float64) @ np.abs(b32).astype(np.float64)
    nt = np.abs(sw.split_matmul(a32, b32, 3, sw.NT_TERMS) - ref).max() / (sw.U * S).min()
    tn = (np.abs(sw.split_matmul(a32, b32, 2, sw.TN_TERMS) - ref) / (sw.U * S)).max()
    assert nt < 1.0 and 1.0 < tn <= sw.TN_SPLIT_WORST


# ---------------------------------------------------------------------------------------------
# sensitivity: one-element kernel bugs
# ---------------------------------------------------------------------------------------------
def _mutations(b, cfg, p):
    W = sw._weights(p, cfg)

    def drop_edge(a1, rec):  # (a) one edge missing from one node's a_1 segment
        e = 5
        a1 = a1.copy()
        a1[rec["dst_s"][e]] -= rec["h"][1][e]
        return a1

    def lost_low_pieces(pre2, rec):  # (b) one message row reduced to its first bf16 piece
        r = 7
        m = sw.message(rec["a"][1], rec["h"][1], rec["src_s"], rec["rev_s"])[r]
        m_hi = sw.split_pieces(m, 1)[0].astype(np.float64)
        pre2 = pre2.copy()
        pre2[r] = m_hi @ W["wl"][1].T + W["bl"][1] + W["sig"][1] * rec["h"][0][r]
        return pre2

    def missing_slab(dw, rec):  # (c) one 32-row K slab left out of one 16 x 16 tile of dW_1
        m = sw.message(rec["a"][1], rec["h"][1], rec["src_s"], rec["rev_s"])
        dw = dw.copy()
        dw[:16, :16] -= (np.asarray(rec["dpre"][1][32:64, :16], np.float64).T
                         @ m[32:64, :16]).astype(dw.dtype)
        return dw

    def neighbour_derivative(dp, rec):  # (d) act' of the neighbouring column for one element
        r, c = 9, 3
        z = np.asarray(rec["pre"][1], np.float64)
        d = on.act_grad(z[r, c:c + 2], cfg["act"])
        dp = dp.copy()
        dp[r, c] = dp[r, c] / d[0] * d[1]
        return dp

    return {"a1": drop_edge, "pre2": lost_low_pieces, "convs.1.lin.weight": missing_slab,
            "dpre.0": neighbour_derivative}


@pytest.fixture(scope="module")
def small_case():
    b = make_batch(6, 14, 16, n_mace=7, seed=3)
    cfg, p, dy = _setup(b, 40, 3, "silu")
    return b, cfg, p, dy


@pytest.mark.parametrize("stage", ["a1", "pre2", "convs.1.lin.weight", "dpre.0"])
def test_one_element_bug_exceeds_its_stage_bar(stage, small_case):
    b, cfg, p, dy = small_case
    hook = _mutations(b, cfg, p)[stage]
    clean = sw.judge(_chain(b, cfg, p, dy, ops=sw.F32, tn_family="b3"), p, cfg, TORCH_F32)
    assert not failures(clean)
    rec = _chain(b, cfg, p, dy, ops=sw.F32, tn_family="b3", hooks={stage: hook})
    rows = sw.judge(rec, p, cfg, TORCH_F32)
    over = [r["stage"] for r in rows if not r["rho"] <= r["bar"]]
    # the stage that is wrong is found, and nothing downstream is blamed for it
    assert over == [stage], over


def test_lost_low_pieces_pass_the_end_to_end_bars(small_case):
    """The gap the per-stage tests close: mutation (b) pushed through the remaining float64
    stages still meets test_gpu_parity's prediction and gradient bars against the oracle."""
    b, cfg, p, dy = small_case
    rec = _chain(b, cfg, p, dy, inputs=True, hooks={"pre2": _mutations(b, cfg, p)["pre2"]})
    y, cache = on.forward(p, b.x, b.edge_index, b.edge_attr, b.batch, cfg["D"], cfg["act"], True,
                          b.num_graphs)
    gin = {}
    g = on.backward(p, cache, dy, gin)
    assert np.abs(rec["y"] - y).max() > 0  # the mutation did reach the output
    assert_y_close(rec["y"], y)
    for k in g:
        assert_g_close(rec["grads"][k], g[k], k,
                       cache.get("skip_abs", {}).get(k) if k.startswith("skip") else None)
    assert_g_close(rec["dx"], gin["x"], "x")
    assert_g_close(rec["de"], gin["edge_attr"], "edge_attr")


# ---------------------------------------------------------------------------------------------
# the standalone DMPNNConv: oracle/stagewise.conv_stages (tests/test_gpu_conv_stagewise.py)
# ---------------------------------------------------------------------------------------------
def _conv_chain(i, ops=sw.REF, hooks=None):
    return sw.conv_chain(i["edge_index"], i["N"], i["h"], i["weight"], i["bias"], i["grad_a"],
                         i["grad_out"], i["mean"], ops, hooks)


@pytest.mark.parametrize("case", ["h45_both", "h45_no_grad_a", "h45_no_grad_out",
                                  "sparse_mean_h45"])
def test_conv_stages_reproduce_torch_autograd(case):
    """conv_stages fed its own float64 outputs: rho = 0, and equal to torch float64 autograd of
    the reference conv (GNN.py: propagate, then lin(a[src] - flipped pairs of h))."""
    i = conv_inputs(case)
    rec = _conv_chain(i)
    for name, got, st in sw.conv_stages(rec):
        assert sw.rho(got, st)[0] == 0.0, name
    ei = torch.from_numpy(i["edge_index"])
    E, H, N = ei.shape[1], i["h"].shape[1], i["N"]
    t8 = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    h, w, b = (t8(i[k]).clone().requires_grad_(True) for k in ("h", "weight", "bias"))
    a = torch.zeros(N, H, dtype=torch.float64).index_add(0, ei[1], h)
    if i["mean"]:  # PyG scatter mean: / max(count, 1)
        a = a / torch.bincount(ei[1], minlength=N).clamp(min=1).double()[:, None]
    rev = torch.flip(h.view(E // 2, 2, H), dims=[1]).reshape(E, H)
    out = torch.nn.functional.linear(a[ei[0]] - rev, w, b)
    loss = 0.0
    if i["grad_a"] is not None:
        loss = loss + (a * t8(i["grad_a"])).sum()
    if i["grad_out"] is not None:
        loss = loss + (out * t8(i["grad_out"])).sum()
    loss.backward()

    def close(got, ref, name):
        ref = ref.detach().numpy()
        err = np.abs(np.asarray(got) - ref).max() / (np.abs(ref).max() + 1e-300)
        assert err <= 1e-12, (name, err)

    close(rec["a"], a, "a")
    close(rec["out"], out, "out")
    close(rec["grad_h"], h.grad, "grad_h")
    if i["grad_out"] is None:  # the ABI's zeroed gradients; autograd leaves them unset
        assert w.grad is None and b.grad is None
        assert not rec["grad_weight"].any() and not rec["grad_bias"].any()
    else:
        close(rec["grad_weight"], w.grad, "grad_weight")
        close(rec["grad_bias"], b.grad, "grad_bias")


@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_conv_fp32_stand_in_meets_the_bars(case):
    rows = sw.conv_judge(_conv_chain(conv_inputs(case), ops=sw.F32), TORCH_F32)
    assert [r["stage"] for r in rows] == ["a", "out", "grad_weight", "grad_bias", "grad_h"]
    assert all(np.isfinite(r["rho_ref"]) for r in rows)
    bad = failures(rows)
    assert not bad, "\n".join(bad)


def _conv_mutations(i):
    E = i["edge_index"].shape[1]

    def paired_with_itself(out, rec):  # one edge's message formed from h[e] instead of h[e ^ 1]
        e = 11
        out = out.copy()
        m = rec["a"][rec["edge_index"][0, e]] - rec["h"][e]
        out[e] = (m.astype(np.float64) @ rec["weight"].T.astype(np.float64) + rec["bias"])
        return out

    def missing_last_split(dw, rec):  # the last split (2 rows of E = 322) left out of one tile
        assert E % 64 == 2
        m = sw.message(rec["a"], rec["h"], rec["edge_index"][0], np.arange(E) ^ 1)
        dw = dw.copy()
        dw[:16, :16] -= (np.asarray(rec["grad_out"][E - 2:, :16], np.float64).T
                         @ m[E - 2:, :16]).astype(dw.dtype)
        return dw

    return {"out": paired_with_itself, "grad_weight": missing_last_split}


@pytest.mark.parametrize("stage", ["out", "grad_weight"])
def test_conv_one_element_bug_exceeds_its_stage_bar(stage):
    i = conv_inputs("h45_both")
    assert not failures(sw.conv_judge(_conv_chain(i, ops=sw.F32), TORCH_F32))
    rec = _conv_chain(i, ops=sw.F32, hooks={stage: _conv_mutations(i)[stage]})
    over = [r["stage"] for r in sw.conv_judge(rec, TORCH_F32) if not r["rho"] <= r["bar"]]
    assert over == [stage], over


def test_conv_in_degree_zero_scale_bug_exceeds_the_aggregate_bar():
    """Mean aggregation's scale of a node without incoming edges, 1 / max(0, 1) = 1.  Its segment
    sum is exactly 0 and in a paired edge list it is no edge's source either, so a scale of 0 in
    place of 1 changes no output bit (asserted: nothing can observe it); the bug that scale
    guards against, 1 / in-degree = inf, makes the row 0 * inf and exceeds the bar of ``a`` alone."""
    i = conv_inputs("sparse_mean_h45")
    deg = np.bincount(i["edge_index"][1], minlength=i["N"])
    v = int(np.flatnonzero(deg == 0)[3])
    assert v not in i["edge_index"]
    clean = _conv_chain(i, ops=sw.F32)
    assert not failures(sw.conv_judge(clean, TORCH_F32))

    def scaled_by(s):
        def hook(a, rec):
            a = a.copy()
            with np.errstate(invalid="ignore"):
                a[v] = a[v] * np.float32(s)  # in place of the * 1 of inv_deg[v]
            return a
        return hook

    zero = _conv_chain(i, ops=sw.F32, hooks={"a": scaled_by(0.0)})
    for k in ("a", "out", "grad_weight", "grad_bias", "grad_h"):
        assert zero[k].tobytes() == clean[k].tobytes(), k
    rec = _conv_chain(i, ops=sw.F32, hooks={"a": scaled_by(np.inf)})
    over = [r["stage"] for r in sw.conv_judge(rec, TORCH_F32) if not r["rho"] <= r["bar"]]
    assert over == ["a"], over
