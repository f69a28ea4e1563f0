"""Shared by tests/test_stagewise_refs.py (CPU) and tests/test_gpu_stagewise.py: the torch fp32
evaluation that sets rho_ref, model parameters by state_dict name, and the report writer."""

import numpy as np
import torch
import torch.nn.functional as F

from oracle import stagewise as sw

_ACT = {"relu": F.relu, "silu": F.silu, "gelu": F.gelu, "tanh": torch.tanh,
        "sigmoid": torch.sigmoid, "elu": F.elu, "leaky_relu": F.leaky_relu,
        "softplus": F.softplus, "mish": F.mish, "selu": F.selu}


class TorchF32(sw.Ops):
    """Every stage operation by torch fp32 on the CPU: the honest fp32 implementation whose error
    against the fp64 stage is rho_ref."""

    def __init__(self):
        super().__init__(np.float32)

    @staticmethod
    def _t(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))

    def mm(self, a, b):
        return (self._t(a) @ self._t(b)).numpy()

    def segsum(self, vals, index, n):
        v = self._t(vals)
        out = torch.zeros((n,) + tuple(v.shape[1:]), dtype=torch.float32)
        out.index_add_(0, torch.from_numpy(np.asarray(index, np.int64)), v)
        return out.numpy()

    def total(self, a):
        return self._t(a).sum().numpy()

    def colsum(self, a):
        return self._t(a).sum(dim=0).numpy()

    def act(self, z, name):
        return _ACT[name](self._t(z)).numpy()

    def act_grad(self, z, name):
        t = self._t(z).clone().requires_grad_(True)
        _ACT[name](t).sum().backward()
        return t.grad.numpy()


TORCH_F32 = TorchF32()


def param_names(D, skip):
    """The C-ABI parameter table order (include/cgr_mpnn3d.h) by reference state_dict name."""
    names = ["edge_init.weight", "edge_init.bias"]
    for l in range(D):
        names += [f"convs.{l}.lin.weight", f"convs.{l}.lin.bias"]
    names += ["edge_to_node.weight", "edge_to_node.bias", "ffn.weight", "ffn.bias"]
    if skip:
        names += [f"skip_weights.{l}" for l in range(D)]
    return names


def random_params(rng, F_, Fe, H, D, scale=1.0):
    """Parameters at nn.Linear's init scale (uniform +-1/sqrt(fan_in)), non-trivial skip weights."""
    def lin(o, i):
        k = scale / np.sqrt(i)
        return rng.uniform(-k, k, (o, i)), rng.uniform(-k, k, o)

    p = {}
    p["edge_init.weight"], p["edge_init.bias"] = lin(H, F_ + Fe)
    for l in range(D):
        p[f"convs.{l}.lin.weight"], p[f"convs.{l}.lin.bias"] = lin(H, H)
        p[f"skip_weights.{l}"] = np.asarray(0.5 + 0.25 * l)
    p["edge_to_node.weight"], p["edge_to_node.bias"] = lin(H, F_ + H)
    p["ffn.weight"], p["ffn.bias"] = lin(1, H)
    return {k: np.asarray(v, np.float32) for k, v in p.items()}


def mixed_dy(B, seed=20261):
    """dy of mixed sign and magnitude (|dy| over three decades), fixed seed."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(B) * 10.0 ** rng.uniform(-2.0, 1.0, B)).astype(np.float32)


def failures(rows):
    return [f"{r['stage']}: rho {r['rho']:.2f} > bar {r['bar']:.2f} (rho_ref {r['rho_ref']:.2f}) "
            f"at {r['argmax']}" for r in rows if not r["rho"] <= r["bar"]]


STAGE_ERRORS = []


def write_report(case, rows):
    """Append this case's rows to stage_errors.json in the test report directory (the one
    test_gpu_parity._write_report writes to: CGR_TEST_REPORT_DIR or its default)."""
    from test_gpu_parity import _write_report

    for r in rows:
        STAGE_ERRORS.append(dict(case=case, **{k: r[k] for k in
                                               ("stage", "rho", "rho_ref", "bar", "argmax",
                                                "rho_fp64")}))
    _write_report("stage_errors.json", STAGE_ERRORS)


# ---------------------------------------------------------------------------------------------
# the standalone DMPNNConv's cases, shared by tests/test_gpu_conv_stagewise.py (the kernels) and
# tests/test_stagewise_refs.py (the fp32 stand-in at the same shapes)
# ---------------------------------------------------------------------------------------------
def conv_graph(name):
    """(edge_index [2, E] int64 in reverse-edge pairs, N)."""
    from test_gpu_parity import _hub_batch, _sparse_batch

    from cgr_mpnn_3D._amd.synth import make_batch

    if name == "e322":  # N 147, E 322: a partial last 64-row tile, a last split-K split of 2 rows
        b = make_batch(7, 21, 23, n_mace=40, seed=112)
    elif name == "hub":  # E 1056: dst segments of 150 / 70 / 300 rows, 17 split-K slabs
        b = _hub_batch([150, 3, 70, 300, 5], seed=43)
    elif name == "sparse":  # N 240, E 48: most nodes have in-degree 0
        b = _sparse_batch(6, 40, seed=31)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(b.edge_index, dtype=np.int64), int(b.x.shape[0])


# name: (graph, H, mean aggregation, grad_a given, grad_out given)
CONV_CASES = {
    "h80_both": ("e322", 80, False, True, True),  # NT RN = 5, TN (5, 5), one column tile
    "h80_no_grad_a": ("e322", 80, False, False, True),
    "h80_no_grad_out": ("e322", 80, False, True, False),
    "h160": ("e322", 160, False, True, True),  # two 80-wide tiles each way
    "h100": ("e322", 100, False, True, True),  # RN = 4, a ragged second tile
    "h45_both": ("e322", 45, False, True, True),  # VEC 1, Hp 48
    "h45_no_grad_a": ("e322", 45, False, False, True),
    "h45_no_grad_out": ("e322", 45, False, True, False),
    "h30": ("e322", 30, False, True, True),  # the VEC = 2 weight loader
    "h12": ("e322", 12, False, True, True),  # Kout <= 16: TN RN = 1
    "h528": ("e322", 528, False, True, True),  # above 512: several tiles each way
    "hub_h160": ("hub", 160, False, True, True),
    "sparse_mean_h45": ("sparse", 45, True, True, True),  # in-degree 0: inv_deg = 1
}


def conv_inputs(case):
    """The case's inputs as fp32 numpy: dict(edge_index, N, h, weight, bias, grad_a, grad_out,
    mean); a gradient the case leaves out is None."""
    import zlib

    graph, H, mean, with_ga, with_go = CONV_CASES[case]
    ei, N = conv_graph(graph)
    E = ei.shape[1]
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    k = 1.0 / np.sqrt(H)
    f4 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return dict(edge_index=ei, N=N, mean=mean, h=f4(rng.standard_normal((E, H))),
                weight=f4(rng.uniform(-k, k, (H, H))), bias=f4(rng.uniform(-k, k, H)),
                grad_a=f4(rng.standard_normal((N, H))) if with_ga else None,
                grad_out=f4(rng.standard_normal((E, H))) if with_go else None)


# ---------------------------------------------------------------------------------------------
# the dropout mask's cases, shared by tests/test_gpu_dropout_mask.py (every evaluation site of the
# mask against oracle/dropout.py, bit for bit) and tests/test_dropout_model.py (what wrong masks
# those shapes tell apart)
# ---------------------------------------------------------------------------------------------
MASK_D = 3  # conv layers 0, 1, 2 all occur

# name: (batch, H, p, seed).  Seeds at or above 2^32 in m1, m3, m5 (the key's high half), 0 in m2.
MASK_CASES = {
    "m1": ("base", 64, 0.5, 2**40 + 1234567),  # fused forward, several 64-row tiles
    "m2": ("base", 39, 0.25, 0),  # H % 4 == 3: the last float4 group partial, Hp = 40 != H
    "m3": ("base", 516, 0.1, 0x9E3779B97F4A7C15 % 2**62),  # unfused forward (EpLayer), fp32 TNs
    "m4": ("unpaired", 64, 0.5, 1234567),  # status 4: the unpaired completion form
    "m5": ("hub", 64, 0.02, 2**62 - 1),  # hub segments spanning row tiles
}


def mask_batch(kind):
    from test_gpu_parity import _hub_batch, _shuffled_pairs

    from cgr_mpnn_3D._amd.synth import make_batch

    if kind == "base":  # N 320, E 640: ten 64-row tiles
        return make_batch(16, n_atoms=20, n_bonds=20, n_mace=0, seed=131)
    if kind == "unpaired":  # edges shuffled inside every graph
        return _shuffled_pairs(make_batch(16, n_atoms=20, n_bonds=20, n_mace=0, seed=132), seed=9)
    if kind == "hub":  # E 1056: dst segments of 150 / 70 / 300 rows
        return _hub_batch([150, 3, 70, 300, 5], seed=44)
    raise KeyError(kind)


def mask_model(case, ps=None):
    """(batch, GNN on the CPU in train mode) of a mask case: sigmoid, so act(pre) > 0 and
    h == 0 holds exactly where the element was dropped; learnable skip.  The hub case's layer
    weights are scaled by 0.1: its in-degree-300 sums would otherwise push |pre| past 80, towards
    where a float32 sigmoid underflows to 0."""
    from cgr_mpnn_3D.models.GNN import GNN

    kind, H, p, _ = MASK_CASES[case]
    b = mask_batch(kind)
    torch.manual_seed(17)
    m = GNN(b.x.shape[1], b.edge_attr.shape[1], depth=MASK_D, hidden_sizes=[H] * MASK_D,
            dropout_ps=[p] * MASK_D if ps is None else list(ps), activation_fn=torch.sigmoid,
            use_learnable_skip=True)
    with torch.no_grad():
        for i, w in enumerate(m.skip_weights):
            w.fill_(0.5 + 0.25 * i)
        if kind == "hub":
            for conv in m.convs:
                conv.lin.weight.mul_(0.1)
    return b, m.train()


def model_masks(key, E, H, ps):
    """oracle.dropout.keep_mask of every layer (None where the layer has no dropout): bool
    [E, H] in dst-sorted edge order."""
    from oracle import dropout as od

    return [od.keep_mask(key, l, E, H, p) if od.thresh_scale(p)[0] else None
            for l, p in enumerate(ps)]
