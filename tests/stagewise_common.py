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
