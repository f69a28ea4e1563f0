"""CPU: the public surface of gradient-norm clipping (FusedAdam(max_grad_norm=...)) and of the
robust losses (L1Loss, HuberLoss): constructor validation and the state-dict round trip.  No
compute here; the kernels are checked in test_gpu_clip.py and test_gpu_losses.py."""

import copy
import ctypes
import pickle

import pytest
import torch

from cgr_mpnn_3D._amd import native
from cgr_mpnn_3D._amd.loss import HuberLoss, L1Loss, MSELoss
from cgr_mpnn_3D._amd.optim import FusedAdam


def _params():
    return [torch.zeros(4, requires_grad=True), torch.zeros(2, 3, requires_grad=True)]


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("-inf")])
def test_max_grad_norm_rejects_non_positive_and_nan(bad):
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam(_params(), lr=1e-3, max_grad_norm=bad)


@pytest.mark.parametrize("ok", [None, 1e-3, 1.0, 5, float("inf")])
def test_max_grad_norm_accepted_values_land_in_the_param_groups(ok):
    opt = FusedAdam(_params(), lr=1e-3, max_grad_norm=ok)
    assert opt.defaults["max_grad_norm"] == ok
    assert opt.param_groups[0]["max_grad_norm"] == ok


def test_max_grad_norm_per_group_override():
    a, b = _params()
    opt = FusedAdam([dict(params=[a], max_grad_norm=2.0), dict(params=[b])], lr=1e-3)
    assert [g["max_grad_norm"] for g in opt.param_groups] == [2.0, None]


def test_state_dict_round_trip_keeps_max_grad_norm():
    opt = FusedAdam(_params(), lr=1e-3, amsgrad=True, max_grad_norm=2.5)
    sd = copy.deepcopy(opt.state_dict())
    assert sd["param_groups"][0]["max_grad_norm"] == 2.5
    other = FusedAdam(_params(), lr=1e-3, amsgrad=True)
    assert other.param_groups[0]["max_grad_norm"] is None
    other.load_state_dict(sd)
    assert other.param_groups[0]["max_grad_norm"] == 2.5


def test_state_dict_without_the_key_loads_and_means_none():
    opt = FusedAdam(_params(), lr=1e-3, amsgrad=True, max_grad_norm=2.5)
    old = copy.deepcopy(FusedAdam(_params(), lr=1e-3, amsgrad=True).state_dict())
    for g in old["param_groups"]:
        del g["max_grad_norm"]  # as saved before the keyword existed
    opt.load_state_dict(old)
    assert opt.param_groups[0]["max_grad_norm"] is None
    assert opt.grad_norm is None and opt.skipped_steps is None


def test_setstate_without_the_key_means_none():
    opt = FusedAdam(_params(), lr=1e-3)
    state = opt.__getstate__()
    for g in state["param_groups"]:
        del g["max_grad_norm"]
    opt.__setstate__(pickle.loads(pickle.dumps(state)))
    assert opt.param_groups[0]["max_grad_norm"] is None


def test_grad_norm_is_none_without_clipping():
    opt = FusedAdam(_params(), lr=1e-3)
    assert opt.grad_norm is None
    assert opt.skipped_steps is None


def test_clipped_step_rejects_cpu_parameters_and_a_bad_group_value():
    ps = _params()
    opt = FusedAdam(ps, lr=1e-3, max_grad_norm=1.0)
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step()
    opt.param_groups[0]["max_grad_norm"] = -3.0  # set after construction: caught at the step
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.step()


def test_sumsq_partials_counts_the_step_kernels_blocks():
    """Host only: one partial per 1024-element block of every tensor that has a gradient."""
    lib = native.load()
    numels = [1, 1024, 1025, 0, 5000]
    tab = (native.CgrAdamTensor * 6)()
    for i, n in enumerate(numels):
        tab[i] = native.CgrAdamTensor(16, 16, 16, 16, 16, 16, n)
    tab[5] = native.CgrAdamTensor(16, None, 16, 16, 16, 16, 4096)  # grad NULL: p.grad is None
    assert lib.cgr_grad_sumsq_partials(tab, 6) == 1 + 1 + 2 + 0 + 5
    assert lib.cgr_grad_sumsq_partials(tab, 0) == 0
    # a partials buffer that is too small is an error before any launch
    assert lib.cgr_grad_sumsq(tab, 6, ctypes.c_void_p(16), 8, None) != 0
    assert b"too small" in lib.cgr_last_error()


@pytest.mark.parametrize("cls", [L1Loss, HuberLoss])
def test_loss_reduction_validation(cls):
    assert cls().reduction == "mean"  # torch's default
    assert cls("sum").reduction == "sum" and cls(reduction="mean").reduction == "mean"
    with pytest.raises(NotImplementedError):
        cls("none")
    with pytest.raises(NotImplementedError):
        cls(reduction="batchmean")


@pytest.mark.parametrize("bad", [0.0, -0.5, float("nan"), float("inf")])
def test_huber_delta_validation(bad):
    with pytest.raises(ValueError, match="delta"):
        HuberLoss("sum", delta=bad)
    assert HuberLoss("sum").delta == 1.0 and HuberLoss("sum", delta=0.5).delta == 0.5


@pytest.mark.parametrize("fn", [L1Loss("sum"), HuberLoss("sum"), MSELoss("sum")])
def test_losses_share_the_input_checks(fn):
    with pytest.raises(RuntimeError, match="GPU"):
        fn(torch.zeros(4), torch.zeros(4))
