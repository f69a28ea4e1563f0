"""bench.py's run modes: a plain run measures the headline figure only, `--full` switches the
other measurements back on, `--dump-outputs DIR` writes the last timed step's results.

CPU: the option handling and the writer (whole arrays within the budget, the same seeded sample
of every large array beyond it).
GPU: one plain cfg1 run with `--dump-outputs`, twice: the line carries `ms_per_step` and none of
the `--full` measurements, and the arrays are identical from run to run.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_switches_every_other_measurement_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2", "--diag-blocks", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert (a.profile_steps, a.collate_bench, a.infer_bench, a.cpu_baseline, a.diag_blocks) == \
        (0, 0, 0, 0, 0)


def test_full_keeps_the_measurements_and_their_switches(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and a.profile_steps == 10
    assert a.collate_bench == a.infer_bench == a.cpu_baseline == 1
    a = _parse(monkeypatch, "--full", "--cpu-baseline", "0", "--diag-blocks", "2")
    assert a.cpu_baseline == 0 and a.diag_blocks == 2 and a.infer_bench == 1


def _toy():
    torch.manual_seed(3)
    m = torch.nn.Linear(300, 400)  # weight: 120,000 elements (above the sampling threshold)
    for p in m.parameters():
        p.grad = torch.randn_like(p)
    return m, {"pred": torch.randn(8), "loss": torch.tensor(2.5)}


def test_dump_outputs_writes_every_array_whole_within_the_budget(tmp_path):
    m, last = _toy()
    bench.dump_outputs(str(tmp_path / "d"), m, last)
    names = sorted(os.listdir(tmp_path / "d"))
    assert names == ["grad.bias.npy", "grad.weight.npy", "loss.npy", "param.bias.npy",
                     "param.weight.npy", "pred.npy"]
    for n, t in (("param.weight", m.weight), ("grad.weight", m.weight.grad),
                 ("grad.bias", m.bias.grad), ("pred", last["pred"]), ("loss", last["loss"])):
        a = np.load(tmp_path / "d" / (n + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, t.detach().numpy())


def test_dump_outputs_samples_large_arrays_beyond_the_budget(tmp_path, monkeypatch):
    m, last = _toy()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 400_000)  # the arrays hold 963,236 bytes
    bench.dump_outputs(str(tmp_path / "a"), m, last)
    bench.dump_outputs(str(tmp_path / "b"), m, last)
    total = 0
    for n in os.listdir(tmp_path / "a"):
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert np.array_equal(a, b)  # a fixed sample
        total += a.nbytes
    assert total <= 400_000
    w = np.load(tmp_path / "a" / "param.weight.npy")
    g = np.load(tmp_path / "a" / "grad.weight.npy")
    assert w.ndim == 1 and 40_000 < w.size < 120_000 and w.size == g.size
    # the sample is elements of the array, in order, at the same places in both
    flat = m.weight.detach().numpy().reshape(-1)
    idx = np.sort(np.random.default_rng(0).choice(flat.size, size=w.size, replace=False))
    assert np.array_equal(w, flat[idx])
    assert np.array_equal(g, m.weight.grad.numpy().reshape(-1)[idx])
    # small arrays stay whole
    assert np.array_equal(np.load(tmp_path / "a" / "param.bias.npy"), m.bias.detach().numpy())


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(cuda_device, tmp_path):
    # the two runs side by side (half the wall time; their warmups then differ in length)
    procs = [subprocess.Popen(
        [sys.executable, "-u", os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "cfg1",
         "--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path / r)],
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in ("a", "b")]
    lines = []
    try:
        for p in procs:
            so, se = p.communicate(timeout=120)
            assert p.returncode == 0, (so + se)[-4000:]
            out = [ln for ln in so.splitlines() if ln.startswith("{")]
            assert len(out) == 1, so[-4000:]
            lines.append(json.loads(out[0]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for j in lines:
        assert j["steps"] == 4 and j["ms_per_step"] > 0 and j["value"] > 0, j
        # ms_per_step is the time of one timed step (printed to 1e-4 ms)
        assert j["value"] == pytest.approx(32 * 1e3 / j["ms_per_step"], rel=5e-3), j
        assert j["roofline"] is None and j["cpu_baseline"] is None and j["kernel_breakdown"] == {}
        assert "collate" not in j and "inference" not in j and "diag_blocks" not in j, sorted(j)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"pred.npy", "loss.npy", "param.ffn.weight.npy", "grad.ffn.weight.npy"} <= set(names)
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n
    assert np.load(tmp_path / "a" / "pred.npy").shape == (32,)
    # the 4 timed steps started from the initial weights, whatever the warmup did before: an Adam
    # step moves a weight by at most lr * 1.007 in its first 4 steps (Cauchy-Schwarz over the
    # bias-corrected weights of m and v at beta = 0.9 / 0.999; amsgrad only shrinks it)
    torch.manual_seed(0)
    from cgr_mpnn_3D.models.GNN import GNN
    w0 = GNN(78, 14, depth=2, hidden_sizes=[128] * 2,
             dropout_ps=[0.02] * 2).ffn.weight.detach().numpy()
    w = np.load(tmp_path / "a" / "param.ffn.weight.npy")
    d = np.abs(w - w0).max()
    assert 0 < d <= 4 * 1e-3 * 1.01, d
