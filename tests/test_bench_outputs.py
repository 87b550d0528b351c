"""bench.py --dump-outputs and --full.

CPU: dump_outputs writes float32 arrays, whole when small and otherwise at a fixed seeded
index set, and refuses to write more than DUMP_MAX_BYTES.  GPU: one small plain run of the
command itself writes the last step's outputs, identically from run to run of the same
arguments, times exactly --steps steps and leaves the --full measurements out.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _params(sizes):
    out = []
    g = torch.Generator().manual_seed(3)
    for i, n in enumerate(sizes):
        p = torch.nn.Parameter(torch.zeros(n))
        p.grad = torch.randn(n, generator=g)
        out.append((f"block.{i}.weight", p))
    return out


def test_dump_outputs_whole_and_sampled(tmp_path):
    big = bench.DUMP_GRAD_ELEMS + 1000
    params = _params([7, bench.DUMP_GRAD_ELEMS, big])
    x_tilde = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(4))
    losses = {"bpp": torch.tensor(1.5), "total_loss": torch.tensor(2.25, requires_grad=True)}
    total = bench.dump_outputs(str(tmp_path / "a"), x_tilde, losses, params)
    bench.dump_outputs(str(tmp_path / "b"), x_tilde, losses, params)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["x_tilde.npy", "loss.bpp.npy", "loss.total_loss.npy"]
                           + [f"grad.block.{i}.weight.npy" for i in range(3)])
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype == np.float32 for a in got.values())
    assert total == sum(a.nbytes for a in got.values()) <= bench.DUMP_MAX_BYTES
    assert np.array_equal(got["x_tilde.npy"], x_tilde.numpy())                      # whole, in its shape
    assert got["loss.total_loss.npy"].tolist() == [2.25]
    for i in (0, 1):
        assert np.array_equal(got[f"grad.block.{i}.weight.npy"], params[i][1].grad.numpy())
    s = got["grad.block.2.weight.npy"]
    assert s.shape == (bench.DUMP_GRAD_ELEMS,)
    assert np.isin(s, params[2][1].grad.numpy()).all()                              # a sample of the gradient
    for n in names:                                                                 # the same sample every time
        assert np.array_equal(got[n], np.load(tmp_path / "b" / n))


def test_dump_outputs_refuses_more_than_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000)
    with pytest.raises(SystemExit, match="--dump-outputs"):
        bench.dump_outputs(str(tmp_path / "c"), torch.zeros(1, 3, 16, 16), {}, [])
    assert not list((tmp_path / "c").glob("*.npy"))


@pytest.mark.gpu
def test_plain_run_dumps_last_step_and_skips_full_measurements(tmp_path):
    def run(out):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
               "--batch", "2", "--size", "128", "--dump-outputs", str(out)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, p.stdout
        return json.loads(lines[0])

    rec = run(tmp_path / "a")
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert rec["unit"] == "images/s" and rec["higher_is_better"] is True and rec["dtype"] == "fp32"
    assert abs(rec["value"] - 2 / (rec["ms_per_step"] * 1e-3)) <= 1e-2 * rec["value"]
    assert rec["roofline"] is None and rec["cpu_baseline"] is None and rec["optimizer_step_ms"] is None
    run(tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert "x_tilde.npy" in names and "loss.total_loss.npy" in names and any(n.startswith("grad.") for n in names)
    xt = np.load(tmp_path / "a" / "x_tilde.npy")
    assert xt.shape == (2, 3, 128, 128) and xt.dtype == np.float32
    assert abs(float(np.load(tmp_path / "a" / "loss.bpp.npy")[0]) - rec["bpp"]) <= 1e-4
    for n in names:
        a = np.load(tmp_path / "a" / n)
        assert np.isfinite(a).all(), n
        assert np.array_equal(a, np.load(tmp_path / "b" / n)), n
