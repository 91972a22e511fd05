"""bench.py's command line: a plain run prints the headline line and nothing
that takes a run of its own, --full adds the roofline, and --dump-outputs
writes the last timed step's outputs as float32 .npy files."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import bench

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_default():
    argv, sys.argv = sys.argv, ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"]
    try:
        args = bench.parse()
    finally:
        sys.argv = argv
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (3, 2, False, None)


def test_dump_outputs_float32_and_fixed_sample(tmp_path, monkeypatch):
    """Small arrays are written whole; one above its share of the limit is cut
    to the same sorted sample every time, and the files stay inside the limit."""
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 2 * 100)  # 100 elements per array
    tensors = {"loss": torch.tensor(1.5, dtype=torch.bfloat16),
               "big": torch.arange(1000, dtype=torch.float64).reshape(10, 100)}
    bench.dump_outputs(str(tmp_path / "a"), tensors)
    bench.dump_outputs(str(tmp_path / "b"), tensors)
    loss, got = np.load(tmp_path / "a" / "loss.npy"), np.load(tmp_path / "a" / "big.npy")
    assert loss.dtype == np.float32 and loss.shape == () and loss == 1.5
    assert got.dtype == np.float32 and got.shape == (100,)
    assert np.all(np.diff(got) > 0) and np.all(got == np.round(got)) and 0 <= got[0] and got[-1] < 1000
    assert np.array_equal(got, np.load(tmp_path / "b" / "big.npy"))
    assert loss.nbytes + got.nbytes <= bench.DUMP_LIMIT_BYTES


def _run(monkeypatch, capsys, *extra):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "c1",
                                      *extra])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path, monkeypatch, capsys):
    """BASELINE C1 (fp32, C=16, 18 blocks, batch 128), two timed steps; a
    second run with the same arguments writes the same files bit for bit (same
    seeded inputs, deterministic reductions)."""
    d = _run(monkeypatch, capsys, "--dump-outputs", str(tmp_path / "a"))
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["dtype"] == "f32"
    # the line rounds ms_per_step to 1e-3 ms and value to 0.1 images/s
    assert d["value"] == pytest.approx(128 / d["ms_per_step"] * 1e3, rel=5e-4 / d["ms_per_step"] + 1e-4)
    assert d["roofline"] is None and d["cpu_baseline"] is None
    assert d["config"]["live_gradient_fraction"] >= 0.9
    out = {p.stem: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(out) == ["grads", "loss", "params", "probs"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
    assert out["probs"].shape == (128, 10) and np.allclose(out["probs"].sum(1), 1, atol=1e-5)
    init = bench.bench_params(16, 18)
    assert out["grads"].shape == out["params"].shape == init.shape
    assert np.abs(out["grads"]).max() > 0 and round(float(out["loss"].reshape(-1)[0]), 4) == d["config"]["final_loss"]
    # the parameters are those after the Adam updates: a coordinate with a gradient has moved by about lr per
    # step (three steps summing back to the same float is a coincidence: 1 % allowed)
    live = out["grads"] != 0
    assert np.mean(out["params"][live] != init[live]) > 0.99
    _run(monkeypatch, capsys, "--dump-outputs", str(tmp_path / "b"))
    for name, a in out.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy"))), name


@pytest.mark.gpu
def test_plain_run_spends_little_outside_its_steps():
    """A plain run of the headline workload in a process of its own: start to
    exit, less the (steps + warmup) steps at ms_per_step, stays under 30 s."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    t0 = time.perf_counter()
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    wall = time.perf_counter() - t0
    assert res.returncode == 0, res.stderr[-3000:]
    d = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][0])
    assert d["steps"] == 5 and d["roofline"] is None and d["cpu_baseline"] is None
    outside = wall - 7 * d["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.2f} s in all, {outside:.2f} s outside its steps")
    assert outside < 30.0


@pytest.mark.gpu
def test_full_adds_the_roofline(monkeypatch, capsys):
    d = _run(monkeypatch, capsys, "--full", "--timed-steps", "1", "--no-random-leg", "--no-cpu-baseline")
    assert d["roofline"]["avg_us"] > 0 and set(d["roofline"]["kernels"]) >= {"fwd", "bwd"}
    assert d["ms_per_step"] > 0 and d["cpu_baseline"] is None
