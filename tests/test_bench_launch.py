"""`python bench.py --gpus N` must start its own ranks (reference launcher: cs_train.py:164-174).
CPU: the launcher path with --dry-run (gloo rendezvous, barrier, max-over-ranks, rank 0's JSON line, exit code)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_self_launch_two_ranks_dry_run():
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout                      # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rccl_world"] == 2 and out["steps"] == 2 and out["warmup"] == 1
    assert sorted(out["ranks"]) == [[0, 0], [1, 1]]
    assert out["max_over_ranks"] == 2.0


def test_self_launch_propagates_a_failing_rank():
    # a rank that dies must turn into a non-zero exit code of `python bench.py --gpus 2`, and no JSON line
    r = _run(["--gpus", "2", "--dry-run"], {"ONIRIS_DRY_RUN_FAIL_RANK": "1", "TORCH_DISTRIBUTED_DEBUG": "OFF"}, timeout=600)
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_mismatched_launcher_is_refused():
    r = _run(["--gpus", "4", "--dry-run"], {"RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "disagree" in (r.stderr + r.stdout)


def test_watchdog_names_the_stage_of_a_hung_collective():
    # rank 1 stops answering after the rendezvous: rank 0's watchdog must end it with exit code 124 and the stage name,
    # well before any outer timeout -- the first 8-GPU run must be diagnosable from its stderr alone
    r = _run(["--gpus", "2", "--dry-run", "--watchdog", "5"], {"ONIRIS_DRY_RUN_HANG_RANK": "1", "TORCH_DISTRIBUTED_DEBUG": "OFF"},
             timeout=300)
    assert r.returncode != 0
    assert "watchdog: rank 0 made no progress" in r.stderr and "all_reduce(MAX)" in r.stderr, r.stderr[-2000:]
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_dump_outputs_are_float32_and_the_same_sample_every_run(tmp_path):
    # --dump-outputs: the last timed step's loss and a fixed seeded sample of parameter-sized arrays, float32 .npy files
    # (run in a child: importing bench.py sets process environment this test process must not carry into later tests)
    code = (
        "import sys, numpy as np, torch\n"
        "import bench\n"
        "torch.manual_seed(0)\n"
        "m = torch.nn.Sequential(torch.nn.Linear(300, 400), torch.nn.Linear(400, 7))\n"
        "named = list(m.named_parameters())\n"
        "out = bench._step_outputs(named, torch.tensor(2.5, dtype=torch.float64), lambda p: 2 * p, [lambda p: 3 * p])\n"
        "bench._write_outputs(sys.argv[1], out)\n")
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, "-c", code, str(tmp_path / d)], cwd=ROOT, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
    import numpy as np
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["ema0.npy", "grads.npy", "loss.npy", "params.npy"]
    a = {n: np.load(tmp_path / "a" / n) for n in names}
    b = {n: np.load(tmp_path / "b" / n) for n in names}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["loss.npy"].tolist() == [2.5]
    n = 300 * 400 + 400 + 400 * 7 + 7
    assert a["params.npy"].shape == (n,)                       # fewer elements than the sample size: all of them
    assert np.array_equal(a["grads.npy"], 2 * a["params.npy"]) and np.array_equal(a["ema0.npy"], 3 * a["params.npy"])
    assert all(np.array_equal(a[k], b[k]) for k in names)


def test_plain_run_options():
    # a plain run leaves the extra measurements to --full; --dump-outputs DIR writes the last timed step's outputs
    r = _run(["--help"])
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_reproducibly(tmp_path):
    """A plain run on the GPU at a small shape, twice: the result line holds the headline fields and none of what --full
    adds, and --dump-outputs writes the same float32 arrays both times (same inputs, reproducible step)."""
    import numpy as np
    lines = []
    for d in ("a", "b"):
        r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "1", "--frames", "8",
                  "--dump-outputs", str(tmp_path / d)], timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    out = lines[0]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["unit"] == "latent-frames/s"
    assert "extra" not in out and out["cpu_baseline"] is None and out["roofline_step"] is None and out["kernels"] is None
    assert not any(k.startswith("ms_") for k in out["config"])
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["ema0.npy", "ema1.npy", "grads.npy", "loss.npy", "params.npy"]
    a = {n: np.load(tmp_path / "a" / n) for n in names}
    b = {n: np.load(tmp_path / "b" / n) for n in names}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["params.npy"].shape == (1 << 21,) and np.abs(a["grads.npy"]).max() > 0
    assert not np.array_equal(a["ema0.npy"], a["params.npy"])       # the EMA profiles trail the parameters
    assert all(np.array_equal(a[n], b[n]) for n in names)
