"""GPU (-m gpu): `bench.py --dump-outputs DIR` writes what the timed path returned in its last step (a fixed, seeded row sample of
every linear's output, float32, at most 64 MB), `--steps` sets the number of timed steps, and the same arguments give the same
inputs -- hence the same outputs -- from run to run.  A run without --full measures the headline only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"attention.qkv": 12288, "mlp.gate": 11008, "mlp.proj": 4096}


def _bench(out_dir, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--tokens", "8192", "--steps", str(steps),
                        "--warmup", "1", "--no-small-m", "--no-decode-step", "--no-sweeps", "--no-cpu-baseline",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_dumps_the_last_steps_outputs_reproducibly(tmp_path):
    rec = _bench(tmp_path / "a", 3)
    assert rec["steps"] == 3 and rec["roofline"]["launches"] == 3 * 96 and rec["ms_per_step"] > 0
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(f"{n}.npy" for n in SHAPES), files
    total = 0
    for name, N in SHAPES.items():
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (256, N), (name, a.dtype, a.shape)
        assert np.isfinite(a).all() and np.abs(a).max() > 0, name
        total += a.nbytes
    assert total <= 64 << 20
    rec2 = _bench(tmp_path / "b", 1)
    assert rec2["steps"] == 1 and rec2["roofline"]["launches"] == 96
    for name in SHAPES:   # the int8 part is exact and the fp32 outlier part may only change its summation order
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.abs(a.astype(np.float64) - b).max() <= 1e-3 * np.abs(a).max(), name


INFORMATIONAL = ("small_m", "config0", "decode_step", "int4", "mid_m", "chunk_sweep", "configs", "cpu_baseline")


def _run(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--tokens", "8192", "--steps", "1",
                        "--warmup", "1", *extra], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_only_and_full_adds_the_rest():
    """A run without --full times the steps and prints the contract fields (with the roofline of those steps' own events), and
    none of the informational measurements; --full runs them, and its --no-* options still leave parts out."""
    rec = _run()
    assert rec["metric"] == "prefill_tokens_per_sec" and rec["unit"] == "tokens/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "int8" and rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["roofline"]["launches"] == 96
    assert not [k for k in INFORMATIONAL if k in rec], sorted(rec)
    rec = _run("--full", "--no-decode-step", "--no-sweeps", "--no-cpu-baseline")
    assert "us_per_call" in rec["small_m"]["config0_bs32_4096x4096"] and "error" not in rec["config0"], rec.get("small_m")
    assert not [k for k in ("decode_step", "int4", "chunk_sweep", "configs", "cpu_baseline", "mid_m") if k in rec], sorted(rec)
