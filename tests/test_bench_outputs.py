"""bench.py's plain run, --dump-outputs and --full: a plain run prints the headline line
only and can write the last timed step's tokens; --full adds the figures that take runs of their own."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

PLAIN_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_KEYS = {"roofline", "attention_roofline", "kernels", "calibration", "cpu_baseline"}


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_writes_last_tokens_as_float32(tmp_path):
    """dump_outputs with a stand-in engine (CPU): one float32 array [B] holding last_tokens(B)."""
    sys.path.insert(0, ROOT)
    import bench

    class Eng:
        def last_tokens(self, n):
            return np.arange(7, 7 + n, dtype=np.int32) * 18000   # ids up to 128256 stay exact in float32

    class One:
        rank, world = 0, 1

    class Two:
        rank, world = 1, 2

    out = tmp_path / "a" / "b"
    bench.dump_outputs(str(out), Eng(), 3, One())
    bench.dump_outputs(str(out), Eng(), 3, Two())
    assert sorted(p.name for p in out.iterdir()) == ["tokens.npy", "tokens_rank1.npy"]
    t = np.load(out / "tokens.npy")
    assert t.dtype == np.float32 and t.tolist() == [126000.0, 144000.0, 162000.0]


@pytest.mark.gpu
def test_plain_run_is_lean_and_repeatable(tmp_path):
    """Two plain runs with the same arguments: the headline fields only (none of the --full
    figures), --steps timed steps, and the same token from the same seeded inputs."""
    args = ["--gpus", "1", "--model", "tinyllama-1.1b", "--steps", "3", "--warmup", "1"]
    outs = [_bench(*args, "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for o in outs:
        assert PLAIN_KEYS <= set(o) and not (FULL_KEYS & set(o)), sorted(o)
        assert o["steps"] == 3 and o["warmup"] == 1 and o["dtype"] == "w8a16" and o["unit"] == "tokens/s"
        assert o["ms_per_step"] > 0 and abs(o["value"] * o["ms_per_step"] / 1e3 - 1.0) < 1e-3   # 1 stream, 1 GPU
    a, b = (np.load(tmp_path / d / "tokens.npy") for d in ("a", "b"))
    assert a.dtype == np.float32 and a.shape == (1,) and 0 <= a[0] < 32000 and a[0] == int(a[0])
    assert np.array_equal(a, b)


@pytest.mark.gpu
def test_full_run_adds_the_side_figures():
    o = _bench("--gpus", "1", "--model", "tinyllama-1.1b", "--steps", "3", "--warmup", "1", "--full",
               "--no-cpu-baseline", "--kernel-reps", "4", "--stamp-steps", "2")
    assert (PLAIN_KEYS | FULL_KEYS) <= set(o), sorted(o)
    assert o["cpu_baseline"] is None and o["roofline"]["achieved"] > 0 and o["calibration"]["hbm_read_GBps"] > 0
    assert set(o["kernels"]) >= {"qkv", "o", "gate_up", "down", "lm_head"}
