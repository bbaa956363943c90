"""InferenceEngine::compute_logprobs of the drop-in C++ API (inference_engine.cpp:873-954 in the
reference), driven through tests/cpp/logprobs_check on the mini_gqa_w4 golden model (the oracle's
weights under the reference's names, as test_cpp_api.py builds it), over the golden's token sequence.

Bar: element i within 2 * TOL * max|logits_i| of log_softmax(golden logits[i])[tokens[i]] (float64) --
the project's logits bar TOL * max|ref| (test_gpu_engine.py) through the 1-Lipschitz log-sum-exp and the
picked logit."""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cpp_api import LIB, read, write
from test_gpu_engine import TOL

pytestmark = pytest.mark.gpu

f32 = np.float32
BIN = os.path.join(ROOT, "tests", "cpp", "bin", "logprobs_check")
SRC = os.path.join(ROOT, "tests", "cpp", "logprobs_check.cpp")


@pytest.fixture(scope="module")
def logprobs_check():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", ROOT, "-j8", "all"], check=True)
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(SRC):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++20", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-o", BIN,
                        "-L" + os.path.dirname(LIB), "-lturboinfer_amd",
                        "-Wl,-rpath,$ORIGIN/../../../turboinfer_amd/lib"], check=True)

    def run(*args):
        return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)
    return run


@pytest.fixture(scope="module")
def model(golden, oracle, tmp_path_factory):
    """(golden arrays, cfg, manifest directory of the mini_gqa_w4 model)."""
    from pyoracle import OracleModel
    d = golden("decode_mini_gqa_w4")
    cfg = json.loads(str(d["cfg"]))
    m = OracleModel(oracle, cfg, int(d["seed"][0]), float(d["jitter"][0]))
    w = m.weights()
    m.close()
    mdir = tmp_path_factory.mktemp("mini_gqa_w4")
    lines = [f"meta {cfg['vocab']} {cfg['hidden']} {cfg['layers']} {cfg['heads']} {cfg['inter']} {cfg['rope_theta']!r}"]
    for j, (k, v) in enumerate(w.items()):
        write(mdir / f"t{j}.bin", v.astype(f32))
        lines.append(f"{k} t{j}.bin")
    (mdir / "manifest.txt").write_text("\n".join(lines) + "\n")
    return d, cfg, mdir


def test_compute_logprobs_matches_reference_logits(logprobs_check, model, tmp_path):
    d, cfg, mdir = model
    ref = d["logits"].astype(np.float64)                  # position i's logits, for every token but the last
    toks = d["tokens"][: len(ref)].astype(np.int32)
    r = logprobs_check(mdir, write(tmp_path / "t.bin", toks), cfg["bits"], tmp_path / "o.bin")
    assert r.returncode == 0, f"logprobs_check failed:\n{r.stdout}\n{r.stderr}"
    lp = read(tmp_path / "o.bin")
    assert lp.shape == (len(toks),) and lp.dtype == np.float32
    top = ref.max(axis=1)
    lse = top + np.log(np.exp(ref - top[:, None]).sum(axis=1))
    for i, t in enumerate(toks):
        want, bar = ref[i, t] - lse[i], 2 * TOL * float(np.max(np.abs(ref[i])))
        print(f"position {i}: lp {lp[i]:.6f} ref {want:.6f} bar {bar:.4g}")
        assert abs(float(lp[i]) - want) <= bar, (i, float(lp[i]), want, bar)


def test_compute_logprobs_rejects_bad_input(logprobs_check, model, tmp_path):
    _, cfg, mdir = model
    r = logprobs_check(mdir, write(tmp_path / "oov.bin", np.array([1, cfg["vocab"], 3], np.int32)), cfg["bits"],
                       tmp_path / "o.bin")
    assert r.returncode != 0 and "out of vocabulary" in r.stderr, (r.returncode, r.stderr)
    r = logprobs_check(mdir, write(tmp_path / "empty.bin", np.zeros(0, np.int32)), cfg["bits"], tmp_path / "o.bin")
    assert r.returncode != 0 and "cannot be empty" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(tmp_path / "o.bin")
