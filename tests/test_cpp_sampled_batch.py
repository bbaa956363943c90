"""Sampled requests of the drop-in C++ API stay on the device (InferenceEngine::generate_batch), driven through
tests/cpp/sampled_batch_check on the mini_gqa_w4 golden model (the oracle's weights under the reference's names,
as test_cpp_logprobs.py builds it).

A group of sampled requests (here top_k = 1 with include_logprobs, so the tokens are decided) goes through
ti_engine_generate_sampled with n streams instead of the host-sampler loop, which env TI_BATCH_SAMPLE_DEVICE=0
keeps; one such request with TI_LOOKAHEAD verifies n-gram drafts (ti_engine_generate_lookahead_sampled).  The
prompts were picked on the CPU oracle for greedy margins above 6 * TOL * max|logit| at every step (10.8, 15.8 and
22.9 for the three 6-token prompts, 7.1 for the repeating one, whose 24 greedy tokens the bookkeeping model of
tests/lookahead_ref.py verifies in 14 steps at k = 4), so every route returns the same tokens."""
from __future__ import annotations

import json
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cpp_api import LIB, write

pytestmark = pytest.mark.gpu

f32 = np.float32
BIN = os.path.join(ROOT, "tests", "cpp", "bin", "sampled_batch_check")
SRC = os.path.join(ROOT, "tests", "cpp", "sampled_batch_check.cpp")
PROMPTS = [[40, 238, 399, 75, 258, 396], [181, 279, 257, 360, 405, 471], [398, 255, 493, 159, 416, 401]]
REPEATING = [[53, 71, 218] * 4]
ENV_KEYS = ("TI_LOOKAHEAD", "TI_KV_BITS", "TI_BATCH_SAMPLE_DEVICE")


@pytest.fixture(scope="module")
def check():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", ROOT, "-j8", "all"], check=True)
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(SRC):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++20", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-o", BIN,
                        "-L" + os.path.dirname(LIB), "-lturboinfer_amd",
                        "-Wl,-rpath,$ORIGIN/../../../turboinfer_amd/lib"], check=True)

    def run(*args, env=None):
        e = {k: v for k, v in os.environ.items() if k not in ENV_KEYS}
        e.update(env or {})
        r = subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600, env=e)
        assert r.returncode == 0, f"sampled_batch_check failed:\n{r.stdout}\n{r.stderr}"
        runs: dict = {}
        for line in r.stdout.splitlines():
            w = line.split()
            if w[:1] != ["run"]:
                continue
            d = runs.setdefault(w[1], dict(tokens={}, logprobs={}, forward_passes=None))
            if w[2] == "forward_passes":
                d["forward_passes"] = int(w[3])
            else:
                d[w[4]][int(w[3])] = [int(x) if w[4] == "tokens" else float(x) for x in w[5:]]
        return runs
    return run


@pytest.fixture(scope="module")
def model(golden, oracle, tmp_path_factory):
    """(cfg, manifest directory of the mini_gqa_w4 model)."""
    from pyoracle import OracleModel
    d = golden("decode_mini_gqa_w4")
    cfg = json.loads(str(d["cfg"]))
    m = OracleModel(oracle, cfg, int(d["seed"][0]), float(d["jitter"][0]))
    w = m.weights()
    m.close()
    mdir = tmp_path_factory.mktemp("mini_gqa_w4_sb")
    lines = [f"meta {cfg['vocab']} {cfg['hidden']} {cfg['layers']} {cfg['heads']} {cfg['inter']} {cfg['rope_theta']!r}"]
    for j, (k, v) in enumerate(w.items()):
        write(mdir / f"t{j}.bin", v.astype(f32))
        lines.append(f"{k} t{j}.bin")
    (mdir / "manifest.txt").write_text("\n".join(lines) + "\n")
    return cfg, mdir


def test_sampled_group_takes_the_device_route(check, model, tmp_path):
    cfg, mdir = model
    new = 8
    pf = write(tmp_path / "p.bin", np.array(PROMPTS, np.int32))
    dev = check(mdir, cfg["bits"], "greedy_logprobs", pf, new)
    host = check(mdir, cfg["bits"], "greedy_logprobs", pf, new, env={"TI_BATCH_SAMPLE_DEVICE": "0"})
    for i in range(len(PROMPTS)):
        toks = dev["logprobs"]["tokens"][i]
        assert len(toks) == new and toks == dev["plain"]["tokens"][i] == host["logprobs"]["tokens"][i]
        lps = dev["logprobs"]["logprobs"][i]
        assert len(lps) == new and all(math.isfinite(x) and x <= 0.0 for x in lps)
        assert dev["plain"]["logprobs"][i] == []
    # the device route prefills the prompts (one chunk each) and then takes one step per new token; the host
    # loop takes one step per prompt token as well
    assert dev["logprobs"]["forward_passes"] < host["logprobs"]["forward_passes"]


def test_lookahead_under_sampling(check, model, tmp_path):
    cfg, mdir = model
    new = 24
    pf = write(tmp_path / "p.bin", np.array(REPEATING, np.int32))
    plain = check(mdir, cfg["bits"], "greedy_logprobs", pf, new)["logprobs"]
    la = check(mdir, cfg["bits"], "greedy_logprobs", pf, new, env={"TI_LOOKAHEAD": "4"})["logprobs"]
    assert len(plain["tokens"][0]) == new and la["tokens"][0] == plain["tokens"][0]
    assert len(la["logprobs"][0]) == new and all(x == 0.0 for x in la["logprobs"][0])     # one survivor: p = 1
    assert la["forward_passes"] < plain["forward_passes"]


def test_default_config_batch_completes(check, model, tmp_path):
    cfg, mdir = model
    new = 8
    pf = write(tmp_path / "p.bin", np.array(PROMPTS, np.int32))
    got = check(mdir, cfg["bits"], "default", pf, new)["default"]
    for i in range(len(PROMPTS)):
        toks, lps = got["tokens"][i], got["logprobs"][i]
        assert 1 <= len(toks) <= new and all(0 <= t < cfg["vocab"] for t in toks)
        assert len(toks) == new or toks[-1] == 2                  # only EOS ends a request early
        assert len(lps) == len(toks) and all(math.isfinite(x) and x <= 0.0 for x in lps)
