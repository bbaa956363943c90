"""The penalty options of the drop-in C++ API (extra_params["turboinfer.repetition_penalty" | "turboinfer.presence_penalty"
| "turboinfer.frequency_penalty"] / TI_REPETITION_PENALTY, TI_PRESENCE_PENALTY, TI_FREQUENCY_PENALTY), driven through
tests/cpp/penalty_check on the mini_gqa_w4 golden model (the oracle's weights under the reference's names, as
test_cpp_logprobs.py builds it).

The three requests of test_cpp_shared_prefix.py: their greedy texts, picked there on the CPU oracle for margins above
6 * TOL * max|logit|, repeat themselves (117 117 117 117 59 317 471 317 and 100 484 117 467 274 50 484 484).  With
a presence penalty of 1e4 no request may repeat a token or return one of its prompt, whatever the rounding -- on
every route: a group on the sampled device loop, a request alone, include_logprobs, and the host-sampler loop
(TI_BATCH_SAMPLE_DEVICE=0, ti_penalize_logits).  Beam search throws while the penalties are active; a value that is
no number, or out of range, and penalties together with lookahead throw at construction."""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cpp_api import LIB, write
from test_cpp_shared_prefix import OWN, PREFIX, WANT

pytestmark = pytest.mark.gpu

f32 = np.float32
BIN = os.path.join(ROOT, "tests", "cpp", "bin", "penalty_check")
SRC = os.path.join(ROOT, "tests", "cpp", "penalty_check.cpp")
NEW = 8
PROMPTS = [PREFIX + o for o in OWN]
ENV_KEYS = ("TI_REPETITION_PENALTY", "TI_PRESENCE_PENALTY", "TI_FREQUENCY_PENALTY", "TI_SHARE_PREFIX", "TI_SHARE_MIN",
            "TI_KV_BITS", "TI_LOOKAHEAD", "TI_BATCH_SAMPLE_DEVICE")


@pytest.fixture(scope="module")
def check():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", ROOT, "-j8", "all"], check=True)
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(SRC):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++20", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-o", BIN,
                        "-L" + os.path.dirname(LIB), "-lturboinfer_amd",
                        "-Wl,-rpath,$ORIGIN/../../../turboinfer_amd/lib"], check=True)

    def run(*args, env=None, fails=False):
        e = {k: v for k, v in os.environ.items() if k not in ENV_KEYS}
        e.update(env or {})
        r = subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600, env=e)
        if fails:
            return r
        assert r.returncode == 0, f"penalty_check failed:\n{r.stdout}\n{r.stderr}"
        runs: dict = {"beam": None}
        for line in r.stdout.splitlines():
            w = line.split()
            if w[:1] == ["beam"]:
                runs["beam"] = " ".join(w[1:])
            elif w[:1] == ["run"]:
                runs.setdefault(w[1], {})[int(w[3])] = [int(x) for x in w[5:]]
        return runs
    return run


@pytest.fixture(scope="module")
def model(golden, oracle, tmp_path_factory):
    """(cfg, manifest directory of the mini_gqa_w4 model, the prompts' file)."""
    from pyoracle import OracleModel
    d = golden("decode_mini_gqa_w4")
    cfg = json.loads(str(d["cfg"]))
    m = OracleModel(oracle, cfg, int(d["seed"][0]), float(d["jitter"][0]))
    w = m.weights()
    m.close()
    mdir = tmp_path_factory.mktemp("mini_gqa_w4_pen")
    lines = [f"meta {cfg['vocab']} {cfg['hidden']} {cfg['layers']} {cfg['heads']} {cfg['inter']} {cfg['rope_theta']!r}"]
    for j, (k, v) in enumerate(w.items()):
        write(mdir / f"t{j}.bin", v.astype(f32))
        lines.append(f"{k} t{j}.bin")
    (mdir / "manifest.txt").write_text("\n".join(lines) + "\n")
    rows = np.full((len(PROMPTS), max(map(len, PROMPTS))), -1, np.int32)
    for i, p in enumerate(PROMPTS):
        rows[i, :len(p)] = p
    return cfg, mdir, write(mdir / "prompts.bin", rows)


def repeats(prompt, new):
    seen, n = set(prompt), 0
    for t in new:
        n += t in seen
        seen.add(t)
    return n


def assert_nothing_returns(runs, what):
    for name in ("batch", "logprobs"):
        for i, p in enumerate(PROMPTS):
            assert len(runs[name][i]) == NEW and repeats(p, runs[name][i]) == 0, (what, name, i, runs[name][i])
    assert len(runs["alone"][0]) == NEW and repeats(PROMPTS[0], runs["alone"][0]) == 0, (what, runs["alone"][0])
    assert runs["beam"].startswith("threw") and "penalties" in runs["beam"], (what, runs["beam"])


def test_repeats_without_the_option_none_with_it(check, model):
    cfg, mdir, pf = model
    plain = check(mdir, cfg["bits"], pf, NEW)
    for name in ("batch", "logprobs"):
        assert [plain[name][i] for i in range(len(PROMPTS))] == WANT, name
    assert plain["alone"][0] == WANT[0] and plain["beam"] == "ok"
    assert sum(repeats(p, w) for p, w in zip(PROMPTS, WANT)) >= 3
    # neutral values are "off"
    assert check(mdir, cfg["bits"], pf, NEW, "turboinfer.repetition_penalty=1", "turboinfer.presence_penalty=0.0",
                 "turboinfer.frequency_penalty=0") == plain
    opt = "turboinfer.presence_penalty=1e4"
    assert_nothing_returns(check(mdir, cfg["bits"], pf, NEW, opt), "extra_params")
    assert_nothing_returns(check(mdir, cfg["bits"], pf, NEW, opt, env={"TI_BATCH_SAMPLE_DEVICE": "0"}), "host-sampler loop")
    # a milder set acts too: other tokens than the plain run's
    mild = check(mdir, cfg["bits"], pf, NEW, "turboinfer.repetition_penalty=1.3", "turboinfer.frequency_penalty=0.5")
    assert mild["batch"] != plain["batch"]


def test_environment_spelling(check, model):
    cfg, mdir, pf = model
    assert_nothing_returns(check(mdir, cfg["bits"], pf, NEW, env={"TI_PRESENCE_PENALTY": "1e4"}), "environment")
    # extra_params win over the environment
    plain = check(mdir, cfg["bits"], pf, NEW)
    assert check(mdir, cfg["bits"], pf, NEW, "turboinfer.presence_penalty=0", env={"TI_PRESENCE_PENALTY": "1e4"}) == plain


@pytest.mark.parametrize("args,env,msg", [
    (("turboinfer.repetition_penalty=abc",), {}, "repetition_penalty must be a finite number"),
    (("turboinfer.repetition_penalty=0",), {}, "repetition_penalty must be greater than 0"),
    (("turboinfer.repetition_penalty=-1.5",), {}, "repetition_penalty must be greater than 0"),
    (("turboinfer.presence_penalty=inf",), {}, "presence_penalty must be a finite number"),
    (("turboinfer.frequency_penalty=0.5x",), {}, "frequency_penalty must be a finite number"),
    ((), {"TI_FREQUENCY_PENALTY": "nan"}, "frequency_penalty must be a finite number"),
    (("turboinfer.presence_penalty=0.5", "turboinfer.lookahead=3"), {}, "penalties and lookahead exclude each other"),
    (("turboinfer.presence_penalty=0.5",), {"TI_LOOKAHEAD": "3"}, "penalties and lookahead exclude each other"),
])
def test_bad_values_and_combinations_throw(check, model, args, env, msg):
    cfg, mdir, pf = model
    r = check(mdir, cfg["bits"], pf, NEW, *args, env=env, fails=True)
    assert r.returncode == 2 and msg in r.stderr, r.stderr
