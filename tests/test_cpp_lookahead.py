"""The lookahead option of the drop-in C++ API (extra_params["turboinfer.lookahead"] / env TI_LOOKAHEAD), driven
through tests/cpp/lookahead_check on the mini_gqa_w4 golden model (the oracle's weights under the reference's
names, as test_cpp_logprobs.py builds it): with 4 drafts per step InferenceEngine::generate returns the golden's
greedy tokens, every step's reference margin above 3 * TOL (assert_greedy skips none); values outside [0, 15]
and the option together with the e4m3 KV cache throw; with the option absent the output is the same tokens."""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cpp_api import LIB, read, write
from test_gpu_engine import assert_greedy

pytestmark = pytest.mark.gpu

f32 = np.float32
BIN = os.path.join(ROOT, "tests", "cpp", "bin", "lookahead_check")
SRC = os.path.join(ROOT, "tests", "cpp", "lookahead_check.cpp")


@pytest.fixture(scope="module")
def lookahead_check():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", ROOT, "-j8", "all"], check=True)
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(SRC):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++20", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-o", BIN,
                        "-L" + os.path.dirname(LIB), "-lturboinfer_amd",
                        "-Wl,-rpath,$ORIGIN/../../../turboinfer_amd/lib"], check=True)

    def run(*args, env=None):
        e = {k: v for k, v in os.environ.items() if k not in ("TI_LOOKAHEAD", "TI_KV_BITS")}
        e.update(env or {})
        return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600, env=e)
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
    mdir = tmp_path_factory.mktemp("mini_gqa_w4_la")
    lines = [f"meta {cfg['vocab']} {cfg['hidden']} {cfg['layers']} {cfg['heads']} {cfg['inter']} {cfg['rope_theta']!r}"]
    for j, (k, v) in enumerate(w.items()):
        write(mdir / f"t{j}.bin", v.astype(f32))
        lines.append(f"{k} t{j}.bin")
    (mdir / "manifest.txt").write_text("\n".join(lines) + "\n")
    return d, cfg, mdir


def generated(run, model, tmp_path, option, env=None):
    d, cfg, mdir = model
    prompt = d["prompt"].astype(np.int32)
    n_new = len(d["tokens"]) - len(prompt)
    out = tmp_path / f"o_{option}.bin"
    r = run(mdir, write(tmp_path / "p.bin", prompt), cfg["bits"], option, n_new, out, env=env)
    return r, out, prompt.tolist(), n_new


@pytest.mark.parametrize("option,env", [("4", None), ("15", None), ("-", {"TI_LOOKAHEAD": "7"}), ("-", None), ("0", None)],
                         ids=["k4", "k15", "env7", "absent", "zero"])
def test_generate_returns_the_golden_greedy_tokens(lookahead_check, model, tmp_path, option, env):
    d = model[0]
    r, out, prompt, n_new = generated(lookahead_check, model, tmp_path, option, env)
    assert r.returncode == 0, f"lookahead_check failed:\n{r.stdout}\n{r.stderr}"
    toks = read(out).tolist()
    assert toks[:len(prompt)] == prompt
    assert_greedy(toks[len(prompt):], d["tokens"].tolist()[len(prompt):], d["logits"][len(prompt) - 1:], f"lookahead {option}")


@pytest.mark.parametrize("option,env,msg", [("16", None, "lookahead must be"), ("-1", None, "lookahead must be"),
                                            ("-", {"TI_LOOKAHEAD": "16"}, "lookahead must be"),
                                            ("4", {"TI_KV_BITS": "8"}, "fp16 KV cache")],
                         ids=["k16", "negative", "env16", "with_kv8"])
def test_bad_option_values_throw(lookahead_check, model, tmp_path, option, env, msg):
    r, out, _, _ = generated(lookahead_check, model, tmp_path, option, env)
    assert r.returncode == 2 and msg in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(out)
