"""The shared-prefix option of the drop-in C++ API (extra_params["turboinfer.share_prefix"] / TI_SHARE_PREFIX), driven
through tests/cpp/shared_prefix_check on the mini_gqa_w4 golden model (the oracle's weights under the reference's
names, as test_cpp_logprobs.py builds it).

Three requests: a common 8-token prefix plus 1, 2 and 3 own tokens, 8 new tokens each.  Prefix and continuations
were picked on the CPU oracle for greedy margins above 6 * TOL * max|logit| at every step (the smallest per request:
2.4e-2, 2.1e-2 and 3.2e-2 of max|logit|) and for texts without the EOS token, so every route returns the same tokens.
With TI_SHARE_PREFIX=4 generate_batch registers the 8 common tokens (ti_engine_share_prefix) and passes the
continuations at start_pos 8: the prefix is one prompt chunk instead of three, and the next call finds it registered.
"""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cpp_api import LIB, write

pytestmark = pytest.mark.gpu

f32 = np.float32
BIN = os.path.join(ROOT, "tests", "cpp", "bin", "shared_prefix_check")
SRC = os.path.join(ROOT, "tests", "cpp", "shared_prefix_check.cpp")
PREFIX = [438, 90, 74, 195, 254, 353, 351, 260]
OWN = [[448], [191, 496], [501, 289, 236]]
WANT = [[117, 117, 117, 117, 59, 317, 471, 317], [100, 484, 117, 467, 274, 50, 484, 484],
        [38, 117, 187, 309, 133, 33, 249, 322]]            # the oracle's greedy tokens
NEW = 8
ENV_KEYS = ("TI_SHARE_PREFIX", "TI_SHARE_MIN", "TI_KV_BITS", "TI_LOOKAHEAD", "TI_BATCH_SAMPLE_DEVICE")


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
        assert r.returncode == 0, f"shared_prefix_check failed:\n{r.stdout}\n{r.stderr}"
        runs: dict = {}
        for line in r.stdout.splitlines():
            w = line.split()
            if w[:1] != ["run"]:
                continue
            d = runs.setdefault(w[1], dict(tokens={}, forward_passes=None))
            if w[2] == "forward_passes":
                d["forward_passes"] = int(w[3])
            else:
                d["tokens"][int(w[3])] = [int(x) for x in w[5:]]
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
    mdir = tmp_path_factory.mktemp("mini_gqa_w4_sp")
    lines = [f"meta {cfg['vocab']} {cfg['hidden']} {cfg['layers']} {cfg['heads']} {cfg['inter']} {cfg['rope_theta']!r}"]
    for j, (k, v) in enumerate(w.items()):
        write(mdir / f"t{j}.bin", v.astype(f32))
        lines.append(f"{k} t{j}.bin")
    (mdir / "manifest.txt").write_text("\n".join(lines) + "\n")
    rows = np.full((len(OWN), len(PREFIX) + max(map(len, OWN))), -1, np.int32)
    for i, o in enumerate(OWN):
        rows[i, :len(PREFIX) + len(o)] = PREFIX + o
    return cfg, mdir, write(mdir / "prompts.bin", rows)


def test_same_tokens_fewer_forward_passes(check, model):
    cfg, mdir, pf = model
    plain = check(mdir, cfg["bits"], pf, NEW)
    for env in ({"TI_SHARE_PREFIX": "4"}, {"TI_SHARE_PREFIX": "4", "TI_SHARE_MIN": "1"}):
        shared = check(mdir, cfg["bits"], pf, NEW, env=env)
        for name in ("greedy", "again", "logprobs"):
            for i in range(len(OWN)):
                assert plain[name]["tokens"][i] == WANT[i], f"plain {name} request {i}"
                assert shared[name]["tokens"][i] == WANT[i], f"{env} {name} request {i}"
            # the prefix is prefilled once, not once per request; the second call finds it registered
            assert shared[name]["forward_passes"] < plain[name]["forward_passes"], (env, name)
        assert shared["again"]["forward_passes"] == shared["greedy"]["forward_passes"] - 1
        assert plain["again"]["forward_passes"] == plain["greedy"]["forward_passes"]
    # a common prefix shorter than the option asks for: the group runs as ever
    short = check(mdir, cfg["bits"], pf, NEW, env={"TI_SHARE_PREFIX": "9"})
    assert short["greedy"] == plain["greedy"]


def test_option_errors(check, model):
    cfg, mdir, pf = model
    r = check(mdir, cfg["bits"], pf, NEW, env={"TI_SHARE_PREFIX": "4", "TI_KV_BITS": "8"}, fails=True)
    assert r.returncode == 2 and "share_prefix needs the fp16 KV cache" in r.stderr, r.stderr
    r = check(mdir, cfg["bits"], pf, NEW, env={"TI_SHARE_PREFIX": "-1"}, fails=True)
    assert r.returncode == 2 and "share_prefix must be" in r.stderr, r.stderr
