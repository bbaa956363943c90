"""The guide_file option of the drop-in C++ API (extra_params["turboinfer.guide_file"] / TI_GUIDE_FILE), driven
through tests/cpp/guide_check on the mini_gqa_w4 golden model (the oracle's weights under the reference's names, as
test_cpp_logprobs.py builds it), with the three requests of test_cpp_shared_prefix.py.

A guide file written here drives generate and generate_batch to sequences guide_ref.run accepts, on every route: a
group on the sampled device loop, a request alone, include_logprobs, and the host-sampler loop
(TI_BATCH_SAMPLE_DEVICE=0, ti_guide_apply) -- a forced path whatever the engine's draws, and the cycle over ids
mod 3 (a sequence may end early at generate()'s end-of-sequence token 2, which the cycle allows in its third state).
Ban: a greedy config (top_k 1) under one state that omits every request's greedy first token emits each request's
runner-up; the CPU oracle's margin between the runner-up and the next allowed logit is asserted above
6 * TOL * max|logit| (measured 2.2 %, 19 % and 2.6 %).  A bad file, beam search and lookahead > 0 each exit non-zero
with the reason in stderr."""
from __future__ import annotations

import json
import os
import struct
import subprocess

import numpy as np
import pytest

import guide_ref as G
from conftest import ROOT
from test_cpp_api import LIB, write
from test_cpp_shared_prefix import OWN, PREFIX, WANT
from test_gpu_engine import TOL

pytestmark = pytest.mark.gpu

f32 = np.float32
BIN = os.path.join(ROOT, "tests", "cpp", "bin", "guide_check")
SRC = os.path.join(ROOT, "tests", "cpp", "guide_check.cpp")
NEW = 8
PROMPTS = [PREFIX + o for o in OWN]
FORCED = [17, 501, 3, 3, 256, 511]
ENV_KEYS = ("TI_GUIDE_FILE", "TI_REPETITION_PENALTY", "TI_PRESENCE_PENALTY", "TI_FREQUENCY_PENALTY", "TI_SHARE_PREFIX",
            "TI_SHARE_MIN", "TI_KV_BITS", "TI_LOOKAHEAD", "TI_BATCH_SAMPLE_DEVICE")


def write_guide(path, g: G.Guide, magic=b"TIGD", version=1, cut=0):
    blob = magic + struct.pack("<iiiq", version, g.n_states, g.start, len(g.tokens))
    blob += g.row_ptr.astype("<i8").tobytes() + g.tokens.astype("<i4").tobytes() + g.next.astype("<i4").tobytes()
    with open(path, "wb") as f:
        f.write(blob[: len(blob) - cut])
    return str(path)


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
        assert r.returncode in (0, 3), f"guide_check failed:\n{r.stdout}\n{r.stderr}"
        runs: dict = {"beam": None, "rc": r.returncode, "stderr": r.stderr}
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
    """(cfg, manifest directory of the mini_gqa_w4 model, the prompts' file, the oracle's first-step logits)."""
    from pyoracle import OracleModel
    d = golden("decode_mini_gqa_w4")
    cfg = json.loads(str(d["cfg"]))
    m = OracleModel(oracle, cfg, int(d["seed"][0]), float(d["jitter"][0]))
    w = m.weights()
    m.close()
    first = []
    for p in PROMPTS:
        m = OracleModel(oracle, cfg, int(d["seed"][0]), float(d["jitter"][0]))
        for tok in p:
            _, lg = m.step(tok)
        m.close()
        first.append(np.array(lg, f32))
    mdir = tmp_path_factory.mktemp("mini_gqa_w4_guide")
    lines = [f"meta {cfg['vocab']} {cfg['hidden']} {cfg['layers']} {cfg['heads']} {cfg['inter']} {cfg['rope_theta']!r}"]
    for j, (k, v) in enumerate(w.items()):
        write(mdir / f"t{j}.bin", v.astype(f32))
        lines.append(f"{k} t{j}.bin")
    (mdir / "manifest.txt").write_text("\n".join(lines) + "\n")
    rows = np.full((len(PROMPTS), max(map(len, PROMPTS))), -1, np.int32)
    for i, p in enumerate(PROMPTS):
        rows[i, :len(p)] = p
    return cfg, mdir, write(mdir / "prompts.bin", rows), first


def every_run(runs):
    for name in ("batch", "logprobs"):
        for i in range(len(PROMPTS)):
            yield name, i, runs[name][i]
    yield "alone", 0, runs["alone"][0]


def assert_beam_refused(runs):
    assert runs["rc"] == 3 and runs["beam"].startswith("threw") and "guide" in runs["beam"], runs["beam"]
    assert "beam search" in runs["stderr"] and "guide" in runs["stderr"]


@pytest.mark.parametrize("top_k", [1, 40])
@pytest.mark.parametrize("env", [{}, {"TI_BATCH_SAMPLE_DEVICE": "0"}], ids=["device_loop", "host_sampler_loop"])
def test_a_guide_file_drives_generate_to_accepted_sequences(check, model, env, top_k):
    cfg, mdir, pf, _ = model
    V = cfg["vocab"]
    forced = G.forced(V, FORCED)
    runs = check(mdir, cfg["bits"], pf, NEW, top_k, "turboinfer.guide_file=" + write_guide(mdir / "forced.tigd", forced), env=env)
    for name, i, toks in every_run(runs):
        assert toks[:6] == FORCED and G.run(forced, toks)[1], (name, i, toks)
    assert_beam_refused(runs)
    cyc = G.cycle(V, 3)
    runs = check(mdir, cfg["bits"], pf, NEW, top_k, env=dict(env, TI_GUIDE_FILE=write_guide(mdir / "cycle.tigd", cyc)))
    for name, i, toks in every_run(runs):
        assert G.run(cyc, toks)[1] and (len(toks) == NEW or toks[-1] == 2) and len(toks) >= 1, (name, i, toks)
    assert_beam_refused(runs)


def test_a_greedy_config_under_a_ban_gives_the_runner_up(check, model):
    cfg, mdir, pf, first = model
    V = cfg["vocab"]
    plain = check(mdir, cfg["bits"], pf, NEW, 1)
    assert plain["rc"] == 0 and plain["beam"] == "ok"
    assert [plain["batch"][i] for i in range(len(PROMPTS))] == WANT
    banned = [w[0] for w in WANT]
    g = G.ban(V, banned)
    want = []
    for i, lg in enumerate(first):
        assert int(np.argmax(lg)) == banned[i]
        allowed = G.mask(g, 0, lg)
        order = np.argsort(allowed)[::-1]
        margin, mx = float(allowed[order[0]] - allowed[order[1]]), float(np.max(np.abs(lg)))
        print(f"\nrequest {i}: runner-up {order[0]} leads {order[1]} by {margin / mx:.4f} of max|logit|")
        assert margin > 6 * TOL * mx, "re-pick the prompts"
        want.append(int(order[0]))
    runs = check(mdir, cfg["bits"], pf, NEW, 1, "turboinfer.guide_file=" + write_guide(mdir / "ban.tigd", g))
    for name, i, toks in every_run(runs):
        assert toks[0] == want[i] and not set(toks) & set(banned), (name, i, toks)


def test_bad_files_and_combinations_exit_non_zero(check, model):
    cfg, mdir, pf, _ = model
    V = cfg["vocab"]
    good = G.cycle(V, 3)
    unsorted = G.cycle(V, 3)
    unsorted.tokens = unsorted.tokens[::-1].copy()
    cases = [
        (str(mdir / "missing.tigd"), "cannot be opened"),
        (write_guide(mdir / "magic.tigd", good, magic=b"TIGX"), "no TIGD magic"),
        (write_guide(mdir / "version.tigd", good, version=2), "version 2"),
        (write_guide(mdir / "short.tigd", good, cut=6), "truncated"),
        (write_guide(mdir / "unsorted.tigd", unsorted), "strictly ascending"),
        (write_guide(mdir / "vocab.tigd", G.cycle(V + 1, 3)), "outside [0, vocab"),
    ]
    for path, msg in cases:
        r = check(mdir, cfg["bits"], pf, NEW, 1, "turboinfer.guide_file=" + path, fails=True)
        assert r.returncode == 2 and msg in r.stderr and "guide" in r.stderr, (path, r.stderr)
    ok = write_guide(mdir / "ok.tigd", good)
    for args, env in ((("turboinfer.guide_file=" + ok, "turboinfer.lookahead=3"), {}),
                      (("turboinfer.guide_file=" + ok,), {"TI_LOOKAHEAD": "3"})):
        r = check(mdir, cfg["bits"], pf, NEW, 1, *args, env=env, fails=True)
        assert r.returncode == 2 and "a guide and lookahead exclude each other" in r.stderr, r.stderr
