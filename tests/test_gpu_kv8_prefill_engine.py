"""Prompt chunks of engines with the e4m3 KV cache on the MFMA route (ti_attn_prefill_f8): which entry point a
chunk takes (ti_engine_prefill_attn_name), and that the route computes the function the decode route computed.

Routing.  Row-major chunks (up to 16 rows, and more than 64 on int4 engines) take ti_attn_prefill_f8 on a KV8
engine and ti_attn_prefill on an fp16-KV engine; packed chunks (int4, 17 .. 64 rows) keep the decode kernel;
a compat engine has no prefill (TI_ERR_UNSUPPORTED).

Same function as the decode route.  On a ONE-layer engine the cache bytes do not depend on the attention, so
the MFMA route (this process) and the decode route (a fresh child process with TI_ATTN_PREFILL=0: the knob is
read once per process) evaluate one function of the same bytes: read_kv of layer 0 must be byte-identical,
the last-row logits of generate(.., 1) agree within test_gpu_engine.py's TOL (2e-3 of max|logit|, the
project's figure for two correct evaluations of one function on these models), and the log-probabilities of
score within 2 * TOL * max|logit_i|, as test_gpu_score.py reads it (max|logit_i| per position from the fp16-KV
oracle of the same one-layer model: a scale, nothing is compared with it).
Measured on an MI355X (`pytest -s`), worst difference / bar:
  mid70 (int4, one chunk of 70 rows)      last-row logits 2.1e-5 = 0.003 of the bar; log-probabilities 0.061 of theirs
  mid8_40 (int8, chunks of 16, 16, 8 rows) last-row logits identical;                 log-probabilities 0.048
Accuracy on the 3-layer models against the oracle is test_gpu_kv8_engine.py::test_score_and_prefill_vs_oracle,
which now runs on this route.
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_engine import MID, TOL, engine_for
from test_gpu_kv8_engine import kv8
from test_gpu_score import MID8

pytestmark = pytest.mark.gpu

f64 = np.float64
TI_ERR_UNSUPPORTED = 3


def test_routing(ti):
    e = engine_for(ti, kv8(MID))
    assert e.prefill_attn_name(70) == "ti_attn_prefill_f8"
    assert e.prefill_attn_name(40) == "ti_attn_decode_packed_f8"
    assert e.prefill_attn_name(8) == "ti_attn_prefill_f8"
    e.close()
    e = engine_for(ti, kv8(MID8))
    assert e.prefill_attn_name(40) == "ti_attn_prefill_f8"
    e.close()
    e = engine_for(ti, MID)
    assert e.prefill_attn_name(70) == "ti_attn_prefill"
    assert e.prefill_attn_name(40) == "ti_attn_decode_packed"
    L = ti.lib()
    import ctypes as C
    buf = C.create_string_buffer(64)
    assert L.ti_engine_prefill_attn_name(e.h, 0, buf, 64) == 1
    assert L.ti_engine_prefill_attn_name(e.h, 8, None, 64) == 1
    assert L.ti_engine_prefill_attn_name(e.h, 8, buf, 0) == 1
    e.close()
    c = ti.Engine(1000, 256, 2, 4, 4, 64, 1024, bits=16, max_seq=64, max_batch=1, compat=True)
    assert L.ti_engine_prefill_attn_name(c.h, 8, buf, 64) == TI_ERR_UNSUPPORTED
    c.close()


CASES = {"mid70": (MID, 70), "mid8_40": (MID8, 40)}
SEED, JIT, RS = 13, 0.1, 3

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import turboinfer_amd as T
from test_gpu_kv8_prefill_engine import run_case
T.init(0)
name, rows, out = run_case(T, sys.argv[2])
assert name == "ti_attn_decode_f8", name
np.save(sys.argv[3] + "/lp.npy", out[0]); np.save(sys.argv[3] + "/last.npy", out[1])
np.save(sys.argv[3] + "/k.npy", out[2]); np.save(sys.argv[3] + "/v.npy", out[3])
"""


def run_case(ti, case):
    """score + generate(.., 1) of the case's tokens on a one-layer KV8 engine -> (route label of the case's
    row-major chunk size, that size, (log-probs, last-row logits, layer-0 K bytes, V bytes))."""
    cfg, n = CASES[case]
    toks = np.random.RandomState(RS).randint(0, cfg["vocab"], size=n).astype(np.int32)
    e = engine_for(ti, kv8(dict(cfg, layers=1)))
    e.synth(SEED, JIT)
    rows = n if cfg["bits"] == 4 else 16          # int4: one row-major chunk of 70; int8: chunks of 16
    name = e.prefill_attn_name(rows)
    lp = e.score(toks)
    kb, vb = e.read_kv(0, 0, 0, 0, n), e.read_kv(0, 0, 1, 0, n)
    _, last = e.generate([toks.tolist()], 1, want_logits=True)
    e.close()
    return name, rows, (lp, last[0], kb, vb)


@pytest.mark.parametrize("case", list(CASES))
def test_same_function_as_the_decode_route(ti, oracle, tmp_path, case):
    cfg, n = CASES[case]
    name, rows, (lp, last, kb, vb) = run_case(ti, case)
    assert name == "ti_attn_prefill_f8"
    env = dict(os.environ, TI_ATTN_PREFILL="0")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, case, str(tmp_path)], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lp_d, last_d = np.load(tmp_path / "lp.npy"), np.load(tmp_path / "last.npy")
    assert np.array_equal(np.load(tmp_path / "k.npy"), kb) and np.array_equal(np.load(tmp_path / "v.npy"), vb)
    assert kb.dtype == np.uint8 and kb.any() and vb.any()
    # the last-row logits: TOL of max|logit|
    bar = TOL * float(np.max(np.abs(last_d)))
    d_last = float(np.max(np.abs(last.astype(f64) - last_d.astype(f64))))
    # the log-probabilities: 2 TOL max|logit_i|, the scale from the fp16-KV oracle of the same model
    from pyoracle import OracleModel
    toks = np.random.RandomState(RS).randint(0, cfg["vocab"], size=n).astype(np.int32)
    m = OracleModel(oracle, dict(cfg, layers=1), SEED, JIT)
    mx = np.array([np.max(np.abs(np.asarray(m.step(int(t))[1], f64))) for t in toks])
    m.close()
    d_lp = np.abs(lp.astype(f64) - lp_d.astype(f64)) / (2 * TOL * mx)
    print(f"kv8 prefill engine {case}: last-row logits differ by {d_last:.3e} (bar {bar:.3e}, {d_last / bar:.3f} of it); "
          f"log-probs worst {float(d_lp.max()):.3f} of 2 TOL max|logit_i|")
    assert d_last <= bar
    assert d_lp.max() <= 1.0
