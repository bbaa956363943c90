"""ti_engine_generate_lookahead against the oracle's greedy decode and the plain-Python model of the step's
bookkeeping (tests/lookahead_ref.py).

Prompt [3, 500, 1023, 17, 250], jitter 0.1, 24 new tokens, KV fill seed 77.  Seeds searched on the CPU oracle
(tools/margin_search.py's method): every one of the 24 steps has a top-2 margin above the 3 * TOL = 6e-3 of
max|logit| that assert_greedy demands, which skips no step:
  MID (GQA 8, head_dim 64)   fill 0   seed 30  min margin 2.8e-2      fill 300  seed 32  1.7e-2
  MHA (4 / 4, head_dim 128)  fill 0   seed 31  1.11e-2                fill 300  seed 40  1.26e-2
The tokens must equal the oracle's whatever the corpus (none, the oracle continuation itself, that continuation
with every fifth token off by one), and the statistics must equal the model's exactly: at k = 15 with the true
corpus 24 tokens in 3 steps with 21 drafts accepted, at k = 4 6 to 8 steps, with no corpus 20 to 24.
"""
from __future__ import annotations

import numpy as np
import pytest

import lookahead_ref as R
from test_gpu_engine import MID, TOL, _oracle_tokens, assert_greedy, engine_for

pytestmark = pytest.mark.gpu

MHA = dict(MID, heads=4, kv_heads=4, head_dim=128)
PROMPT, JIT, N_NEW, KV_SEED, NGRAM = [3, 500, 1023, 17, 250], 0.1, 24, 77, 3
MODELS = {"MID-0": (MID, 0, 30), "MID-300": (MID, 300, 32), "MHA-0": (MHA, 0, 31), "MHA-300": (MHA, 300, 40)}
_REF: dict = {}


def reference(oracle, name):
    """The oracle's 24 greedy tokens and logits of a model, computed once for the module."""
    if name not in _REF:
        cfg, fill, seed = MODELS[name]
        _REF[name] = _oracle_tokens(oracle, cfg, seed, JIT, PROMPT, N_NEW, fill, KV_SEED)
    return _REF[name]


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    _REF.clear()


def make_engine(ti, name, splits=0, bits=None, max_seq=None):
    cfg, fill, seed = MODELS[name]
    e = engine_for(ti, dict(cfg, bits=bits or cfg["bits"]), max_seq=max_seq, splits=splits)
    e.synth(seed, JIT)
    if fill:
        e.fill_kv(0, fill, KV_SEED)
    return e, fill


def corpora(ref, vocab):
    return {"none": None, "true": list(ref), "garbled": [(t + 1) % vocab if i % 5 == 4 else t for i, t in enumerate(ref)]}


@pytest.mark.parametrize("k", [1, 4, 15])
@pytest.mark.parametrize("name", list(MODELS))
def test_tokens_and_stats(ti, oracle, name, k):
    ref, ref_logits = reference(oracle, name)
    e, fill = make_engine(ti, name)
    for cname, corpus in corpora(ref, MODELS[name][0]["vocab"]).items():
        got, st = e.generate_lookahead(PROMPT, N_NEW, k=k, ngram=NGRAM, corpus=corpus, start_pos=fill)
        assert_greedy(got.tolist(), ref, ref_logits, f"{name} k {k} corpus {cname}")
        _, want, _ = R.simulate(PROMPT, corpus, ref, k, NGRAM, N_NEW)
        assert st == want, f"{name} k {k} corpus {cname}: stats {st}, model {want}"
        if cname == "true" and k >= 4 and fill:
            assert st["steps"] < N_NEW and st["accepted"] > 0      # a build that never accepts fails here
        if cname == "true" and k == 15:
            assert (st["steps"], st["accepted"]) == (3, 21)
    e.close()


@pytest.mark.parametrize("name", ["MID-300", "MHA-300"])
def test_key_split_attention_in_the_step(ti, oracle, name):
    """The same request with the verify step's attention forced to 7 splits of the 300-key prefix (the automatic
    choice at max_seq 512 is 4)."""
    ref, ref_logits = reference(oracle, name)
    e, fill = make_engine(ti, name, splits=7)
    got, st = e.generate_lookahead(PROMPT, N_NEW, k=15, ngram=NGRAM, corpus=ref, start_pos=fill)
    assert_greedy(got.tolist(), ref, ref_logits, f"{name} 7 splits")
    assert (st["steps"], st["accepted"]) == (3, 21)
    e.close()


@pytest.mark.parametrize("second", ["lookahead", "generate"])
@pytest.mark.parametrize("name", ["MID-300", "MHA-0"])
def test_continuation(ti, oracle, name, second):
    """12 tokens, then 12 more from start_pos + prompt_len + 11 with the 12th token as the prompt."""
    ref, ref_logits = reference(oracle, name)
    e, fill = make_engine(ti, name)
    a, _ = e.generate_lookahead(PROMPT, 12, k=4, ngram=NGRAM, corpus=ref, start_pos=fill)
    assert_greedy(a.tolist(), ref[:12], ref_logits[:12], f"{name} first half")
    at = fill + len(PROMPT) + 11
    if second == "lookahead":
        b, _ = e.generate_lookahead([int(a[11])], 12, k=4, ngram=NGRAM, corpus=ref, start_pos=at)
    else:
        b = e.generate([[int(a[11])]], 12, start_pos=[at])[0]
    assert_greedy(b.tolist(), ref[12:], ref_logits[12:], f"{name} second half by {second}")
    e.close()


@pytest.mark.parametrize("name", ["MID-0", "MHA-300"])
def test_stop_token(ti, oracle, name):
    ref, _ = reference(oracle, name)
    stop = ref[9]
    n = ref.index(stop) + 1
    e, fill = make_engine(ti, name)
    e.set_stop(stop)
    got, st = e.generate_lookahead(PROMPT, N_NEW, k=4, ngram=NGRAM, corpus=ref, start_pos=fill)
    _, want, _ = R.simulate(PROMPT, ref, ref, 4, NGRAM, N_NEW, stop)
    assert got.tolist() == ref[:n] + [-1] * (N_NEW - n)
    assert st == want and st["produced"] == n and st["steps"] < N_NEW
    e.set_stop(-1)
    got, st = e.generate_lookahead(PROMPT, N_NEW, k=4, ngram=NGRAM, corpus=ref, start_pos=fill)
    assert got.tolist() == ref and st["produced"] == N_NEW
    e.close()


def test_graphs_coexist_and_counters(ti, oracle):
    ref, _ = reference(oracle, "MID-300")
    e, fill = make_engine(ti, "MID-300")
    before = e.generate([PROMPT], N_NEW, start_pos=[fill])[0].tolist()
    d0, p0 = e.counters()
    got, st = e.generate_lookahead(PROMPT, N_NEW, k=4, ngram=NGRAM, corpus=ref, start_pos=fill)
    d1, p1 = e.counters()
    assert d1 - d0 == st["steps"] and p1 - p0 == 1          # 4 prompt tokens: one chunk
    after = e.generate([PROMPT], N_NEW, start_pos=[fill])[0].tolist()
    assert before == after == got.tolist() == ref
    d1, p1 = e.counters()
    got1, st1 = e.generate_lookahead(PROMPT[-1:], 3, k=4, ngram=NGRAM, start_pos=fill + 4)   # one-token prompt: no chunk
    assert e.counters() == (d1 + st1["steps"], p1) and got1.tolist() == ref[:3]
    e.close()


def test_head_room(ti, oracle):
    """start_pos + prompt_len + max_new - 1 + k == max_seq runs (and stays inside the cache: the tokens are
    right and the replays after `done` are idle); one more token is an argument error."""
    ref, ref_logits = reference(oracle, "MID-0")
    k = 4
    max_seq = len(PROMPT) + N_NEW - 1 + k
    e, _ = make_engine(ti, "MID-0", max_seq=max_seq)
    got, st = e.generate_lookahead(PROMPT, N_NEW, k=k, ngram=NGRAM, corpus=ref)
    assert_greedy(got.tolist(), ref, ref_logits, "tight head-room")
    with pytest.raises(ti.TiError, match="ti error 1: ti_engine_generate_lookahead"):
        e.generate_lookahead(PROMPT, N_NEW + 1, k=k, ngram=NGRAM)
    with pytest.raises(ti.TiError, match="ti error 1: ti_engine_generate_lookahead"):
        e.generate_lookahead(PROMPT, N_NEW, k=k + 1, ngram=NGRAM)
    e.close()


def test_argument_errors(ti):
    e, _ = make_engine(ti, "MID-0")
    d0 = e.counters()
    ok = dict(prompt=PROMPT, max_new=4, k=4, ngram=3, corpus=None, stream=0, start_pos=0)
    for bad in (dict(stream=1), dict(stream=-1), dict(prompt=[]), dict(max_new=0), dict(k=0), dict(k=16), dict(ngram=0),
                dict(ngram=9), dict(prompt=[3, 1024]), dict(prompt=[-1]), dict(corpus=[5, 1024]), dict(start_pos=-1),
                dict(start_pos=512 - 5 - 4 + 1 - 4 + 1)):
        with pytest.raises(ti.TiError, match="ti error 1: ti_engine_generate_lookahead"):
            e.generate_lookahead(**dict(ok, **bad))
    assert e.counters() == d0                                  # nothing was enqueued
    e.generate_lookahead(**dict(ok, start_pos=512 - 5 - 4 + 1 - 4))
    e.close()


def test_kv8_engine_is_unsupported(ti):
    e, _ = make_engine(ti, "MID-0", bits=4 | ti.BITS_KV8)
    with pytest.raises(ti.TiError, match="ti error 3: ti_engine_generate_lookahead"):
        e.generate_lookahead(PROMPT, 4, k=4)
    e.close()
