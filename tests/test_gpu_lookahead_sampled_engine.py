"""ti_engine_generate_lookahead_sampled against the CPU oracle's sampler, teacher-forced, and the plain-Python
model of the step's bookkeeping (tests/lookahead_ref.py).

The sampler runs at T = 1.0, top_k = 2, top_p = 1.0, and the draws are CONSTRUCTED so that every decision has a
margin: per new token the more probable of the two survivors is taken, on every fourth token (t % 4 == 3) the
other one, so a build that ignores the draws fails; the draw is the midpoint of the chosen token's interval of u,
found by bisection on oracle.sample_token.  With eps = TOL * max|oracle logit| of the step, sampled_reference
asserts at every step (no step is skipped; "re-pick the seed" as assert_greedy does):
  (a) the 2nd-to-3rd logit gap is at least 3 eps, so the survivor set is stable;
  (b) the interval's half-width is at least 3 (e^{2 eps / T} - 1), the most any cumulative boundary moves when
      every logit moves by eps.
Prompt [3, 500, 1023, 17, 250], jitter 0.1, 24 new tokens, KV fill seed 77.  Seeds and their worst-step margins,
(a) as gap / eps and (b) as half-width / bound, checked with oracle.sample_token on the CPU (max|logit| ~ 4):
  MID (GQA 8, head_dim 64)   fill 0   seed 77  (a) 6.38  (b) 5.08      fill 300  seed 41  (a) 3.34  (b) 2.75
  MHA (4 / 4, head_dim 128)  fill 0   seed 31  (a) 3.33  (b) 4.06      fill 300  seed 34  (a) 6.29  (b) 3.91
((a) must be at least 3; (b) at least 1, its bound already holding the factor 3.)
The tokens must equal that sequence whatever the corpus (none, the sequence itself, the sequence with every fifth
token off by one), the statistics must equal the model's exactly, and the log-probabilities must be within
2 * TOL * max|oracle logit| of the oracle sampler's (the bar of test_gpu_kv8_prefill_engine.py).
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import lookahead_ref as R
from test_gpu_engine import MID, TOL, engine_for
from test_gpu_lookahead_engine import JIT, KV_SEED, MHA, MODELS, N_NEW, NGRAM, PROMPT, corpora
from test_gpu_lookahead_engine import make_engine as make_greedy_engine

pytestmark = pytest.mark.gpu

f32 = np.float32
T, TOP_K, TOP_P = 1.0, 2, 1.0
SAMPLED = {"MID-0": (MID, 0, 77), "MID-300": (MID, 300, 41), "MHA-0": (MHA, 0, 31), "MHA-300": (MHA, 300, 34)}
U_TOP = 1.0 - 1e-6       # (at u = 1 the float32 running sum may fall short: the sampler then returns the last index)
_REF: dict = {}


def boundary(oracle, lg, low):
    """The largest float32 u for which the sampler still returns `low` (the lower-indexed survivor), by bisection."""
    lo, hi = 0.0, 1.0                                   # sample(lo) == low, sample(hi) != low
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if oracle.sample_token(lg, T, TOP_K, TOP_P, float(f32(mid)))[0] == low:
            lo = mid
        else:
            hi = mid
    return lo


def sampled_reference(oracle, cfg, seed, fill, what=""):
    """-> (tokens, draws, logprobs, max|logit| per step, worst margins) of the constructed request."""
    from pyoracle import OracleModel
    m = OracleModel(oracle, cfg, seed, JIT)
    if fill:
        m.fill_kv(fill, KV_SEED)
    for tok in PROMPT:
        _, lg = m.step(tok)
    toks, draws, lps, mxs, worst_a, worst_b = [], [], [], [], math.inf, math.inf
    for t in range(N_NEW):
        order = np.lexsort((np.arange(lg.size), -lg))
        first, second, third = (int(i) for i in order[:3])
        mx = float(np.max(np.abs(lg)))
        eps = TOL * mx
        gap = float(lg[second] - lg[third])
        assert gap >= 3 * eps, f"{what} step {t}: 2nd-to-3rd gap {gap:.4g} < 3 eps {3 * eps:.4g} (re-pick the seed)"
        chosen = second if t % 4 == 3 else first
        low, high = min(first, second), max(first, second)
        assert oracle.sample_token(lg, T, TOP_K, TOP_P, 1e-6)[0] == low
        assert oracle.sample_token(lg, T, TOP_K, TOP_P, U_TOP)[0] == high
        c = boundary(oracle, lg, low)
        a, b = (0.0, c) if chosen == low else (c, U_TOP)
        u, half = float(f32(0.5 * (a + b))), 0.5 * (b - a)
        bound = 3 * (math.exp(2 * eps / T) - 1)
        assert half >= bound, f"{what} step {t}: half-width {half:.4g} < {bound:.4g} (re-pick the seed)"
        tok, lp = oracle.sample_token(lg, T, TOP_K, TOP_P, u)
        assert tok == chosen, (what, t, tok, chosen)
        worst_a, worst_b = min(worst_a, gap / eps), min(worst_b, half / bound)
        toks.append(tok)
        draws.append(u)
        lps.append(lp)
        mxs.append(mx)
        _, lg = m.step(tok)
    m.close()
    return toks, np.array(draws, f32), np.array(lps, f32), np.array(mxs, f32), (worst_a, worst_b)


def reference(oracle, name):
    if name not in _REF:
        cfg, fill, seed = SAMPLED[name]
        _REF[name] = sampled_reference(oracle, cfg, seed, fill, name)
    return _REF[name]


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    _REF.clear()


def make_engine(ti, name, bits=None, max_seq=None):
    cfg, fill, seed = SAMPLED[name]
    e = engine_for(ti, dict(cfg, bits=bits or cfg["bits"]), max_seq=max_seq)
    e.synth(seed, JIT)
    if fill:
        e.fill_kv(0, fill, KV_SEED)
    return e, fill


def assert_logprobs(got, want, mxs, what):
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= 2 * TOL * mxs), f"{what}: log-probability error {err.max():.3g} (bars {2 * TOL * mxs.min():.3g}..)"


@pytest.mark.parametrize("k", [1, 4, 15])
@pytest.mark.parametrize("name", list(SAMPLED))
def test_tokens_stats_and_logprobs(ti, oracle, name, k):
    ref, draws, ref_lp, mxs, _ = reference(oracle, name)
    e, fill = make_engine(ti, name)
    for cname, corpus in corpora(ref, SAMPLED[name][0]["vocab"]).items():
        got, lp, st = e.generate_lookahead_sampled(PROMPT, N_NEW, T, TOP_K, TOP_P, draws, k=k, ngram=NGRAM,
                                                   corpus=corpus, start_pos=fill)
        what = f"{name} k {k} corpus {cname}"
        assert got.tolist() == ref, what
        _, want, _ = R.simulate(PROMPT, corpus, ref, k, NGRAM, N_NEW)
        assert st == want, f"{what}: stats {st}, model {want}"
        if cname == "true" and k >= 4:
            assert st["steps"] < N_NEW and st["accepted"] > 0      # a build that never accepts fails here
        assert_logprobs(lp, ref_lp, mxs, what)
    e.close()


def test_draws_decide_the_tokens(ti, oracle):
    """The constructed sequence leaves the greedy one at every fourth token: a build that ignored the draws
    would return the greedy tokens."""
    ref, draws, _, _, _ = reference(oracle, "MHA-0")
    e, fill = make_engine(ti, "MHA-0")
    greedy, _ = e.generate_lookahead(PROMPT, N_NEW, k=4, ngram=NGRAM, start_pos=fill)
    assert greedy.tolist()[:3] == ref[:3] and greedy.tolist()[3] != ref[3]
    e.close()


@pytest.mark.parametrize("name", list(MODELS))
def test_greedy_limit_and_greedy_graph_untouched(ti, name):
    """top_k = 1: the tokens and the statistics of generate_lookahead; a greedy call after a sampled one replays
    a graph without the sampler and returns what it returned before."""
    e, fill = make_greedy_engine(ti, name)
    draws = np.random.RandomState(3).uniform(0, 1, N_NEW).astype(f32)
    for k in (4, 15):
        g0, st0 = e.generate_lookahead(PROMPT, N_NEW, k=k, ngram=NGRAM, start_pos=fill)
        s, lp, st = e.generate_lookahead_sampled(PROMPT, N_NEW, 0.7, 1, 0.9, draws, k=k, ngram=NGRAM, start_pos=fill)
        g1, st1 = e.generate_lookahead(PROMPT, N_NEW, k=k, ngram=NGRAM, start_pos=fill)
        assert s.tolist() == g0.tolist() and st == st0, (name, k)
        assert g1.tolist() == g0.tolist() and st1 == st0, (name, k)
        assert np.all(lp == 0.0)                                   # one survivor: p = 1
    e.close()


@pytest.mark.parametrize("second", ["lookahead_sampled", "generate_sampled"])
@pytest.mark.parametrize("name", ["MID-300", "MHA-0"])
def test_continuation(ti, oracle, name, second):
    """12 tokens, then 12 more from start_pos + prompt_len + 11 with the 12th token as the prompt and the other
    12 draws."""
    ref, draws, ref_lp, mxs, _ = reference(oracle, name)
    e, fill = make_engine(ti, name)
    a, lpa, _ = e.generate_lookahead_sampled(PROMPT, 12, T, TOP_K, TOP_P, draws[:12], k=4, ngram=NGRAM, corpus=ref,
                                             start_pos=fill)
    assert a.tolist() == ref[:12]
    at = fill + len(PROMPT) + 11
    if second == "lookahead_sampled":
        b, lpb, _ = e.generate_lookahead_sampled([int(a[11])], 12, T, TOP_K, TOP_P, draws[12:], k=4, ngram=NGRAM,
                                                 corpus=ref, start_pos=at)
    else:
        b, lpb = e.generate_sampled([[int(a[11])]], 12, T, TOP_K, TOP_P, draws[12:], start_pos=[at])
        b, lpb = b[0], lpb[0]
    assert b.tolist() == ref[12:], f"{name} second half by {second}"
    assert_logprobs(np.concatenate([lpa, lpb]), ref_lp, mxs, f"{name} continued by {second}")
    e.close()


@pytest.mark.parametrize("name", ["MID-300", "MHA-0"])
def test_stop_token(ti, oracle, name):
    ref, draws, ref_lp, mxs, _ = reference(oracle, name)
    stop = ref[9]
    n = ref.index(stop) + 1
    e, fill = make_engine(ti, name)
    e.set_stop(stop)
    got, lp, st = e.generate_lookahead_sampled(PROMPT, N_NEW, T, TOP_K, TOP_P, draws, k=4, ngram=NGRAM, corpus=ref,
                                               start_pos=fill)
    _, want, _ = R.simulate(PROMPT, ref, ref, 4, NGRAM, N_NEW, stop)
    assert got.tolist() == ref[:n] + [-1] * (N_NEW - n)
    assert st == want and st["produced"] == n and st["steps"] < N_NEW
    assert np.all(lp[n:] == 0.0)                                   # 0.0 where the token is -1
    assert_logprobs(lp[:n], ref_lp[:n], mxs[:n], f"{name} up to the stop token")
    e.set_stop(-1)
    got, lp, st = e.generate_lookahead_sampled(PROMPT, N_NEW, T, TOP_K, TOP_P, draws, k=4, ngram=NGRAM, corpus=ref,
                                               start_pos=fill)
    assert got.tolist() == ref and st["produced"] == N_NEW
    e.close()


def test_counters_and_sampler_changes(ti, oracle):
    """decode_steps rises by the verify steps, prefill_chunks by the prompt chunks; other sampler parameters,
    then the first ones again (each change drops and recaptures the graph), give the same tokens."""
    ref, draws, _, _, _ = reference(oracle, "MID-300")
    e, fill = make_engine(ti, "MID-300")
    d0, p0 = e.counters()
    got, _, st = e.generate_lookahead_sampled(PROMPT, N_NEW, T, TOP_K, TOP_P, draws, k=4, ngram=NGRAM, corpus=ref,
                                              start_pos=fill)
    d1, p1 = e.counters()
    assert d1 - d0 == st["steps"] and p1 - p0 == 1          # 4 prompt tokens: one chunk
    other, _, _ = e.generate_lookahead_sampled(PROMPT, 2 * N_NEW + 50, 0.8, 40, 0.9, np.full(2 * N_NEW + 50, 0.5, f32),
                                               k=4, ngram=NGRAM, start_pos=fill)       # (grows the draw buffer too)
    assert other.min() >= 0
    again, _, st2 = e.generate_lookahead_sampled(PROMPT, N_NEW, T, TOP_K, TOP_P, draws, k=4, ngram=NGRAM, corpus=ref,
                                                 start_pos=fill)
    assert again.tolist() == got.tolist() == ref and st2 == st
    d1, p1 = e.counters()
    got1, _, st1 = e.generate_lookahead_sampled(PROMPT[-1:], 3, T, TOP_K, TOP_P, draws[:3], k=4, ngram=NGRAM,
                                                start_pos=fill + 4)                    # one-token prompt: no chunk
    assert e.counters() == (d1 + st1["steps"], p1) and got1.tolist() == ref[:3]
    e.close()


def test_head_room(ti, oracle):
    """start_pos + prompt_len + max_new - 1 + k == max_seq runs; one more token or draft is an argument error."""
    ref, draws, _, _, _ = reference(oracle, "MHA-0")
    k = 4
    max_seq = len(PROMPT) + N_NEW - 1 + k
    e, _ = make_engine(ti, "MHA-0", max_seq=max_seq)
    got, _, _ = e.generate_lookahead_sampled(PROMPT, N_NEW, T, TOP_K, TOP_P, draws, k=k, ngram=NGRAM, corpus=ref)
    assert got.tolist() == ref
    more = np.full(N_NEW + 1, 0.5, f32)
    with pytest.raises(ti.TiError, match="ti error 1: ti_engine_generate_lookahead_sampled"):
        e.generate_lookahead_sampled(PROMPT, N_NEW + 1, T, TOP_K, TOP_P, more, k=k, ngram=NGRAM)
    with pytest.raises(ti.TiError, match="ti error 1: ti_engine_generate_lookahead_sampled"):
        e.generate_lookahead_sampled(PROMPT, N_NEW, T, TOP_K, TOP_P, draws, k=k + 1, ngram=NGRAM)
    e.close()


def test_argument_errors(ti):
    e, _ = make_engine(ti, "MHA-0")
    d0 = e.counters()
    ok = dict(prompt=PROMPT, max_new=4, temperature=T, top_k=TOP_K, top_p=TOP_P, draws=np.full(4, 0.5, f32), k=4, ngram=3,
              corpus=None, stream=0, start_pos=0)
    for bad in (dict(stream=1), dict(stream=-1), dict(prompt=[]), dict(max_new=0), dict(k=0), dict(k=16), dict(ngram=0),
                dict(ngram=9), dict(prompt=[3, 1024]), dict(prompt=[-1]), dict(corpus=[5, 1024]), dict(start_pos=-1),
                dict(start_pos=512 - 5 - 4 + 1 - 4 + 1), dict(draws=None), dict(top_k=0), dict(top_k=1025)):
        with pytest.raises(ti.TiError, match="ti error 1: ti_engine_generate_lookahead_sampled"):
            e.generate_lookahead_sampled(**dict(ok, **bad))
    assert e.counters() == d0                                  # nothing was enqueued
    e.generate_lookahead_sampled(**dict(ok, start_pos=512 - 5 - 4 + 1 - 4))
    e.generate_lookahead_sampled(**dict(ok, top_k=1024))
    e.close()


def test_kv8_engine_is_unsupported(ti):
    e, _ = make_engine(ti, "MHA-0", bits=4 | ti.BITS_KV8)
    with pytest.raises(ti.TiError, match="ti error 3: ti_engine_generate_lookahead_sampled"):
        e.generate_lookahead_sampled(PROMPT, 4, T, TOP_K, TOP_P, np.full(4, 0.5, f32), k=4)
    e.close()
