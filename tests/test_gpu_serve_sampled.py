"""Continuous batching with the device sampler (ti_engine_serve_sampled): ti_engine_serve's loop with the step
graph's sampler on, request r's t-th new token decided by draws[r][t] whatever slot and chunk it runs in.

MID, max_batch 3, the 7 prompts of tests/test_gpu_serve.py.  Since the batched kernels compute every row from its
own inputs, tokens and log-probabilities are bit for bit the same whatever the chunking; top_k = 1 returns
serve()'s tokens; and with one-token prompts (no prefill runs) every request equals a host loop over
ti_engine_step on a twin engine with the oracle's sampler and that request's draws -- the method and the bars of
test_gpu_sample.py::test_engine_sampled_generate_matches_host_loop."""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_engine import MID, engine_for
from test_gpu_serve import PROMPTS

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED, JIT, NEW, B = 9, 0.1, 6, 3
T, K, P = 0.8, 40, 0.9
DRAWS = np.random.RandomState(11).uniform(0, 1, (len(PROMPTS), NEW)).astype(f32)


def engine(ti):
    e = engine_for(ti, MID, max_batch=B)
    e.synth(SEED, JIT)
    return e


def same(a, b):
    (ta, la), (tb, lb) = a, b
    return ta == tb and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(la, lb))


def test_chunking_changes_nothing(ti):
    e = engine(ti)
    got4 = e.serve_sampled(PROMPTS, NEW, T, K, P, DRAWS, eos=-1, chunk=4)
    got7 = e.serve_sampled(PROMPTS, NEW, T, K, P, DRAWS, eos=-1, chunk=7)
    got1 = e.serve_sampled(PROMPTS, NEW, T, K, P, DRAWS, eos=-1, chunk=1)
    e.close()
    assert same(got4, got7) and same(got4, got1)
    for toks, lps in zip(*got4):
        assert len(toks) == NEW == len(lps) and all(0 <= t < MID["vocab"] for t in toks)
        assert np.all(np.isfinite(lps)) and np.all(lps <= 0.0)
    # the draws decide: other draws, other tokens
    e = engine(ti)
    other = e.serve_sampled(PROMPTS, NEW, T, K, P, 1.0 - DRAWS, eos=-1, chunk=4)
    e.close()
    assert other[0] != got4[0]


def test_top_k_1_is_serve(ti):
    e = engine(ti)
    full = e.serve(PROMPTS, NEW, eos=-1, chunk=4)
    eos = full[0][1]                       # request 0 stops after its second token
    cut = e.serve(PROMPTS, NEW, eos=eos, chunk=4)
    got_full, lp_full = e.serve_sampled(PROMPTS, NEW, T, 1, P, DRAWS, eos=-1, chunk=4)
    got_cut, lp_cut = e.serve_sampled(PROMPTS, NEW, T, 1, P, DRAWS, eos=eos, chunk=4)
    again = e.serve(PROMPTS, NEW, eos=-1, chunk=4)         # the greedy graph is still the greedy graph
    e.close()
    assert got_full == full == again and got_cut == cut and cut != full
    for toks, lps in zip(got_cut, lp_cut):
        assert len(lps) == len(toks) and np.all(lps == 0.0)           # one survivor: p = 1


def test_requests_match_the_host_loop(ti, oracle):
    """One-token prompts: no prefill, every token comes from a decode step of max_batch rows.  The twin engine
    steps max_batch rows too: the request in row 0, the idle-slot filler (token 0, position 0) in the others."""
    prompts = [[p[-1]] for p in PROMPTS]
    e = engine(ti)
    got, got_lp = e.serve_sampled(prompts, NEW, T, K, P, DRAWS, eos=-1, chunk=4)
    e.close()
    ref = engine(ti)
    for r, p in enumerate(prompts):
        tok, want, want_lp = p[0], [], []
        for pos in range(NEW):
            lg = ref.step([tok] + [0] * (B - 1), [pos] + [0] * (B - 1))[0]
            tok, lp = oracle.sample_token(lg, T, K, P, float(DRAWS[r, pos]))
            want.append(tok)
            want_lp.append(lp)
        assert got[r] == want, f"request {r}"
        np.testing.assert_allclose(got_lp[r], np.array(want_lp, f32), rtol=1e-5, atol=1e-5)
    ref.close()


def test_eos_frees_the_slot_and_later_requests_keep_their_draws(ti):
    e = engine_for(ti, MID, max_batch=2)
    e.synth(SEED, JIT)
    full, full_lp = e.serve_sampled(PROMPTS, NEW, T, K, P, DRAWS, eos=-1, chunk=3)
    eos = full[0][1]                       # request 0 stops after its second token
    cut, cut_lp = e.serve_sampled(PROMPTS, NEW, T, K, P, DRAWS, eos=eos, chunk=3)
    e.close()
    assert len(cut[0]) == 2
    for f, flp, c, clp in zip(full, full_lp, cut, cut_lp):
        n = f.index(eos) + 1 if eos in f else len(f)
        assert c == f[:n]
        assert np.array_equal(clp.view(np.uint32), flp[:n].view(np.uint32))


def test_argument_errors(ti):
    e = engine(ti)
    d0 = e.counters()
    for bad in (dict(top_k=0), dict(top_k=MID["vocab"] + 1), dict(max_new=0), dict(chunk=0)):
        kw = dict(dict(max_new=NEW, top_k=K, chunk=4), **bad)
        with pytest.raises(ti.TiError, match="ti error 1: ti_engine_serve_sampled"):
            e.serve_sampled(PROMPTS, kw["max_new"], T, kw["top_k"], P, np.zeros((len(PROMPTS), kw["max_new"]), f32),
                            eos=-1, chunk=kw["chunk"])
    assert e.counters() == d0
    e.close()
