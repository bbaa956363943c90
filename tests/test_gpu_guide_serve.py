"""Guided decoding in continuous batching (ti_engine_serve_sampled under ti_engine_set_guide): MID, the 7 prompts of
tests/test_gpu_serve.py.

A request starts in the guide's start state whatever slot it is admitted into, and its state follows its own
tokens whatever chunk they run in: every chunk restarts at step 0 with the previous chunk's last token as its
input, which only the carry row tells the guide kernel.  Forced path (tests/guide_ref.py): with max_batch 2 and 5
requests, chunks of 1, 4 and 7 steps all emit the six forced tokens first -- a freed slot restarts at `start`, and
with chunks of one step every token arrives through the carry -- and give the same bits.  Cycle: one-token prompts
equal the host loop (a twin engine's ti_engine_step logits -> guide_ref -> the oracle's sampler, placed draws; the
bars of tests/test_gpu_penalty_serve.py).  Under a registered prefix (TI_SHARE_MIN=1: the shared attention) the
forced path holds in the serve loop and in ti_engine_generate_sampled at start_pos = prefix length."""
from __future__ import annotations

import numpy as np
import pytest

import guide_ref as G
from test_gpu_engine import MID, engine_for
from test_gpu_serve import PROMPTS

pytestmark = pytest.mark.gpu

f32 = np.float32
V = MID["vocab"]
SEED, JIT, NEW, B = 9, 0.1, 8, 3
T, K, P = 0.8, 40, 0.9
DRAWS = np.random.RandomState(11).uniform(1e-6, 1, (len(PROMPTS), NEW)).astype(f32)


def engine(ti, max_batch=B):
    e = engine_for(ti, MID, max_batch=max_batch)
    e.synth(SEED, JIT)
    return e


def same(a, b):
    (ta, la), (tb, lb) = a, b
    return ta == tb and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(la, lb))


def test_forced_path_in_every_chunking_and_freed_slots(ti):
    prompts = PROMPTS[:5]
    e = engine(ti, max_batch=2)
    plain = e.serve_sampled(prompts, NEW, T, K, P, DRAWS[:5], eos=-1, chunk=4)
    e.set_guide(*G.forced(V).args)
    got = {c: e.serve_sampled(prompts, NEW, T, K, P, DRAWS[:5], eos=-1, chunk=c) for c in (1, 4, 7)}
    e.set_guide(None)
    again = e.serve_sampled(prompts, NEW, T, K, P, DRAWS[:5], eos=-1, chunk=4)
    e.close()
    for c, (toks, lps) in got.items():
        for r in range(5):
            assert toks[r][:6] == G.FORCED and len(toks[r]) == NEW, (c, r, toks[r])
            assert np.all(lps[r][:6] == 0.0) and np.all(np.isfinite(lps[r])), (c, r)
    assert same(got[4], got[1]) and same(got[4], got[7])
    assert same(plain, again) and not same(plain, got[4])


def test_an_early_end_frees_the_slot_for_a_fresh_start(ti):
    """eos = the third forced token: every request ends after three tokens, mid-chunk, and the slot's state has run
    on to the chunk's end when the next request is admitted into it."""
    e = engine(ti, max_batch=2)
    e.set_guide(*G.forced(V).args)
    toks, _ = e.serve_sampled(PROMPTS, NEW, T, K, P, DRAWS, eos=G.FORCED[2], chunk=4)
    e.close()
    for r in range(len(PROMPTS)):
        assert toks[r] == G.FORCED[:3], (r, toks[r])


def test_cycle_one_token_prompts_match_the_host_loop(ti, oracle):
    """No prefill runs; every token comes from a decode step of max_batch rows.  The twin steps max_batch rows
    too: the request in row 0, the idle-slot filler (token 0, position 0) in the others."""
    g = G.cycle(V, 3)
    prompts = [[p[-1]] for p in PROMPTS]
    rng = np.random.RandomState(5)
    ref = engine(ti)
    draws = np.full((len(prompts), NEW), 0.5, f32)
    want, want_lp, worst = [], [], np.inf
    for r, p in enumerate(prompts):
        toks, lps, s = [], [], g.start
        for pos in range(NEW):
            lg = ref.step([(p + toks)[-1]] + [0] * (B - 1), [pos] + [0] * (B - 1))[0]
            if toks:
                s = G.advance(g, s, toks[-1])
            pl = G.mask(g, s, lg)
            pr = oracle.sample_probs(pl, T, K, P)
            cum = np.concatenate(([f32(0)], np.cumsum(pr, dtype=f32)))
            big = np.flatnonzero(pr >= 2e-3)
            j = int(big[rng.randint(big.size)])
            u = f32((np.float64(cum[j]) + np.float64(cum[j + 1])) / 2)
            worst = min(worst, float(u) - float(cum[j]), float(cum[j + 1]) - float(u))
            draws[r, pos] = u
            tok, lp = oracle.sample_token(pl, T, K, P, float(u))
            assert tok == j, "the placed draw picks its survivor"
            toks.append(tok)
            lps.append(lp)
        want.append(toks)
        want_lp.append(lps)
    ref.close()
    print(f"\nsmallest distance of a draw to its interval's ends: {worst:.3e}")
    assert worst >= 1e-4
    e = engine(ti)
    e.set_guide(*g.args)
    got, got_lp = e.serve_sampled(prompts, NEW, T, K, P, draws, eos=-1, chunk=3)
    e.close()
    for r in range(len(prompts)):
        assert G.run(g, got[r])[1], f"request {r}: not accepted"
        assert got[r] == want[r], f"request {r}"
        np.testing.assert_allclose(got_lp[r], np.array(want_lp[r], f32), rtol=1e-5, atol=1e-5)


PREFIX = np.random.RandomState(77).randint(0, V, 40).tolist()


def test_forced_path_under_a_registered_prefix(ti, monkeypatch):
    monkeypatch.setenv("TI_SHARE_MIN", "1")
    e = engine(ti)
    e.share_prefix(PREFIX, B)
    e.set_guide(*G.forced(V).args)
    got, _ = e.serve_sampled(PROMPTS, NEW, T, K, P, DRAWS, eos=-1, chunk=4)
    assert e.shared_prefix() == (len(PREFIX), B)
    for r, toks in enumerate(got):
        assert toks[:6] == G.FORCED and len(toks) == NEW, (r, toks)
    conts = PROMPTS[:B]
    reg, _ = e.generate_sampled(conts, NEW, T, K, P, DRAWS[:B], start_pos=[len(PREFIX)] * B)
    assert e.shared_prefix() == (len(PREFIX), B)
    for m in range(B):
        assert reg[m, :6].tolist() == G.FORCED, (m, reg[m].tolist())
    e.close()
