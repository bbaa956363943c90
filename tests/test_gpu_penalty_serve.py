"""Penalties in continuous batching (ti_engine_serve_sampled under ti_engine_set_penalties): MID, max_batch 3, the
7 prompts of tests/test_gpu_serve.py.

A request's context is its prompt, then its new tokens, whatever slot and chunk they ran in.  Every chunk restarts
at step 0 with the previous chunk's last token as its input, which only the carry row tells the penalty kernel:
chunks of 1, 4 and 7 steps must give the same bits, and with chunks of one step (every generated token arrives
through the carry) a presence penalty of 1e4 under top_k = 1 must keep every request from repeating anything.
One-token prompts equal the host loop of tests/test_gpu_penalty_engine.py (a twin engine's ti_engine_step logits ->
tests/penalty_ref.py -> the oracle's sampler, placed draws).  A slot freed by one request starts empty for the
next: with max_batch 2 and an eos that ends request 0 early, every request equals its run alone.  Under a
registered prefix (TI_SHARE_MIN=1, so the 40 keys take the shared attention) the prefix tokens head every
context, in the serve loop and in ti_engine_generate_sampled at start_pos = prefix length."""
from __future__ import annotations

import numpy as np
import pytest

import penalty_ref as R
from test_gpu_engine import MID, engine_for
from test_gpu_serve import PROMPTS

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED, JIT, NEW, B = 9, 0.1, 8, 3
T, K, P = 0.8, 40, 0.9
PEN = (1.3, 0.4, 0.2)
BAN = (1.0, 1e4, 0.0)          # a counted token cannot win again
DRAWS = np.random.RandomState(11).uniform(0, 1, (len(PROMPTS), NEW)).astype(f32)
HALF = np.full((len(PROMPTS), NEW), 0.5, f32)


def engine(ti, max_batch=B):
    e = engine_for(ti, MID, max_batch=max_batch)
    e.synth(SEED, JIT)
    return e


def same(a, b):
    (ta, la), (tb, lb) = a, b
    return ta == tb and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(la, lb))


def repeats(prompt, new):
    seen, n = set(prompt), 0
    for t in new:
        n += t in seen
        seen.add(t)
    return n


def test_chunking_changes_nothing(ti):
    e = engine(ti)
    plain = e.serve_sampled(PROMPTS, NEW, T, K, P, DRAWS, eos=-1, chunk=4)
    e.set_penalties(*PEN)
    got4 = e.serve_sampled(PROMPTS, NEW, T, K, P, DRAWS, eos=-1, chunk=4)
    got7 = e.serve_sampled(PROMPTS, NEW, T, K, P, DRAWS, eos=-1, chunk=7)
    got1 = e.serve_sampled(PROMPTS, NEW, T, K, P, DRAWS, eos=-1, chunk=1)
    e.set_penalties()
    again = e.serve_sampled(PROMPTS, NEW, T, K, P, DRAWS, eos=-1, chunk=4)
    e.close()
    assert same(got4, got7) and same(got4, got1)
    assert same(plain, again) and not same(plain, got4)
    for toks, lps in zip(*got4):
        assert len(toks) == NEW == len(lps) and np.all(np.isfinite(lps)) and np.all(lps <= 0.0)


@pytest.mark.parametrize("chunk", [1, 4, 7])
def test_a_banned_token_never_returns(ti, chunk):
    e = engine(ti)
    plain = e.serve(PROMPTS, NEW, eos=-1, chunk=chunk)
    assert sum(repeats(p, g) for p, g in zip(PROMPTS, plain)) >= 3, plain     # (the model does repeat when it may)
    e.set_penalties(*BAN)
    got, _ = e.serve_sampled(PROMPTS, NEW, 1.0, 1, 1.0, HALF, eos=-1, chunk=chunk)
    e.close()
    for p, g in zip(PROMPTS, got):
        assert len(g) == NEW and repeats(p, g) == 0, (p, g)


def test_one_token_prompts_match_the_host_loop(ti, oracle):
    """No prefill runs; every token comes from a decode step of max_batch rows.  The twin steps max_batch rows
    too: the request in row 0, the idle-slot filler (token 0, position 0) in the others."""
    prompts = [[p[-1]] for p in PROMPTS]
    rng = np.random.RandomState(5)
    ref = engine(ti)
    draws = np.full((len(prompts), NEW), 0.5, f32)
    want, want_lp, worst = [], [], np.inf
    for r, p in enumerate(prompts):
        toks, lps = [], []
        for pos in range(NEW):
            lg = ref.step([(p + toks)[-1]] + [0] * (B - 1), [pos] + [0] * (B - 1))[0]
            pl = R.penalize(lg, p + toks, *PEN)
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
    e.set_penalties(*PEN)
    got, got_lp = e.serve_sampled(prompts, NEW, T, K, P, draws, eos=-1, chunk=4)
    e.close()
    for r in range(len(prompts)):
        assert got[r] == want[r], f"request {r}"
        np.testing.assert_allclose(got_lp[r], np.array(want_lp[r], f32), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("pen,top_k", [(BAN, 1), (PEN, K)], ids=["ban_greedy", "sampled"])
def test_a_freed_slot_starts_empty(ti, pen, top_k):
    e = engine(ti, max_batch=2)
    e.set_penalties(*pen)
    full, _ = e.serve_sampled(PROMPTS, NEW, T, top_k, P, DRAWS, eos=-1, chunk=3)
    eos = full[0][1]                       # request 0 stops after its second token
    cut = e.serve_sampled(PROMPTS, NEW, T, top_k, P, DRAWS, eos=eos, chunk=3)
    assert len(cut[0][0]) == 2
    for r, p in enumerate(PROMPTS):
        alone = e.serve_sampled([p], NEW, T, top_k, P, DRAWS[r: r + 1], eos=eos, chunk=3)
        assert alone[0][0] == cut[0][r], f"request {r}"
        assert np.array_equal(alone[1][0].view(np.uint32), cut[1][r].view(np.uint32)), f"request {r}"
    e.close()


PREFIX = np.random.RandomState(77).randint(0, MID["vocab"], 40).tolist()


def test_a_registered_prefix_heads_every_context(ti, monkeypatch):
    monkeypatch.setenv("TI_SHARE_MIN", "1")
    e = engine(ti)
    e.share_prefix(PREFIX, B)
    e.set_penalties(*BAN)
    got, _ = e.serve_sampled(PROMPTS, NEW, 1.0, 1, 1.0, HALF, eos=-1, chunk=4)
    assert e.shared_prefix() == (len(PREFIX), B)
    for p, g in zip(PROMPTS, got):
        assert len(g) == NEW and repeats(PREFIX + p, g) == 0, (p, g)
    # ti_engine_generate_sampled at start_pos = prefix length: what the unregistered run of the full prompts bans
    conts = PROMPTS[:B]
    reg, _ = e.generate_sampled(conts, NEW, 1.0, 1, 1.0, HALF[:B], start_pos=[len(PREFIX)] * B)
    assert e.shared_prefix() == (len(PREFIX), B)
    for p, g in zip(conts, reg.tolist()):
        assert repeats(PREFIX + p, g) == 0, (p, g)
    e.close()
