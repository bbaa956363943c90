"""Repetition / presence / frequency penalties in the sampled device loop (ti_engine_set_penalties,
ti_engine_generate_sampled), on the MID model of tests/test_gpu_engine.py.

Host loop, exact (prefill off): the device loop against a twin engine's ti_engine_step logits -> the NumPy
restatement of the penalties over the context so far (tests/penalty_ref.py) -> the oracle's sampler with the same
draws.  The twin steps the same number of rows, so the logits are bit-equal (the method of
test_gpu_sample.py::test_engine_sampled_generate_matches_host_loop and
test_gpu_serve_sampled.py::test_requests_match_the_host_loop, whose bars apply: equal tokens, log-probabilities
within rtol = atol = 1e-5).  The draws are placed while the reference runs: a seeded choice among the survivors of
probability >= 2e-3, the fp32 midpoint of its cumulative interval, so every draw lies >= 1e-3 inside its token's
interval (asserted at 1e-4) where exp / log differences of an ulp move a boundary by 1e-6, and a build that
ignores the draws or the penalties fails.

Prefill on, property: a prompt and weight seed picked on the CPU oracle (as tools/margin_search.py does: seed 26,
jitter 0.1, 40 tokens).  The oracle's unpenalised greedy run of 16 tokens -- 511 775 993 287 583 589 287 722 287
90 723 287 874 287 157 680 -- repeats 5 times (511 is a prompt token, 287 returns four times), every top-2 margin
>= 1.3 % of max|logit|, six times the engine's logits tolerance.  With presence = 1e4 and top_k = 1 no token may
repeat and none may come from the prompt, whatever the rounding.  That needs the prompt's histogram on the prefill
route: a run that counts the generated tokens alone picks 511, 141 and 702 out of the prompt (oracle, same seed).

Neutral values are the parent's engine bit for bit; the entry points that cannot penalise refuse while active."""
from __future__ import annotations

import numpy as np
import pytest

import penalty_ref as R
from test_gpu_engine import MID, engine_for

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED, JIT = 9, 0.1
PEN = (1.3, 0.4, 0.2)
T, K, P = 0.8, 40, 0.9
PROMPTS3 = [[400], [5, 7, 5], [100, 200, 300, 100, 500, 200]]


def engine(ti, max_batch, seed=SEED, jit=JIT):
    e = engine_for(ti, MID, max_batch=max_batch)
    e.synth(seed, jit)
    return e


def host_loop(ti, oracle, prompts, new, top_k, pen, place_seed):
    """-> (draws [n][new], tokens, logprobs, the smallest distance of a draw to its interval's ends)."""
    n = len(prompts)
    ref = engine(ti, n)
    rng = np.random.RandomState(place_seed)
    gen = [[] for _ in prompts]
    lps = [[] for _ in prompts]
    draws = np.full((n, new), 0.5, f32)
    worst = np.inf
    for s in range(max(len(p) for p in prompts) + new - 1):
        row = []
        for m, p in enumerate(prompts):
            g = s - len(p)
            row.append(p[s] if s < len(p) else gen[m][g] if g < len(gen[m]) else 0)   # (0: a finished stream's filler)
        lg = ref.step(row, [s] * n)
        for m, p in enumerate(prompts):
            if s < len(p) - 1 or len(gen[m]) >= new:
                continue
            pl = R.penalize(lg[m], p + gen[m], *pen)      # the context so far: the prompt, every token fed
            t_i = len(gen[m])
            if top_k > 1:
                pr = oracle.sample_probs(pl, T, top_k, P)
                cum = np.concatenate(([f32(0)], np.cumsum(pr, dtype=f32)))
                big = np.flatnonzero(pr >= 2e-3)
                j = int(big[rng.randint(big.size)])
                u = f32((np.float64(cum[j]) + np.float64(cum[j + 1])) / 2)
                worst = min(worst, float(u) - float(cum[j]), float(cum[j + 1]) - float(u))
                draws[m, t_i] = u
            tok, lp = oracle.sample_token(pl, T, top_k, P, float(draws[m, t_i]))
            if top_k > 1:
                assert tok == j, "the placed draw picks its survivor"
            gen[m].append(tok)
            lps[m].append(lp)
    ref.close()
    return draws, gen, lps, worst


@pytest.mark.parametrize("top_k", [1, K])
@pytest.mark.parametrize("prompts", [[[3, 17, 99, 5, 17, 7]], PROMPTS3], ids=["one_stream", "three_streams"])
def test_generate_sampled_matches_the_host_loop(ti, oracle, prompts, top_k):
    new = 12
    draws, want, want_lp, worst = host_loop(ti, oracle, prompts, new, top_k, PEN, place_seed=7)
    plain = host_loop(ti, oracle, prompts, new, 1, (1.0, 0.0, 0.0), place_seed=7)[1]
    print(f"\nsmallest distance of a draw to its interval's ends: {worst:.3e}")
    assert worst >= 1e-4
    e = engine(ti, len(prompts))
    e.set_prefill(0)
    e.set_penalties(*PEN)
    assert e.penalties() == tuple(float(f32(x)) for x in PEN)
    got, got_lp = e.generate_sampled(prompts, new, T, top_k, P, draws)
    e.close()
    for m in range(len(prompts)):
        assert got[m].tolist() == want[m], f"stream {m}"
        np.testing.assert_allclose(got_lp[m], np.array(want_lp[m], f32), rtol=1e-5, atol=1e-5)
    if top_k == 1:     # the penalties act: the unpenalised greedy sequence is another one
        assert want != plain


PROP_SEED, PROP_JIT, PROP_NEW = 26, 0.1, 16
PROP_PROMPT = [970, 958, 144, 29, 511, 916, 141, 410, 979, 212, 447, 356, 609, 539, 515, 702, 69, 272, 701, 831, 143, 21,
               942, 990, 217, 137, 387, 255, 502, 774, 88, 76, 354, 910, 579, 364, 886, 391, 976, 396]


def repeats(prompt, new):
    seen, n = set(prompt), 0
    for t in new:
        n += t in seen
        seen.add(t)
    return n


def test_prefill_route_counts_the_prompt(ti):
    e = engine(ti, 1, PROP_SEED, PROP_JIT)
    plain = e.generate([PROP_PROMPT], PROP_NEW)[0].tolist()
    assert repeats(PROP_PROMPT, plain) >= 3, plain
    c0 = e.counters()
    e.set_penalties(1.0, 1e4, 0.0)
    got, _ = e.generate_sampled([PROP_PROMPT], PROP_NEW, 1.0, 1, 1.0, np.full((1, PROP_NEW), 0.5, f32))
    c1 = e.counters()
    e.close()
    assert c1[1] > c0[1], "the prompt ran as prompt chunks"
    got = got[0].tolist()
    assert len(set(got)) == PROP_NEW, got
    assert not set(got) & set(PROP_PROMPT), sorted(set(got) & set(PROP_PROMPT))


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
               for x, y in zip(a, b))


@pytest.mark.parametrize("prefill", [0, 16])
def test_neutral_is_the_parent(ti, prefill):
    new = 12
    draws = np.random.RandomState(3).uniform(0, 1, (3, new)).astype(f32)
    e = engine(ti, 3)
    e.set_prefill(prefill)
    assert e.penalties() == (1.0, 0.0, 0.0)
    never = e.generate_sampled(PROMPTS3, new, T, K, P, draws)
    e.set_penalties(1.0, 0.0, 0.0)
    neutral = e.generate_sampled(PROMPTS3, new, T, K, P, draws)
    e.set_penalties(1.0, 1e4, 0.0)
    active = e.generate_sampled(PROMPTS3, new, T, K, P, draws)
    e.set_penalties()
    after = e.generate_sampled(PROMPTS3, new, T, K, P, draws)
    greedy = e.generate(PROMPTS3, new)                # the refusal is gone with the penalties
    e.close()
    assert same(never, neutral) and same(never, after)
    assert greedy.shape == (3, new)
    for m, p in enumerate(PROMPTS3):                  # (and the active call was one)
        toks = active[0][m].tolist()
        assert len(set(toks)) == new and not set(toks) & set(p)


def test_refusals_while_active(ti):
    e = engine(ti, 3)
    e.set_penalties(1.1, 0.0, 0.0)
    c0 = e.counters()
    d = np.full(4, 0.5, f32)
    calls = {
        "ti_engine_generate": lambda: e.generate([[1, 2, 3]], 4),
        "ti_engine_serve": lambda: e.serve([[1, 2, 3], [4]], 4, eos=-1, chunk=4),
        "ti_engine_generate_lookahead": lambda: e.generate_lookahead([1, 2, 3], 4),
        "ti_engine_generate_lookahead_sampled": lambda: e.generate_lookahead_sampled([1, 2, 3], 4, T, K, P, d),
        "ti_engine_beam_search": lambda: e.beam_search([1, 2, 3], 4, 2),
    }
    for fn, call in calls.items():
        with pytest.raises(ti.TiError, match=f"ti error 3: {fn}:"):
            call()
    assert e.counters() == c0
    # ti_engine_step and ti_engine_score return the model's own numbers
    twin = engine(ti, 3)
    assert same([e.step([5, 6, 7], [0, 0, 0])], [twin.step([5, 6, 7], [0, 0, 0])])
    assert same([e.score([1, 2, 3, 4])], [twin.score([1, 2, 3, 4])])
    twin.close()
    for bad in ((0.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (float("nan"), 0.0, 0.0), (float("inf"), 0.0, 0.0),
                (1.0, float("inf"), 0.0), (1.0, 0.0, float("nan"))):
        with pytest.raises(ti.TiError, match="ti error 1: ti_engine_set_penalties"):
            e.set_penalties(*bad)
    assert e.penalties() == (float(f32(1.1)), 0.0, 0.0)
    e.close()


def test_compat_engine_is_unsupported(ti):
    e = ti.Engine(1000, 256, 1, 4, 4, 64, 1024, bits=16, max_seq=64, max_batch=1, compat=True)
    with pytest.raises(ti.TiError, match="ti error 3: ti_engine_set_penalties"):
        e.set_penalties(1.1, 0.0, 0.0)
    e.close()
