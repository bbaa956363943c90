"""Token-automaton guided decoding in the sampled device loop (ti_engine_set_guide, ti_engine_generate_sampled), on
the MID model of tests/test_gpu_engine.py, with the four automata of tests/guide_ref.py.

Forced path: six one-transition states, then a free one -- the six tokens come out whatever the draws, for one
stream and for four of different prompt lengths (prefill on: the shortest prompt's rows run as prompt chunks).
Cycle (state i allows the ids = i mod 3): the device loop equals the host loop of tests/test_gpu_penalty_engine.py
-- a twin engine's ti_engine_step logits -> tests/penalty_ref.py (when penalties are on) -> guide_ref.mask in the
state guide_ref.advance gives -> the oracle's sampler with draws placed mid-interval -- token for token,
log-probabilities within that file's rtol = atol = 1e-5.
Ban: prompt and weight seed picked on the CPU oracle (the method of tools/margin_search.py: seed 25, jitter 0.1, the
six tokens of RandomState(25)): the oracle's first token is 888, its runner-up 884 leads the third logit by 10 % of
max|logit| (and trails the first by 12 %), asserted above 6 * TOL; one state that omits 888 makes top_k = 1 emit 884.
Digits then stop runs with ti_engine_set_stop; refusals, clearing and ti_engine_guide_states close the file."""
from __future__ import annotations

import numpy as np
import pytest

import guide_ref as G
import penalty_ref as R
from test_gpu_engine import MID, TOL, engine_for

pytestmark = pytest.mark.gpu

f32 = np.float32
V = MID["vocab"]
SEED, JIT = 9, 0.1
T, K, P = 0.8, 40, 0.9
OFF = (1.0, 0.0, 0.0)
PEN = (1.3, 0.4, 0.2)
PROMPTS3 = [[400], [5, 7, 5], [100, 200, 300, 100, 500, 200]]
PROMPTS4 = [[400], [5, 7, 5], [100, 200, 300, 100, 500, 200], [9, 8]]


def engine(ti, max_batch, seed=SEED, jit=JIT):
    e = engine_for(ti, MID, max_batch=max_batch)
    e.synth(seed, jit)
    return e


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
               for x, y in zip(a, b))


@pytest.mark.parametrize("prompts", [[[3, 17, 99, 5, 17, 7]], PROMPTS4], ids=["one_stream", "four_streams"])
def test_forced_path_whatever_the_draws(ti, prompts):
    new, n = 10, len(prompts)
    g = G.forced(V)
    e = engine(ti, n)
    e.set_guide(*g.args)
    for seed in (1, 2):
        draws = np.random.RandomState(seed).uniform(1e-6, 1, (n, new)).astype(f32)
        got, lp = e.generate_sampled(prompts, new, T, K, P, draws)
        for m in range(n):
            assert got[m, :6].tolist() == G.FORCED, (seed, m, got[m].tolist())
            assert np.all(lp[m, :6] == 0.0), "a forced token has probability 1"
            assert np.all(np.isfinite(lp[m])) and np.all((got[m] >= 0) & (got[m] < V))
    e.close()


def host_loop(ti, oracle, prompts, new, top_k, pen, g, place_seed):
    """-> (draws [n][new], tokens, logprobs, the state each stream's last token was drawn in, the smallest distance
    of a draw to its interval's ends)."""
    n = len(prompts)
    ref = engine(ti, n)
    rng = np.random.RandomState(place_seed)
    gen = [[] for _ in prompts]
    lps = [[] for _ in prompts]
    state = [g.start] * n
    draws = np.full((n, new), 0.5, f32)
    worst = np.inf
    for s in range(max(len(p) for p in prompts) + new - 1):
        row = []
        for m, p in enumerate(prompts):
            i = s - len(p)
            row.append(p[s] if s < len(p) else gen[m][i] if i < len(gen[m]) else 0)   # (0: a finished stream's filler)
        lg = ref.step(row, [s] * n)
        for m, p in enumerate(prompts):
            if s < len(p) - 1 or len(gen[m]) >= new:
                continue
            pl = R.penalize(lg[m], p + gen[m], *pen) if pen != OFF else lg[m]
            if gen[m]:
                state[m] = G.advance(g, state[m], gen[m][-1])     # the token this step fed
            pl = G.mask(g, state[m], pl)
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
    return draws, gen, lps, state, worst


@pytest.mark.parametrize("pen", [OFF, PEN], ids=["guide", "penalties_then_guide"])
@pytest.mark.parametrize("top_k", [1, K])
@pytest.mark.parametrize("prompts", [[[3, 17, 99, 5, 17, 7]], PROMPTS3], ids=["one_stream", "three_streams"])
def test_cycle_matches_the_host_loop(ti, oracle, prompts, top_k, pen):
    new = 12
    g = G.cycle(V, 3)
    draws, want, want_lp, _, worst = host_loop(ti, oracle, prompts, new, top_k, pen, g, place_seed=7)
    print(f"\nsmallest distance of a draw to its interval's ends: {worst:.3e}")
    assert worst >= 1e-4
    e = engine(ti, len(prompts))
    e.set_prefill(0)
    if top_k == 1:                                   # (either order of activation: the two share the carry row)
        e.set_guide(*g.args)
        e.set_penalties(*pen)
    else:
        e.set_penalties(*pen)
        e.set_guide(*g.args)
    got, got_lp = e.generate_sampled(prompts, new, T, top_k, P, draws)
    e.close()
    for m in range(len(prompts)):
        assert G.run(g, want[m])[1] and G.run(g, got[m].tolist())[1], f"stream {m}: not accepted"
        assert got[m].tolist() == want[m], f"stream {m}"
        np.testing.assert_allclose(got_lp[m], np.array(want_lp[m], f32), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("prefill", [0, 16])
def test_cycle_is_accepted_and_states_are_the_restatements(ti, prefill):
    """Equal prompt lengths: every stream runs exactly `new` sampled steps, so a slot ends in the state its last
    token was drawn in (the step consumed every token but that one)."""
    new, prompts = 9, [[1, 2, 3], [400, 401, 402], [7, 7, 7]]
    g = G.cycle(V, 3)
    e = engine(ti, 4)
    e.set_prefill(prefill)
    assert e.guide_states().tolist() == [-1] * 4
    e.set_guide(*g.args)
    assert e.guide_states().tolist() == [-1] * 4
    draws = np.random.RandomState(5).uniform(1e-6, 1, (3, new)).astype(f32)
    got, lp = e.generate_sampled(prompts, new, T, K, P, draws)
    st = e.guide_states()
    e.close()
    for m in range(3):
        states, ok = G.run(g, got[m].tolist())
        assert ok, (m, got[m].tolist())
        assert [int(t) % 3 for t in got[m]] == [i % 3 for i in range(new)]
        assert int(st[m]) == states[new - 1] == (new - 1) % 3
        assert np.all(np.isfinite(lp[m])) and np.all(lp[m] <= 0.0)
    assert int(st[3]) == -1, "a slot no request ran in stays free"


BAN_SEED, BAN_JIT = 25, 0.1
BAN_PROMPT = np.random.RandomState(BAN_SEED).randint(0, V, 6).tolist()


def test_ban_gives_the_runner_up(ti, oracle):
    from pyoracle import OracleModel
    m = OracleModel(oracle, MID, BAN_SEED, BAN_JIT)
    for tok in BAN_PROMPT:
        _, lg = m.step(tok)
    m.close()
    order = np.argsort(lg)[::-1]
    first, second, third = (int(x) for x in order[:3])
    mx = float(np.max(np.abs(lg)))
    m12, m23 = float(lg[first] - lg[second]), float(lg[second] - lg[third])
    print(f"\noracle top-3 {first} {second} {third}: margins {m12 / mx:.4f} {m23 / mx:.4f} of max|logit|")
    assert m12 > 6 * TOL * mx and m23 > 6 * TOL * mx, "re-pick the seed"
    half = np.full((1, 1), 0.5, f32)
    for prefill in (0, 16):
        e = engine(ti, 1, BAN_SEED, BAN_JIT)
        e.set_prefill(prefill)
        assert e.generate_sampled([BAN_PROMPT], 1, 1.0, 1, 1.0, half)[0][0, 0] == first
        g = G.ban(V, [first])
        e.set_guide(*g.args)
        tok, lp = e.generate_sampled([BAN_PROMPT], 1, 1.0, 1, 1.0, half)
        assert tok[0, 0] == second, prefill
        e.set_guide(*G.ban(V, [first, second]).args)
        assert e.generate_sampled([BAN_PROMPT], 1, 1.0, 1, 1.0, half)[0][0, 0] == third
        e.close()


def test_digits_then_stop(ti):
    """Streams 0 and 1 take a draw of 1e-9 at their second / fourth token: the first survivor that kept probability,
    which in the state that allows it is the stop token (the lowest allowed id; top_p = 1, top_k = 40 >= 11 keeps
    every allowed id).  Stream 2 draws 0.999 throughout.  Lock-step: the stopped streams go on stepping, in the
    state that allows only the stop token."""
    stop, digits, new = 2, list(range(100, 110)), 12
    g = G.digits_then_stop(digits, stop)
    draws = np.full((3, new), 0.5, f32)
    draws[0, 1] = draws[1, 3] = 1e-9
    draws[2, :] = 0.999
    e = engine(ti, 3)
    e.set_guide(*g.args)
    e.set_stop(stop)
    got, lp = e.generate_sampled(PROMPTS3, new, 1.0, K, 1.0, draws)
    e.close()
    ends = []
    for m in range(3):
        toks = got[m].tolist()
        end = toks.index(stop) + 1 if stop in toks else new
        ends.append(end)
        assert G.run(g, toks[:end])[1], (m, toks)
        assert all(t in digits for t in toks[: end - 1]) and toks[0] in digits, (m, toks)
        assert toks[end:] == [-1] * (new - end), (m, toks)
    assert ends[0] == 2 and ends[1] <= 4 and got[1, ends[1] - 1] == stop, got.tolist()
    assert ends[2] == new and stop not in got[2].tolist()


def test_refusals_and_clearing(ti):
    new = 8
    draws = np.random.RandomState(3).uniform(1e-6, 1, (3, new)).astype(f32)
    e = engine(ti, 3)
    never = e.generate_sampled(PROMPTS3, new, T, K, P, draws)
    e.set_guide(*G.cycle(V, 3).args)
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
    guided = e.generate_sampled(PROMPTS3, new, T, K, P, draws)
    assert not same(never, guided)
    bad = G.cycle(V, 3)
    bad.tokens = bad.tokens[::-1].copy()
    with pytest.raises(ti.TiError, match="ti error 1: ti_guide_check"):
        e.set_guide(*bad.args)
    with pytest.raises(ti.TiError, match="ti error 1: ti_guide_check"):
        e.set_guide(*G.cycle(V + 1, 3).args)               # an id outside the engine's vocabulary
    assert same(guided, e.generate_sampled(PROMPTS3, new, T, K, P, draws)), "a refused guide leaves the live one"
    e.set_guide(None)
    assert e.guide_states().tolist() == [-1] * 3
    assert same(never, e.generate_sampled(PROMPTS3, new, T, K, P, draws))
    assert e.generate(PROMPTS3, new).shape == (3, new)     # the refusal is gone with the guide
    e.close()


def test_kv8_engine_takes_a_guide(ti):
    g = G.forced(V)
    e = ti.Engine(V, MID["hidden"], MID["layers"], MID["heads"], MID["kv_heads"], MID["head_dim"], MID["inter"],
                  bits=MID["bits"] | ti.BITS_KV8, max_seq=MID["max_seq"], max_batch=2)
    e.synth(SEED, JIT)
    e.set_guide(*g.args)
    draws = np.random.RandomState(8).uniform(1e-6, 1, (2, 8)).astype(f32)
    got, _ = e.generate_sampled([[1, 2, 3], [4]], 8, T, K, P, draws)
    e.close()
    assert got[0, :6].tolist() == G.FORCED and got[1, :6].tolist() == G.FORCED


def test_compat_engine_is_unsupported(ti):
    e = ti.Engine(1000, 256, 1, 4, 4, 64, 1024, bits=16, max_seq=64, max_batch=1, compat=True)
    with pytest.raises(ti.TiError, match="ti error 3: ti_engine_set_guide"):
        e.set_guide(*G.cycle(1000, 3).args)
    e.close()
