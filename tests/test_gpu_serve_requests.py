"""Continuous batching with per-request parameters (ti_engine_serve_requests): every request carries its own budget,
stop token, sampler values and penalties, and all of them share one loop, one batch and one step graph whose
launches behind the lm_head read each slot's values from a device table.

MID, max_batch 3, the 7 prompts of tests/test_gpu_serve.py, seeded draws [7][6].  The four parameter sets of SETS are
cycled over the requests, max_new over (6, 2, 5, 3), and requests 0 and 2 stop at a token of their own unconstrained
output.  The contract of ti_engine.h: request r equals, tokens and log p bit for bit, the uniform
ti_engine_serve_sampled run of r's own set (ti_engine_set_penalties set to r's three values) on a fresh engine of the
same shape, cut at r's max_new or stop -- whatever the other requests' values, the slot and the chunking.  The
four uniform runs are computed once (REF) and shared.  One-token prompts equal the host loop of
tests/test_gpu_serve_sampled.py::test_requests_match_the_host_loop with ti_penalize_logits and the oracle's sampler
taking each request's values, also on a vocab-8192 engine where one request's top_k = vocab puts the call on the
sampler's workspace instance."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import guide_ref as G
from test_gpu_engine import MID, engine_for
from test_gpu_serve import PROMPTS

pytestmark = pytest.mark.gpu

f32 = np.float32
V = MID["vocab"]
SEED, JIT, NEW, B = 9, 0.1, 6, 3
N = len(PROMPTS)
DRAWS = np.random.RandomState(11).uniform(0, 1, (N, NEW)).astype(f32)
# (temperature, top_k, top_p), (repetition, presence, frequency)
SETS = [((1.0, 1, 1.0), (1.0, 0.0, 0.0)),
        ((0.8, 40, 0.9), (1.0, 0.0, 0.0)),
        ((1.2, 200, 1.0), (1.3, 0.2, 0.1)),
        ((0.7, 1024, 0.5), (1.0, 0.5, 0.0))]
MAX_NEW = (6, 2, 5, 3)
STOPPERS = {0: 1, 2: 2}            # request -> index into its own unconstrained output of its stop token


def engine(ti, max_batch=B):
    e = engine_for(ti, MID, max_batch=max_batch)
    e.synth(SEED, JIT)
    return e


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def same(a, b):
    (ta, la), (tb, lb) = a, b
    return ta == tb and all(np.array_equal(bits(x), bits(y)) for x, y in zip(la, lb))


REF = {}


def ref(ti, s):
    """The uniform ti_engine_serve_sampled run of set s over all prompts on a fresh engine: NEW tokens, no stop."""
    if s not in REF:
        (T, k, p), pen = SETS[s]
        e = engine(ti)
        e.set_penalties(*pen)
        toks, lps = e.serve_sampled(PROMPTS, NEW, T, k, p, DRAWS, eos=-1, chunk=4)
        e.close()
        REF[s] = toks, [lp.copy() for lp in lps]
    return REF[s]


def params(ti, shift=0):
    """Request r: set (r + shift) % 4, max_new cycled, the two stoppers' tokens from their own set's run."""
    out = []
    for r in range(N):
        s = (r + shift) % len(SETS)
        (T, k, p), (rep, pres, freq) = SETS[s]
        stop = ref(ti, s)[0][r][STOPPERS[r]] if r in STOPPERS else -1
        out.append(dict(max_new=MAX_NEW[r % 4], stop_token=stop, temperature=T, top_k=k, top_p=p, repetition=rep,
                        presence=pres, frequency=freq))
    return out


def assert_contract(ti, got, prm, shift=0):
    toks, lps = got
    early = 0
    for r in range(N):
        want_t, want_lp = ref(ti, (r + shift) % len(SETS))
        n = prm[r]["max_new"]
        if prm[r]["stop_token"] in want_t[r][:n]:
            n = want_t[r].index(prm[r]["stop_token"]) + 1
            early += n < prm[r]["max_new"]
        assert toks[r] == want_t[r][:n], (r, toks[r], want_t[r])
        assert np.array_equal(bits(lps[r]), bits(want_lp[r][:n])), (r, lps[r], want_lp[r][:n])
    assert early == len(STOPPERS), "the stop tokens end their requests early"


def test_each_request_is_the_uniform_run_of_its_own_set(ti):
    prm = params(ti)
    e = engine(ti)
    got = {c: e.serve_requests(PROMPTS, prm, DRAWS, chunk=c) for c in (4, 1, 7)}
    assert_contract(ti, got[4], prm)
    assert same(got[4], got[1]) and same(got[4], got[7])               # chunking changes nothing
    # the sets rotated by one on the same engine, no setter in between: other values, the same graphs
    rot = params(ti, shift=1)
    assert_contract(ti, e.serve_requests(PROMPTS, rot, DRAWS, chunk=4), rot, shift=1)
    e.close()
    assert ref(ti, 1)[0] != ref(ti, 2)[0] and ref(ti, 0)[0] != ref(ti, 3)[0]     # (the sets do differ)


@pytest.mark.parametrize("s", [1, 2])
def test_all_requests_on_one_set_is_serve_sampled(ti, s):
    (T, k, p), (rep, pres, freq) = SETS[s]
    e = engine(ti)
    got = e.serve_requests(PROMPTS, [dict(max_new=NEW, temperature=T, top_k=k, top_p=p, repetition=rep, presence=pres,
                                          frequency=freq)] * N, DRAWS, chunk=4)
    e.close()
    assert same(got, ref(ti, s))


def host_loop(ti, oracle, ref_e, prompts, prm, draws, batch):
    """tests/test_gpu_serve_sampled.py's host loop with request r's own values: a twin engine's ti_engine_step logits
    -> ti_penalize_logits over prompt + new tokens -> the oracle's sampler."""
    want, want_lp = [], []
    for r, p in enumerate(prompts):
        q = prm[r]
        toks, lps = [], []
        for pos in range(q["max_new"]):
            lg = ref_e.step([(p + toks)[-1]] + [0] * (batch - 1), [pos] + [0] * (batch - 1))[0]
            pl = ti.penalize_logits(lg, p + toks, q["repetition"], q["presence"], q["frequency"])
            tok, lp = oracle.sample_token(pl, q["temperature"], q["top_k"], q["top_p"], float(draws[r, pos]))
            toks.append(tok)
            lps.append(lp)
        want.append(toks)
        want_lp.append(lps)
    return want, want_lp


def test_one_token_prompts_match_the_host_loop(ti, oracle):
    prompts = [[p[-1]] for p in PROMPTS]
    prm = [dict(q, stop_token=-1) for q in params(ti)]
    twin = engine(ti)
    want, want_lp = host_loop(ti, oracle, twin, prompts, prm, DRAWS, B)
    twin.close()
    e = engine(ti)
    got, got_lp = e.serve_requests(prompts, prm, DRAWS, chunk=4)
    e.close()
    for r in range(N):
        assert got[r] == want[r], f"request {r}"
        np.testing.assert_allclose(got_lp[r], np.array(want_lp[r], f32), rtol=1e-5, atol=1e-5)


def test_workspace_route_matches_the_host_loop(ti, oracle):
    """vocab 8192 (the mini_gqa shape, 2 layers): request 1 has top_k = vocab, above TI_SAMPLE_MAX_K, so every row of
    the call runs on the sampler's workspace instance."""
    v, new = 8192, 4

    def small():
        e = ti.Engine(v, 256, 2, 4, 2, 64, 512, bits=4, max_seq=128, max_batch=B)
        e.synth(0x7157, 0.1)
        return e
    prompts = [[3], [17], [99], [250]]
    prm = [dict(max_new=new, temperature=1.0, top_k=1),
           dict(max_new=new, temperature=0.9, top_k=v, top_p=0.95, repetition=1.2, presence=0.1, frequency=0.1),
           dict(max_new=3, temperature=0.8, top_k=40, top_p=0.9),
           dict(max_new=new, temperature=1.1, top_k=5000, top_p=1.0, presence=0.5)]
    prm = [dict(dict(stop_token=-1, top_p=1.0, repetition=1.0, presence=0.0, frequency=0.0), **q) for q in prm]
    draws = np.random.RandomState(12).uniform(0, 1, (len(prompts), new)).astype(f32)
    twin = small()
    want, want_lp = host_loop(ti, oracle, twin, prompts, prm, draws, B)
    twin.close()
    e = small()
    got, got_lp = e.serve_requests(prompts, prm, draws, chunk=3)
    e.close()
    for r in range(len(prompts)):
        assert got[r] == want[r], f"request {r}"
        np.testing.assert_allclose(got_lp[r], np.array(want_lp[r], f32), rtol=1e-5, atol=1e-5)


def test_the_engine_guide_applies_to_every_request(ti):
    """One-token prompts (no prefill: the twin's ti_engine_step logits are the first step's).  The greedy requests'
    favourites are banned: nobody emits a banned id, and the greedy requests open with their runner-up."""
    prompts = [[p[-1]] for p in PROMPTS]
    prm = [dict(q, stop_token=-1) for q in params(ti)]
    greedy = [r for r in range(N) if prm[r]["top_k"] == 1]
    assert len(greedy) == 2
    twin = engine(ti)
    order = {r: np.argsort(-twin.step([prompts[r][0]] + [0] * (B - 1), [0] * B)[0], kind="stable") for r in greedy}
    twin.close()
    banned = {int(order[r][0]) for r in greedy}
    e = engine(ti)
    plain, _ = e.serve_requests(prompts, prm, DRAWS, chunk=4)
    e.set_guide(*G.ban(V, banned).args)
    got, got_lp = e.serve_requests(prompts, prm, DRAWS, chunk=4)
    e.set_guide(None)
    again, _ = e.serve_requests(prompts, prm, DRAWS, chunk=4)
    e.close()
    assert again == plain
    for r in greedy:
        assert plain[r][0] == int(order[r][0])
        runner_up = int(order[r][1])
        assert runner_up not in banned
        assert got[r][0] == runner_up and got_lp[r][0] == 0.0, (r, got[r], order[r][:3])
    for r in range(N):
        assert len(got[r]) == prm[r]["max_new"] and not banned & set(got[r]), (r, got[r])


def test_engine_state_and_the_other_entry_points_are_untouched(ti):
    """ti_engine_set_penalties' values, ti_engine_serve_sampled's and ti_engine_serve's results, and the launch count
    of the greedy replay step are the same before and after a ti_engine_serve_requests call."""
    prm = params(ti)
    e = engine(ti)
    pen = (1.1, 0.4, 0.2)
    e.set_penalties(*pen)
    e.set_stop(5)
    before = e.serve_sampled(PROMPTS, NEW, 0.8, 40, 0.9, DRAWS, eos=-1, chunk=4)
    mixed = e.serve_requests(PROMPTS, prm, DRAWS, chunk=4)          # the engine-wide penalties do not apply
    assert_contract(ti, mixed, prm)
    assert e.penalties() == pytest.approx(pen)
    after = e.serve_sampled(PROMPTS, NEW, 0.8, 40, 0.9, DRAWS, eos=-1, chunk=4)
    assert same(before, after)
    e.close()
    e = engine(ti)
    greedy = e.serve(PROMPTS, NEW, eos=-1, chunk=4)
    e.replay_prepare(B, 8, 42)
    n0 = [(d["kind"], d["tag"], d["workgroups"]) for d in e.stamp_steps(2)]
    e.serve_requests(PROMPTS, prm, DRAWS, chunk=4)
    assert e.serve(PROMPTS, NEW, eos=-1, chunk=4) == greedy
    e.replay_prepare(B, 8, 42)
    n1 = [(d["kind"], d["tag"], d["workgroups"]) for d in e.stamp_steps(2)]
    e.close()
    assert len(n0) > 0 and n0 == n1


GOOD = dict(max_new=NEW, stop_token=-1, temperature=0.8, top_k=40, top_p=0.9, repetition=1.0, presence=0.0, frequency=0.0)
BAD = [dict(max_new=0), dict(max_new=NEW + 1), dict(stop_token=-2), dict(stop_token=V), dict(top_k=0), dict(top_k=V + 1),
       dict(repetition=0.0), dict(repetition=float("nan")), dict(repetition=float("inf")), dict(presence=float("inf")),
       dict(frequency=float("nan"))]


def test_argument_errors(ti):
    e = engine(ti)
    d0 = e.counters()
    err = "ti error 1: ti_engine_serve_requests"
    for bad in BAD:
        prm = [GOOD] * (N - 1) + [dict(GOOD, **bad)]
        with pytest.raises(ti.TiError, match=err + ".*request 6"):
            e.serve_requests(PROMPTS, prm, DRAWS, chunk=4)
    with pytest.raises(ti.TiError, match=err):
        e.serve_requests(PROMPTS, [GOOD] * N, DRAWS, chunk=0)
    with pytest.raises(ti.TiError, match=err + ".*request 1"):                # an empty prompt
        e.serve_requests([[1], [], [2]], [GOOD] * 3, DRAWS[:3], chunk=4)
    long = MID["max_seq"] - NEW + 2                                            # prompt + max_new - 1 = max_seq + 1
    with pytest.raises(ti.TiError, match=err + ".*request 0.*max_seq"):
        e.serve_requests([[7] * long], [GOOD], DRAWS[:1], chunk=4)
    # nulls (the wrapper cannot pass them)
    L = ti.lib()
    flat, offs = np.array([1, 2], np.int32), np.array([0, 1, 2], np.int32)
    out, ln, dr = np.zeros((2, NEW), np.int32), np.zeros(2, np.int32), np.zeros((2, NEW), f32)
    q = (ti.RequestParams * 2)(ti.RequestParams(**GOOD), ti.RequestParams(**GOOD))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    for args in [(e.h, 2, vp(flat), vp(offs), None, 4, vp(dr), NEW, vp(out), vp(ln), None),
                 (e.h, 2, vp(flat), vp(offs), q, 4, None, NEW, vp(out), vp(ln), None),
                 (e.h, 2, None, vp(offs), q, 4, vp(dr), NEW, vp(out), vp(ln), None),
                 (e.h, 2, vp(flat), vp(offs), q, 4, vp(dr), NEW, None, vp(ln), None),
                 (e.h, 0, vp(flat), vp(offs), q, 4, vp(dr), NEW, vp(out), vp(ln), None),
                 (e.h, 2, vp(flat), vp(offs), q, 4, vp(dr), 0, vp(out), vp(ln), None)]:
        assert L.ti_engine_serve_requests(*args) == 1
        assert b"ti_engine_serve_requests" in L.ti_last_error()
    assert e.counters() == d0
    # and the engine still serves
    toks, _ = e.serve_requests(PROMPTS, [GOOD] * N, DRAWS, chunk=4)
    assert [len(t) for t in toks] == [NEW] * N
    e.close()


def test_compat_engine_is_unsupported(ti):
    e = ti.Engine(1000, 256, 1, 4, 4, 64, 1024, bits=16, max_seq=64, max_batch=1, compat=True)
    with pytest.raises(ti.TiError, match="ti error 3: ti_engine_serve_requests"):
        e.serve_requests([[1, 2]], [dict(GOOD, max_new=2)], np.zeros((1, 2), f32), chunk=2)
    e.close()
