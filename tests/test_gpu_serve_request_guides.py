"""Per-request guides in continuous batching (ti_engine_add_guide + ti_engine_serve_requests_guided): every request
names a guide of the engine's library by handle, or none, and all of them share one loop, one batch and one step graph
whose guide launch reads each slot's handle from the ti_row_params table.

MID, max_batch 3, the 7 prompts of tests/test_gpu_serve.py, the seeded draws, parameter sets and budgets of
tests/test_gpu_serve_requests.py (request r: set r mod 4, max_new cycled over (6, 2, 5, 3)); every request's
stop_token is STOP.  The library holds three guides (tests/guide_ref.py): a ban of every token the unguided run
produced (so a banned request is certain to differ from it), the forced chain, and digits_then_stop over STOP.
Request r's kind is (r + r // 4 + rot) mod 4 over (ban, forced, digits, none), so kinds and parameter sets meet in
different pairs.  The contract of ti_engine.h: request r equals, tokens and log p bit for bit, ti_engine_serve_requests
on a fresh engine of the same shape whose ti_engine_set_guide is r's guide (none for handle 0) -- whatever the other
requests' guides and values, the slot and the chunking.  The four uniform runs per engine shape are computed once
(REFS) and shared."""
from __future__ import annotations

import numpy as np
import pytest

import guide_ref as G
from test_gpu_engine import MID, engine_for
from test_gpu_serve import PROMPTS
from test_gpu_serve_requests import B, DRAWS, JIT, MAX_NEW, NEW, SEED, SETS, bits, same

pytestmark = pytest.mark.gpu

f32 = np.float32
V = MID["vocab"]
N = len(PROMPTS)
STOP = 2
DIGITS = list(range(48, 58))
KINDS = ("ban", "forced", "digits", None)
PREFIX = np.random.RandomState(77).randint(0, V, 40).tolist()


def engine(ti, max_batch=B, kv8=False, prefix=False):
    e = engine_for(ti, dict(MID, bits=MID["bits"] | (ti.BITS_KV8 if kv8 else 0)), max_batch=max_batch)
    e.synth(SEED, JIT)
    if prefix:
        e.share_prefix(PREFIX, max_batch)
    return e


def prm_for(n=N):
    out = []
    for r in range(n):
        (T, k, p), (rep, pres, freq) = SETS[r % len(SETS)]
        out.append(dict(max_new=MAX_NEW[r % 4], stop_token=STOP, temperature=T, top_k=k, top_p=p, repetition=rep,
                        presence=pres, frequency=freq))
    return out


PRM = prm_for()
REFS: dict = {}
GUIDES: dict = {}


def uniform_run(ti, shape, kind):
    """ti_engine_serve_requests over all requests on a fresh engine of `shape` (a tuple of engine() keywords set to
    True) under ti_engine_set_guide(kind's guide); kind None: no guide set."""
    e = engine(ti, **{k: True for k in shape})
    if kind:
        e.set_guide(*guide(ti, kind).args)
    toks, lps = e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4)
    e.close()
    return toks, [lp.copy() for lp in lps]


def refs(ti, shape=()):
    """{kind: (tokens, log p)}: the four uniform runs of an engine shape."""
    if shape not in REFS:
        REFS[shape] = {kind: uniform_run(ti, shape, kind) for kind in KINDS}
    return REFS[shape]


def guide(ti, kind) -> G.Guide:
    if kind not in GUIDES:
        if kind == "ban":                                        # every token of the unguided run of the plain shape
            GUIDES[kind] = G.ban(V, {t for toks in uniform_run(ti, (), None)[0] for t in toks})
        else:
            GUIDES[kind] = G.forced(V) if kind == "forced" else G.digits_then_stop(DIGITS, STOP)
    return GUIDES[kind]


def library(ti, e):
    """The three guides join e's library -> {kind: handle}."""
    h = {kind: e.add_guide(*guide(ti, kind).args) for kind in KINDS[:3]}
    assert h == {"ban": 1, "forced": 2, "digits": 3} and e.guide_count() == 3
    h[None] = 0
    return h


def kind_of(r, rot=0):
    return KINDS[(r + r // 4 + rot) % 4]


def handles(h, rot=0, n=N):
    return [h[kind_of(r, rot)] for r in range(n)]


def assert_contract(ti, got, rot=0, shape=()):
    toks, lps = got
    want = refs(ti, shape)
    for r in range(N):
        want_t, want_lp = want[kind_of(r, rot)]
        assert toks[r] == want_t[r], (r, kind_of(r, rot), toks[r], want_t[r])
        assert np.array_equal(bits(lps[r]), bits(want_lp[r])), (r, kind_of(r, rot), lps[r], want_lp[r])


def test_each_request_is_the_run_under_its_own_guide(ti):
    e = engine(ti)
    h = library(ti, e)
    got = {c: e.serve_requests(PROMPTS, PRM, DRAWS, chunk=c, guides=handles(h)) for c in (4, 1, 7)}
    assert_contract(ti, got[4])
    assert same(got[4], got[1]) and same(got[4], got[7])               # chunking changes nothing
    # the handles rotated by one on the same engine: other guides in every slot, the same graphs
    steps0, graphs0 = e.counters(), e.graph_counters()
    rot = e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=handles(h, 1))
    assert e.graph_counters() == graphs0 and e.counters()[0] > steps0[0]
    assert_contract(ti, rot, rot=1)
    e.close()
    # the guides did constrain: a banned request differs from the unguided run in its first token, a forced one walks
    # the chain, a digits one emits digits and may end with STOP
    plain = refs(ti)[None][0]
    banned = set(np.flatnonzero(~np.isin(np.arange(V), guide(ti, "ban").allowed(0))).tolist())
    seen = {k: 0 for k in KINDS}
    for toks, r_ in ((got[4][0], 0), (rot[0], 1)):
        for r in range(N):
            k = kind_of(r, r_)
            seen[k] += 1
            if k == "ban":
                assert plain[r][0] in banned and toks[r][0] != plain[r][0] and not banned & set(toks[r]), (r, toks[r])
            elif k == "forced":
                assert toks[r] == G.FORCED[:PRM[r]["max_new"]], (r, toks[r])
            elif k == "digits":
                body = toks[r][:-1] if toks[r][-1] == STOP else toks[r]
                assert set(body) <= set(DIGITS) and G.run(guide(ti, k), toks[r])[1], (r, toks[r])
            else:
                assert toks[r] == plain[r], r
    assert min(seen.values()) >= 3


def test_adding_and_removing_guides_drops_no_graph(ti):
    e = engine(ti)
    h1 = e.add_guide(*guide(ti, "ban").args)
    assert h1 == 1 and e.guide_count() == 1
    only_ban = [h1 if kind_of(r) == "ban" else 0 for r in range(N)]
    first = e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=only_ban)
    want = refs(ti)
    for r in range(N):
        assert first[0][r] == want["ban" if only_ban[r] else None][0][r], r
    graphs0 = e.graph_counters()
    assert graphs0[0] >= 1
    assert e.add_guide(*guide(ti, "forced").args) == 2 and e.add_guide(*guide(ti, "digits").args) == 3
    spare = e.add_guide(*G.cycle(V, 3).args)
    assert spare == 4 and e.guide_count() == 4
    assert e.graph_counters() == graphs0                                # add: no graph dropped
    h = {"ban": 1, "forced": 2, "digits": 3, None: 0}
    assert_contract(ti, e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=handles(h)))
    assert e.graph_counters() == graphs0                                # the new guides run on the graphs of the first call
    e.remove_guide(spare)                                               # never named by a request
    assert e.guide_count() == 3 and e.graph_counters() == graphs0
    assert_contract(ti, e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=handles(h)))
    assert e.graph_counters() == graphs0
    steps0 = e.counters()
    with pytest.raises(ti.TiError, match="ti error 1: ti_engine_serve_requests_guided.*request 6.*not live"):
        e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=[0] * 6 + [spare])
    with pytest.raises(ti.TiError, match="ti error 1: ti_engine_remove_guide"):
        e.remove_guide(spare)
    assert e.counters() == steps0 and e.graph_counters() == graphs0
    assert e.add_guide(*G.cycle(V, 3).args) == spare                    # the lowest free handle
    e.remove_guide(0)                                                   # all of them
    assert e.guide_count() == 0 and e.graph_counters() == graphs0
    with pytest.raises(ti.TiError, match="ti error 1: ti_engine_serve_requests_guided.*request 0.*not live"):
        e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=[1] * N)
    plain = e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=[0] * N)
    assert same(plain, want[None])
    e.close()


def test_one_token_prompts_match_the_host_loop(ti, oracle):
    """No prefill runs.  The host loop of tests/test_gpu_serve_requests.py with the request's own guide between the
    penalties and the sampler: a twin engine's ti_engine_step logits -> ti_penalize_logits over prompt + new tokens
    -> ti_guide_apply (it consumes the token the step fed) -> the oracle's sampler with the request's draws."""
    prompts = [[p[-1]] for p in PROMPTS]
    twin = engine(ti)
    want, want_lp = [], []
    for r, p in enumerate(prompts):
        q, kind = PRM[r], kind_of(r)
        toks, lps, s = [], [], 0
        for pos in range(q["max_new"]):
            lg = twin.step([(p + toks)[-1]] + [0] * (B - 1), [pos] + [0] * (B - 1))[0]
            pl = ti.penalize_logits(lg, p + toks, q["repetition"], q["presence"], q["frequency"])
            if kind:
                g = guide(ti, kind)
                s, pl = ti.guide_apply(g.csr, s if toks else g.start, toks[-1] if toks else -1, pl)
            tok, lp = oracle.sample_token(pl, q["temperature"], q["top_k"], q["top_p"], float(DRAWS[r, pos]))
            toks.append(tok)
            lps.append(lp)
            if tok == STOP:
                break
        want.append(toks)
        want_lp.append(lps)
    twin.close()
    e = engine(ti)
    h = library(ti, e)
    got, got_lp = e.serve_requests(prompts, PRM, DRAWS, chunk=4, guides=handles(h))
    e.close()
    for r in range(N):
        assert got[r] == want[r], f"request {r} ({kind_of(r)})"
        np.testing.assert_allclose(got_lp[r], np.array(want_lp[r], f32), rtol=1e-5, atol=1e-5)


def test_under_a_registered_shared_prefix(ti, monkeypatch):
    monkeypatch.setenv("TI_SHARE_MIN", "1")
    e = engine(ti, prefix=True)
    h = library(ti, e)
    got = e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=handles(h))
    assert e.shared_prefix() == (len(PREFIX), B)
    e.close()
    assert_contract(ti, got, shape=("prefix",))
    assert refs(ti, ("prefix",))[None][0] != refs(ti)[None][0]          # (the prefix is attended)


def test_on_an_e4m3_kv_cache(ti):
    e = engine(ti, kv8=True)
    h = library(ti, e)
    got = e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=handles(h))
    e.close()
    assert_contract(ti, got, shape=("kv8",))


def stamped(e):
    e.replay_prepare(B, 8, 42)
    return [(d["kind"], d["tag"], d["workgroups"]) for d in e.stamp_steps(2)]


def other_entry_points(ti, e):
    """What the entry points that know nothing of the library return."""
    out = {}
    out["generate"] = e.generate(PROMPTS[:B], NEW).tolist()
    out["serve"] = e.serve(PROMPTS, NEW, eos=-1, chunk=4)
    out["lookahead"] = e.generate_lookahead(PROMPTS[4], NEW)[0].tolist()
    out["lookahead_sampled"] = [x.tolist() for x in e.generate_lookahead_sampled(PROMPTS[4], NEW, 0.8, 40, 0.9, DRAWS[4])[:2]]
    out["beam"] = e.beam_search(PROMPTS[0], 4, 2)
    t, lp = e.generate_sampled(PROMPTS[:B], NEW, 0.8, 40, 0.9, DRAWS[:B])
    out["generate_sampled"] = t.tolist(), bits(lp).tolist()
    t, lp = e.serve_sampled(PROMPTS, NEW, 0.8, 40, 0.9, DRAWS, eos=-1, chunk=4)
    out["serve_sampled"] = t, [bits(x).tolist() for x in lp]
    return out


def test_the_library_is_inert_until_a_request_names_a_handle(ti):
    bare = engine(ti)
    base = bare.serve_requests(PROMPTS, PRM, DRAWS, chunk=4)
    base_others = other_entry_points(ti, bare)
    base_stamps = stamped(bare)
    bare.close()
    assert same(base, refs(ti)[None]) and len(base_stamps) > 0
    e = engine(ti)
    library(ti, e)
    assert same(e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4), base)                        # guides=None: the old entry point
    graphs0 = e.graph_counters()
    assert same(e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=[0] * N), base)        # every handle 0
    assert e.graph_counters() == graphs0                                                     # ... on the same graphs
    assert e.guide_states().tolist() == [-1] * B
    assert other_entry_points(ti, e) == base_others                                          # none of them refuses
    assert stamped(e) == base_stamps
    e.close()


def test_guide_states_after_a_call(ti):
    """max_batch = 3 requests of 4 tokens in one chunk of 4 steps, no stop: slot m is request m and its last step
    masked with the state behind all but its last token; a slot whose request has no guide reads -1, also when the
    slot's previous request had one."""
    prompts = PROMPTS[:B]
    prm = [dict(q, max_new=4, stop_token=-1) for q in PRM[:B]]
    e = engine(ti)
    h = library(ti, e)
    toks, _ = e.serve_requests(prompts, prm, DRAWS[:B, :4], chunk=4, guides=[0, h["forced"], 0])
    st = e.guide_states().tolist()
    assert st[0] == st[2] == -1 and st[1] == G.run(guide(ti, "forced"), toks[1][:-1])[0][-1] == 3
    toks, _ = e.serve_requests(prompts, prm, DRAWS[:B, :4], chunk=4, guides=[h["forced"], 0, h["digits"]])
    st = e.guide_states().tolist()
    assert st[1] == -1
    assert st[0] == 3 and st[2] == G.run(guide(ti, "digits"), toks[2][:-1])[0][-1] >= 0
    e.close()


def test_argument_errors(ti):
    e = engine(ti)
    h = library(ti, e)
    e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=handles(h))
    steps0, graphs0 = e.counters(), e.graph_counters()
    err = "ti error 1: ti_engine_serve_requests_guided"
    for bad in (-1, ti.GUIDE_CAP + 1, 4, ti.GUIDE_CAP):                 # out of range; in range and not live
        with pytest.raises(ti.TiError, match=err + ".*request 5"):
            e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=[1, 2, 3, 0, 1] + [bad, 0])
    with pytest.raises(ti.TiError, match=err + ".*request 6"):          # ti_engine_serve_requests' own checks hold
        e.serve_requests(PROMPTS, PRM[:6] + [dict(PRM[6], top_k=0)], DRAWS, chunk=4, guides=handles(h))
    with pytest.raises(ti.TiError, match="ti error 1: ti_guide_check"):
        e.add_guide([0, 1], [V], [0])                                   # a token outside the vocabulary
    assert e.guide_count() == 3
    assert e.counters() == steps0 and e.graph_counters() == graphs0
    # one source of constraint per call
    e.set_guide(*guide(ti, "forced").args)
    steps0, graphs0 = e.counters(), e.graph_counters()
    with pytest.raises(ti.TiError, match="ti error 3: ti_engine_serve_requests_guided.*ti_engine_add_guide.*ti_engine_set_guide"):
        e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=handles(h))
    assert e.counters() == steps0 and e.graph_counters() == graphs0
    under = e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=[0] * N)   # no handle named: the engine's guide
    assert same(under, refs(ti)["forced"])
    e.set_guide(None)
    assert_contract(ti, e.serve_requests(PROMPTS, PRM, DRAWS, chunk=4, guides=handles(h)))
    e.close()


def test_compat_engine_is_unsupported(ti):
    e = ti.Engine(1000, 256, 1, 4, 4, 64, 1024, bits=16, max_seq=64, max_batch=1, compat=True)
    with pytest.raises(ti.TiError, match="ti error 3: ti_engine_add_guide"):
        e.add_guide(*G.ban(1000, {5}).args)
    with pytest.raises(ti.TiError, match="ti error 3: ti_engine_serve_requests_guided"):
        e.serve_requests([[1, 2]], [dict(PRM[0], max_new=2)], np.zeros((1, 2), f32), chunk=2, guides=[0])
    assert e.guide_count() == 0
    e.close()
