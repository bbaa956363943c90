"""ti_engine_share_prefix: a prompt prefix prefilled once into slot 0, copied to the other slots and attended once per
step for all streams (ti_attn_decode_shared), against the oracle's greedy decode of the FULL prompts.

Four streams: a 40-token prefix plus four continuations of 3, 4, 5 and 6 tokens, 16 new tokens each, jitter 0.1.
Prefix, continuations and seeds searched on the CPU oracle (tools/margin_search.py's method) so that every one of
the 4 x 16 steps has a top-2 margin above 6 * TOL = 1.2e-2 of max|logit| (asserted below, no step is skipped); the
smallest margin per continuation, as a fraction of max|logit|:
  MID (GQA 8, head_dim 64)   seed 108   1.78e-2  2.22e-2  1.77e-2  1.52e-2
  MHA (4 / 4, head_dim 128)  seed 214   1.64e-2  2.41e-2  1.92e-2  1.40e-2
The 20-stream runs (int4, the packed route of the batched step, three splits of the prefix) give stream i
continuation i % 4.  Streams of one call step together until the longest continuation has its tokens, so a shorter
one runs on past its 16th token, where the oracle's margins are not pinned (some are below 1e-2): its last logits
are compared in a call whose max_new makes token 16 its last (check_streams).
Every engine here is created under TI_SHARE_MIN=1, so the 40-token prefix takes the shared attention.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_engine import MID, TOL, _oracle_tokens, engine_for, margin

pytestmark = pytest.mark.gpu

MHA = dict(MID, heads=4, kv_heads=4, head_dim=128)
JIT, N_NEW = 0.1, 16
MODELS = {
    "MID": (MID, 108,
            [100, 792, 146, 460, 367, 855, 595, 117, 307, 1002, 566, 391, 375, 862, 394, 877, 322, 1011, 5, 359, 24, 127,
             849, 77, 989, 440, 393, 688, 959, 380, 339, 935, 132, 595, 244, 456, 830, 984, 424, 15],
            [[982, 40, 592], [475, 449, 884, 836], [314, 857, 809, 719, 216], [213, 917, 840, 29, 574, 374]]),
    "MHA": (MHA, 214,
            [118, 706, 610, 119, 504, 624, 127, 480, 887, 489, 533, 927, 728, 804, 311, 432, 581, 249, 923, 419, 368, 58,
             885, 182, 650, 956, 2, 196, 471, 675, 527, 934, 584, 918, 102, 888, 952, 216, 150, 323],
            [[780, 379, 161], [900, 697, 11, 216], [846, 934, 378, 355, 44], [654, 134, 815, 520, 63, 76]]),
}
P = 40
_REF: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    mp = pytest.MonkeyPatch()
    mp.setenv("TI_SHARE_MIN", "1")
    yield
    mp.undo()
    _REF.clear()


def reference(oracle, name):
    """Per continuation the oracle's 16 greedy tokens and logits of prefix + continuation, once for the module."""
    if name not in _REF:
        cfg, seed, prefix, conts = MODELS[name]
        assert len(prefix) == P
        _REF[name] = [_oracle_tokens(oracle, cfg, seed, JIT, prefix + c, N_NEW) for c in conts]
    return _REF[name]


def make_engine(ti, name, max_batch=4, bits=None, compat=False):
    cfg, seed, _, _ = MODELS[name]
    if compat:   # (the plumbing model of test_gpu_score.py: no KV cache)
        return ti.Engine(1000, 256, 2, 4, 4, 64, 1024, bits=16, max_seq=64, max_batch=1, compat=True)
    e = engine_for(ti, dict(cfg, bits=bits or cfg["bits"]), max_batch=max_batch)
    e.synth(seed, JIT)
    return e


def assert_greedy6(got, ref, ref_logits, what):
    """assert_greedy of test_gpu_engine.py with this module's wider margin: 6 * TOL of max|logit| at every step."""
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        m, mx = margin(ref_logits[i]), float(np.max(np.abs(ref_logits[i])))
        assert m > 6 * TOL * mx, f"{what} step {i}: reference margin {m:.4g} <= 6 * TOL * {mx:.4g} (re-pick the prompts)"
        assert g == r, f"{what} token {i}: gpu {g} ref {r} (margin {m})"


def assert_last_logits(got, ref_logits, what):
    tol = TOL * float(np.max(np.abs(ref_logits[-1])))
    err = float(np.max(np.abs(got.astype(np.float64) - ref_logits[-1])))
    assert err <= tol, f"{what}: last logits off by {err} > {tol}"


def check_streams(ti, e, name, refs, n, what):
    """generate and generate_sampled (top_k 1) of n continuations at start_pos P against the oracle."""
    conts = [MODELS[name][3][i % 4] for i in range(n)]
    # The streams step together until the longest continuation (6 tokens) has its max_new tokens, so a stream of
    # L prompt tokens runs 6 - L steps more and its last logits are those of new token max_new + 6 - L.  The
    # oracle's margins are pinned for 16 tokens: the call with max_new = 10 + L leaves the logits of token 16 for
    # the streams of L prompt tokens, and the call with 16 gives every stream's 16 tokens.
    longest = max(len(c) for c in conts)
    for L in sorted({len(c) for c in conts}):
        new = N_NEW - (longest - L)
        got, lg = e.generate(conts, new, start_pos=[P] * n, want_logits=True)
        for i in range(n):
            ref, ref_logits = refs[i % 4]
            assert_greedy6(got[i].tolist(), ref[:new], ref_logits[:new], f"{what} generate({new}) stream {i}")
            if len(conts[i]) == L:
                assert_last_logits(lg[i], ref_logits, f"{what} generate({new}) stream {i}")
    assert got.shape == (n, N_NEW)
    assert e.shared_prefix() == (P, e.cfg.max_batch), "generate at start_pos P must keep the registration"
    draws = np.full((n, N_NEW), 0.5, np.float32)
    toks, lps = e.generate_sampled(conts, N_NEW, 1.0, 1, 1.0, draws, start_pos=[P] * n)
    # the log-probabilities an unregistered engine reports for the full prompts
    plain = make_engine(ti, name, max_batch=n)
    _, want_lps = plain.generate_sampled([MODELS[name][2] + c for c in conts], N_NEW, 1.0, 1, 1.0, draws)
    plain.close()
    for i in range(n):
        ref, ref_logits = refs[i % 4]
        assert_greedy6(toks[i].tolist(), ref, ref_logits, f"{what} generate_sampled stream {i}")
        tol = 2 * TOL * max(float(np.max(np.abs(z))) for z in ref_logits)
        assert np.all(np.isfinite(lps[i])) and np.max(np.abs(lps[i] - want_lps[i])) <= tol, \
            f"{what} stream {i}: log-probabilities {lps[i]} vs the unregistered engine's {want_lps[i]}"
    return got


@pytest.mark.parametrize("name", list(MODELS))
def test_four_streams_after_share_prefix(ti, oracle, name):
    refs = reference(oracle, name)
    cfg, _, prefix, _ = MODELS[name]
    e = make_engine(ti, name)
    assert e.shared_prefix() == (0, 0)
    steps0, chunks0 = e.counters()
    e.share_prefix(prefix, 4)
    assert e.shared_prefix() == (P, 4)
    assert e.counters() == (steps0, chunks0 + 1), "the prefix is one prompt chunk, counted once"
    e.share_prefix(prefix, 4)                               # the live registration again: nothing moves
    assert e.counters() == (steps0, chunks0 + 1) and e.shared_prefix() == (P, 4)
    for layer in range(cfg["layers"]):
        for which in (0, 1):
            row0 = e.read_kv(layer, 0, which, 0, P).view(np.uint16)
            assert np.any(row0), "slot 0's prefix rows were never written"
            for slot in (1, 2, 3):
                assert np.array_equal(e.read_kv(layer, slot, which, 0, P).view(np.uint16), row0), \
                    f"layer {layer} {'KV'[which]}: slot {slot} differs from slot 0"
    check_streams(ti, e, name, refs, 4, name)
    # two and three streams of the four take the shared route too (M <= n_streams)
    got = e.generate(MODELS[name][3][:2], N_NEW, start_pos=[P, P])
    for i in range(2):
        assert_greedy6(got[i].tolist(), refs[i][0], refs[i][1], f"{name} two streams, stream {i}")
    # a batched step at the positions behind the continuation
    cont = MODELS[name][3][0]
    lg = e.step([cont[0]] * 4, [P] * 4)
    assert e.shared_prefix() == (P, 4)
    assert np.all(np.isfinite(lg)) and np.max(np.abs(lg - lg[0])) <= TOL * float(np.max(np.abs(lg[0]))), \
        "four streams feeding one token behind one prefix must agree"
    e.close()


def test_twenty_streams_int4_packed_route(ti, oracle, monkeypatch):
    monkeypatch.setenv("TI_SHARE_SPLITS", "3")              # (the engine's own choice for 40 keys is one split)
    refs = reference(oracle, "MID")
    e = make_engine(ti, "MID", max_batch=20, bits=4)
    e.share_prefix(MODELS["MID"][2], 20)
    assert e.shared_prefix() == (P, 20)
    check_streams(ti, e, "MID", refs, 20, "MID x20")
    e.close()


def test_writes_below_the_prefix_clear_the_registration(ti, oracle):
    refs = reference(oracle, "MID")
    _, _, prefix, conts = MODELS["MID"]
    e = make_engine(ti, "MID")
    e.share_prefix(prefix, 4)
    # start_pos 0: the registration goes, the plain result stays
    got, lg = e.generate([prefix + c for c in conts], N_NEW, want_logits=True)
    assert e.shared_prefix() == (0, 0)
    for i in range(4):
        assert_greedy6(got[i].tolist(), refs[i][0], refs[i][1], f"plain stream {i}")
    assert_last_logits(lg[3], refs[3][1], "plain stream 3")     # (the longest prompt: its last step is token 16's)
    e.share_prefix(prefix, 4)
    e.fill_kv(1, 8, 77)
    assert e.shared_prefix() == (0, 0), "fill_kv"
    e.share_prefix(prefix, 4)
    e.beam_search(prefix[:4], 2, 2)
    assert e.shared_prefix() == (0, 0), "beam_search"
    e.share_prefix(prefix, 4)
    e.step([1, 2], [P, 3])
    assert e.shared_prefix() == (0, 0), "step below the prefix"
    e.share_prefix(prefix, 4)
    e.score(prefix[:4], stream=2, start_pos=P - 2)
    assert e.shared_prefix() == (0, 0), "score below the prefix"
    e.share_prefix(prefix, 4)
    e.score(prefix[:4], stream=2, start_pos=P)
    assert e.shared_prefix() == (P, 4), "score behind the prefix"
    e.share_prefix([], 4)                                   # n == 0 clears
    assert e.shared_prefix() == (0, 0)
    # after all that the registered route still gives the oracle's tokens
    e.share_prefix(prefix, 4)
    got = e.generate(conts, N_NEW, start_pos=[P] * 4)
    for i in range(4):
        assert_greedy6(got[i].tolist(), refs[i][0], refs[i][1], f"re-registered stream {i}")
    e.close()


def test_argument_errors_and_unsupported_engines(ti):
    e = make_engine(ti, "MID")
    prefix = MODELS["MID"][2]
    c0 = e.counters()
    for toks, n in ((prefix, 1), (prefix, 5), (prefix[:3] + [1024], 4), (prefix[:3] + [-1], 4), ([1] * 512, 4)):
        with pytest.raises(ti.TiError, match="ti error 1: ti_engine_share_prefix"):
            e.share_prefix(toks, n)
    assert e.counters() == c0 and e.shared_prefix() == (0, 0)
    e.close()
    e = make_engine(ti, "MID", bits=4 | ti.BITS_KV8)
    with pytest.raises(ti.TiError, match="ti error 3: ti_engine_share_prefix"):
        e.share_prefix(prefix, 4)
    e.close()
    e = make_engine(ti, "MID", compat=True)
    with pytest.raises(ti.TiError, match="ti error 3: ti_engine_share_prefix"):
        e.share_prefix(prefix, 4)
    e.close()


@pytest.mark.parametrize("name", list(MODELS))
def test_serve_continuations_behind_the_prefix(ti, oracle, name):
    """10 requests through 4 slots; `eos` is continuation 0's third token, so its requests end early."""
    refs = reference(oracle, name)
    _, _, prefix, conts = MODELS[name]
    reqs = [conts[i % 4] for i in range(10)]
    eos = refs[0][0][2]
    plain = make_engine(ti, name)
    want = plain.serve([prefix + r for r in reqs], N_NEW, eos=eos, chunk=4)
    draws = np.full((10, N_NEW), 0.5, np.float32)
    want_s, want_lp = plain.serve_sampled([prefix + r for r in reqs], N_NEW, 1.0, 1, 1.0, draws, eos=eos, chunk=4)
    assert plain.shared_prefix() == (0, 0)
    plain.close()
    assert min(len(w) for w in want) == 3 and max(len(w) for w in want) > 3
    for i, w in enumerate(want):                            # (the unregistered serve itself gives the oracle's tokens)
        assert w == refs[i % 4][0][:len(w)], f"request {i}"
    e = make_engine(ti, name)
    e.share_prefix(prefix, 4)
    chunks0 = e.counters()[1]
    got = e.serve(reqs, N_NEW, eos=eos, chunk=4)
    assert got == want
    assert e.shared_prefix() == (P, 4), "serve keeps a registration of max_batch streams"
    assert e.counters()[1] - chunks0 == 10, "one chunk per request: its continuation, never the prefix"
    got_s, got_lp = e.serve_sampled(reqs, N_NEW, 1.0, 1, 1.0, draws, eos=eos, chunk=4)
    assert got_s == want_s == want
    for i in range(10):
        mx = max(float(np.max(np.abs(lg))) for lg in refs[i % 4][1])
        assert np.max(np.abs(got_lp[i] - want_lp[i])) <= 2 * TOL * mx, f"request {i}: log-probabilities"
    # slot 0's prefix rows still feed every slot: the copies are as share_prefix left them
    for slot in (1, 2, 3):
        assert np.array_equal(e.read_kv(0, slot, 0, 0, P).view(np.uint16), e.read_kv(0, 0, 0, 0, P).view(np.uint16))
    e.close()
    # a registration of fewer streams than max_batch: serve clears it and serves full prompts as ever
    e = make_engine(ti, name, max_batch=5)
    e.share_prefix(prefix, 4)
    got = e.serve([prefix + r for r in reqs[:5]], N_NEW, eos=eos, chunk=4)
    assert e.shared_prefix() == (0, 0) and got == want[:5]
    e.close()
