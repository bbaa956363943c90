"""ti_engine_score (teacher-forced scoring on the device; InferenceEngine::compute_logprobs,
inference_engine.cpp:873-954) against the oracle.

Reference: OracleModel.step logits at every position, log-softmax in float64.

Bar per position i: |lp - lp_ref| <= 2 * TOL * max|ref_logits_i|.  The project's logits bar is
TOL * max|ref| (test_gpu_engine.py); log-sum-exp is 1-Lipschitz in the sup norm, and the picked logit
moves by at most the same amount.  It comes to 0.011 .. 0.019 for log-probabilities of -5 .. -10 here.

out_top1 equals the oracle's argmax at every position whose reference top-2 margin exceeds
3 * TOL * max|ref|; at most 10 % of a sequence's positions may be excused (asserted; on the reference
alone 68/70 positions are wide for MID seed 13 jitter 0.1 RandomState(3), 37/40 for MID8 with the same
seeds, 284/300 for MID seed 21 RandomState(9)).

Each oracle sequence is computed once per session (_ref_logits) and never modified."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from test_gpu_engine import MID, TOL, _oracle_tokens, assert_greedy, assert_logits_close, engine_for

pytestmark = pytest.mark.gpu

MID8 = dict(MID, kv_heads=4, head_dim=128, heads=4, bits=8)
SEQS = {   # name: (cfg, seed, jitter, RandomState seed, tokens)
    "mid70": (MID, 13, 0.1, 3, 70),
    "mid8_40": (MID8, 13, 0.1, 3, 40),
    "mid300": (MID, 21, 0.1, 9, 300),
}
_cache: dict = {}


def _ref_logits(oracle, name):
    """(tokens int32 [n], oracle logits float64 [n][vocab]) of SEQS[name]."""
    if name not in _cache:
        from pyoracle import OracleModel
        cfg, seed, jit, rs, n = SEQS[name]
        toks = np.random.RandomState(rs).randint(0, cfg["vocab"], size=n).astype(np.int32)
        m = OracleModel(oracle, cfg, seed, jit)
        lg = np.stack([np.asarray(m.step(int(t))[1], np.float64) for t in toks])
        m.close()
        lg.setflags(write=False)
        toks.setflags(write=False)
        _cache[name] = (toks, lg)
    return _cache[name]


def _engine(ti, name, **kw):
    cfg, seed, jit, _, _ = SEQS[name]
    e = engine_for(ti, cfg, **kw)
    e.synth(seed, jit)
    return e


def next_targets(toks):
    return np.concatenate([toks[1:], [-1]]).astype(np.int32)


def assert_logprobs(lp, ref, targets, what=""):
    mx = np.max(np.abs(ref), axis=1)
    top = ref.max(axis=1)
    lse = top + np.log(np.exp(ref - top[:, None]).sum(axis=1))
    worst = 0.0
    for i, t in enumerate(targets):
        if t < 0:
            assert lp[i] == 0.0, f"{what} position {i}: no target, got {lp[i]}"
            continue
        err, bar = abs(float(lp[i]) - (ref[i, t] - lse[i])), 2 * TOL * mx[i]
        worst = max(worst, err / bar)
        assert err <= bar, f"{what} position {i}: |lp - lp_ref| {err:.4g} > {bar:.4g} (lp {lp[i]:.5g})"
    print(f"{what}: worst |lp - lp_ref| / bar = {worst:.3f} over {len(targets)} positions")


def assert_top1(top1, ref, what=""):
    s = np.sort(ref, axis=1)
    wide = (s[:, -1] - s[:, -2]) > 3 * TOL * np.max(np.abs(ref), axis=1)
    excused = int((~wide).sum())
    assert excused <= 0.1 * len(ref), f"{what}: {excused} of {len(ref)} reference margins are narrow (re-pick the seed)"
    am = np.argmax(ref, axis=1)
    bad = [i for i in np.flatnonzero(wide) if top1[i] != am[i]]
    assert not bad, f"{what}: top1 differs from the oracle's argmax at positions {bad}"


@pytest.mark.parametrize("name,rows,chunks", [("mid70", 32, 3), ("mid8_40", None, 3), ("mid300", None, 1)],
                         ids=["gqa8_w4_32+32+6", "mha_hd128_w8_16+16+8", "tile_300_rows_128+128+44"])
def test_score_vs_oracle(ti, oracle, name, rows, chunks):
    """Next-token targets (-1 last), then targets = NULL (= tokens), both against the oracle; every
    call is `chunks` prefill chunks and no decode step.  mid300 is one 300-row chunk on the tile GEMM
    and the MFMA attention, its lm_head split 128 + 128 + 44 (TI_SCORE_ROWS): an offset bug shows at
    rows 127 / 128 and 255 / 256."""
    toks, ref = _ref_logits(oracle, name)
    e = _engine(ti, name)
    if rows:
        e.set_prefill(rows)
    mem, c0 = e.memory(), e.counters()
    tg = next_targets(toks)
    lp, top1 = e.score(toks, tg, want_top1=True)
    c1 = e.counters()
    lp_self = e.score(toks)
    c2 = e.counters()
    assert e.memory() == mem
    e.close()
    assert_logprobs(lp, ref, tg, f"{name} next-token")
    assert_top1(top1, ref, name)
    assert_logprobs(lp_self, ref, toks, f"{name} targets=None")
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (0, chunks) and (c2[0] - c1[0], c2[1] - c1[1]) == (0, chunks), (c0, c1, c2)


def test_score_prefill_off_uses_rows_path(ti, oracle):
    """set_prefill(0): scoring still runs as prompt chunks (the chunk ti_engine_serve uses), never decode steps."""
    toks, ref = _ref_logits(oracle, "mid70")
    e = _engine(ti, "mid70")
    e.set_prefill(0)
    c0 = e.counters()
    lp = e.score(toks)
    c1 = e.counters()
    e.close()
    assert_logprobs(lp, ref, toks, "prefill off")
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (0, 1)


def test_score_continues_from_start_pos(ti, oracle):
    """score(tokens[:40]) then score(tokens[40:], start_pos=40): all 70 positions meet the bar."""
    toks, ref = _ref_logits(oracle, "mid70")
    tg = next_targets(toks)
    e = _engine(ti, "mid70")
    e.set_prefill(32)
    a = e.score(toks[:40], tg[:40], want_top1=True)
    b = e.score(toks[40:], tg[40:], start_pos=40, want_top1=True)
    e.close()
    assert_logprobs(np.concatenate([a[0], b[0]]), ref, tg, "40 + 30")
    assert_top1(np.concatenate([a[1], b[1]]), ref, "40 + 30")


def test_generate_continues_after_score(ti, oracle):
    """The KV rows a score call leaves are a prefill's: the setup of
    test_gpu_prefill.py::test_prefill_start_pos_and_cache_contents (100 synthetic cache slots, its 37-token
    prompt, whose 3 greedy steps have wide reference margins -- assert_greedy checks them anyway; the same
    prompt from an empty cache has a narrow margin at its second step), with all but the prompt's last
    token scored instead of prefilled: generate from the last token at position 136 gives the oracle's
    greedy tokens."""
    seed, jit, kv_seed, fill = 5, 0.1, 77, 100
    prompt = np.random.RandomState(7).randint(0, MID["vocab"], size=37).tolist()
    ref, ref_logits = _oracle_tokens(oracle, MID, seed, jit, prompt, 3, fill, kv_seed)
    e = engine_for(ti, MID)
    e.synth(seed, jit)
    e.fill_kv(0, fill, kv_seed)
    e.score(prompt[:36], start_pos=fill)
    got = e.generate([[prompt[36]]], 3, start_pos=[fill + 36])
    e.close()
    assert_greedy(got[0].tolist(), ref, ref_logits)


def test_score_stream_slots_are_independent(ti, oracle):
    """max_batch = 2: scoring in slot 1 meets the bar, and a score in slot 0 in between does not disturb
    slot 1's continuation."""
    toks, ref = _ref_logits(oracle, "mid70")
    tg = next_targets(toks)
    e = _engine(ti, "mid70", max_batch=2)
    a = e.score(toks[:40], tg[:40], stream=1)
    other = e.score(toks[::-1].copy(), stream=0)
    b = e.score(toks[40:], tg[40:], stream=1, start_pos=40)
    e.close()
    assert np.all(np.isfinite(other)) and np.all(other < 0)
    assert_logprobs(np.concatenate([a, b]), ref, tg, "slot 1")


def test_score_between_generates_changes_nothing(ti, oracle):
    """generate, score, generate on one engine: the same tokens both times, and last logits within the
    logits bar of each other (no graph or step buffer clobbered; the 20 scored tokens fit the token
    buffer the first generate sized, so its captured step graphs are the ones replayed), and
    ti_engine_memory reports what it did before the first score call."""
    toks, _ = _ref_logits(oracle, "mid70")
    e = _engine(ti, "mid70")
    mem = e.memory()
    g1, l1 = e.generate([toks[:20].tolist()], 6, want_logits=True)
    e.score(toks[20:40])
    g2, l2 = e.generate([toks[:20].tolist()], 6, want_logits=True)
    assert e.memory() == mem
    e.close()
    assert g1.tolist() == g2.tolist()
    assert_logits_close(l2[0], l1[0].astype(np.float64))


def test_score_argument_errors(ti):
    """Every error returns non-zero with ti_engine_score in the message, before anything is enqueued."""
    L = ti.lib()
    e = engine_for(ti, MID, max_batch=2)
    V, S = MID["vocab"], MID["max_seq"]
    tok = np.arange(8, dtype=np.int32)
    lp, top1 = np.zeros(S + 1, np.float32), np.zeros(S + 1, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    c0 = e.counters()

    def bad(h, stream, tokens, n, start, targets, out, code=1):
        rc = L.ti_engine_score(h, stream, p(tokens), n, start, p(targets), p(out), p(top1))
        assert rc == code, (rc, code)
        assert b"ti_engine_score" in L.ti_last_error(), L.ti_last_error()

    bad(None, 0, tok, 8, 0, None, lp)
    bad(e.h, 0, None, 8, 0, None, lp)
    bad(e.h, 0, tok, 8, 0, None, None)
    bad(e.h, 0, tok, 0, 0, None, lp)
    bad(e.h, -1, tok, 8, 0, None, lp)
    bad(e.h, 2, tok, 8, 0, None, lp)
    bad(e.h, 0, tok, 8, -1, None, lp)
    bad(e.h, 0, tok, 8, S - 7, None, lp)
    bad(e.h, 0, np.zeros(S + 1, np.int32), S + 1, 0, None, lp)
    for t in (-1, V):
        bad(e.h, 0, np.array([1, 2, t, 3], np.int32), 4, 0, np.zeros(4, np.int32), lp)
    for t in (-2, V):
        bad(e.h, 0, tok, 8, 0, np.array([0, 0, 0, t, 0, 0, 0, 0], np.int32), lp)
    assert e.counters() == c0
    e.close()
    c = ti.Engine(1000, 256, 2, 4, 4, 64, 1024, bits=16, max_seq=64, max_batch=1, compat=True)
    bad(c.h, 0, tok, 8, 0, None, lp, code=3)
    c.close()
