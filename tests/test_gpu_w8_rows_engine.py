"""INT8 engines above 16 rows (gemm_w8_kernel under prompt chunks, batched decode steps and scoring) against the
oracle, on MID8 with the bars of test_gpu_engine.py / test_gpu_score.py.  The tests hold on either route
(TI_GEMM_W8_ROWS=0: 16-row fused pieces); they check the function, not the kernel.

Reference margins, checked on the oracle alone: seed 13 jitter 0.1 RandomState(3), 70 tokens: all 8 greedy steps
wide (the narrowest 2.6 x the 3 TOL rule); seed 17, 20 streams with the 4-token prompts RandomState(100 + b):
10 of the 160 steps narrow, at most 3 in one stream."""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_engine import TOL, _oracle_tokens, assert_greedy, assert_logits_close, engine_for, margin
from test_gpu_score import MID8, assert_logprobs

pytestmark = pytest.mark.gpu

SEED, JIT = 13, 0.1
TOKS = np.random.RandomState(3).randint(0, MID8["vocab"], size=70).astype(np.int32)


def test_prompt_70_then_8_greedy_steps(ti, oracle):
    ref, ref_logits = _oracle_tokens(oracle, MID8, SEED, JIT, TOKS.tolist(), 8)
    e = engine_for(ti, MID8)
    e.synth(SEED, JIT)
    got, lg = e.generate([TOKS.tolist()], 8, want_logits=True)
    e.close()
    assert_greedy(got[0].tolist(), ref, ref_logits, "70-token prompt")
    assert_logits_close(lg[0], ref_logits[-1])


def test_20_streams_8_steps(ti, oracle):
    """Teacher-forced with the oracle's tokens: every stream's logits at each of the 8 steps, and its argmax
    wherever the reference margin is wide."""
    B, P, S, seed = 20, 4, 8, 17
    prompts = [np.random.RandomState(100 + b).randint(0, MID8["vocab"], size=P).tolist() for b in range(B)]
    refs = [_oracle_tokens(oracle, MID8, seed, JIT, p, S + 1) for p in prompts]   # step s's input: token s - 1
    e = engine_for(ti, MID8, max_batch=B)
    e.synth(seed, JIT)
    for t in range(P - 1):
        e.step([p[t] for p in prompts], [t] * B)
    feed, narrow = [p[P - 1] for p in prompts], 0
    for s in range(S):
        lg = e.step(feed, [P - 1 + s] * B)
        for b, (toks, lgs) in enumerate(refs):
            assert_logits_close(lg[b], lgs[s])
            if margin(lgs[s]) > 3 * TOL * float(np.max(np.abs(lgs[s]))):
                assert int(np.argmax(lg[b])) == toks[s], f"stream {b} step {s}"
            else:
                narrow += 1
        feed = [toks[s] for toks, _ in refs]
    e.close()
    assert narrow <= B * S // 4, f"{narrow} of {B * S} reference margins are narrow (re-pick the seed)"


def test_score_70_tokens(ti, oracle):
    from pyoracle import OracleModel
    m = OracleModel(oracle, MID8, SEED, JIT)
    ref = np.stack([np.asarray(m.step(int(t))[1], np.float64) for t in TOKS])
    m.close()
    e = engine_for(ti, MID8)
    e.synth(SEED, JIT)
    lp = e.score(TOKS)
    e.close()
    assert_logprobs(lp, ref, TOKS, "mid8 70 tokens")
