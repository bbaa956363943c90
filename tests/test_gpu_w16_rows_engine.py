"""An fp16-weight engine (bits 16) above 16 rows (gemm_w16_kernel under prompt chunks and batched decode steps)
against the oracle, on the MID8 shape with the bars of test_gpu_engine.py.  The oracle model's linear weights are
rounded to fp16 and written back, the engine gets the same values through set_tensor (fp16 values pack exactly).

Reference margins, checked on the oracle alone: seed 13 jitter 0.1 RandomState(3), 70 tokens: all 8 greedy steps
wide (the narrowest 2.6 x the 3 TOL rule); seed 17, 20 streams with the 4-token prompts RandomState(100 + b):
8 of the 160 steps narrow (cap 40), at most 2 in one stream."""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_engine import TOL, assert_greedy, assert_logits_close, engine_for, margin
from test_gpu_score import MID8

pytestmark = pytest.mark.gpu

CFG, JIT = dict(MID8, bits=16), 0.1
TOKS = np.random.RandomState(3).randint(0, CFG["vocab"], size=70).astype(np.int32)
SLOTS = {"attention.q_proj.weight": "W_Q", "attention.k_proj.weight": "W_K", "attention.v_proj.weight": "W_V",
         "attention.o_proj.weight": "W_O", "feed_forward.w3.weight": "W_GATE", "feed_forward.w1.weight": "W_UP",
         "feed_forward.w2.weight": "W_DOWN", "attention_norm.weight": "V_ATTN_NORM", "ffn_norm.weight": "V_FFN_NORM"}


def fp16_weights(oracle, seed):
    """The synthetic MID8 model's tensors with every matrix rounded to fp16."""
    from pyoracle import OracleModel
    return {k: v.astype(np.float16).astype(np.float32) if v.ndim == 2 else v
            for k, v in OracleModel(oracle, MID8, seed, JIT).weights().items()}


def oracle_run(oracle, w, prompt, n_new):
    """Greedy tokens and logits of n_new steps after the prompt, on an oracle model holding w."""
    from pyoracle import OracleModel
    m = OracleModel(oracle, MID8, 1, JIT)
    m.set_weights(w)
    for tok in prompt[:-1]:
        m.step(tok)
    out, logits = [prompt[-1]], []
    for _ in range(n_new):
        t, lg = m.step(out[-1])
        out.append(t)
        logits.append(lg)
    return out[1:], logits


def engine_with(ti, w, max_batch=1):
    e = engine_for(ti, CFG, max_batch=max_batch)
    e.set_tensor(ti.E_EMBED, 0, w["token_embeddings.weight"])
    e.set_tensor(ti.V_OUT_NORM, 0, w["norm.weight"])
    e.set_tensor(ti.W_LM_HEAD, 0, w["lm_head.weight"])
    for l in range(CFG["layers"]):
        for k, slot in SLOTS.items():
            e.set_tensor(getattr(ti, slot), l, w[f"layers.{l}.{k}"])
    return e


def test_prompt_70_then_8_greedy_steps(ti, oracle):
    w = fp16_weights(oracle, 13)
    ref, ref_logits = oracle_run(oracle, w, TOKS.tolist(), 8)
    e = engine_with(ti, w)
    e.set_prefill(64)   # (refused while fp16 weights ran 16-row pieces: rows > the largest chunk)
    got, lg = e.generate([TOKS.tolist()], 8, want_logits=True)
    e.close()
    assert_greedy(got[0].tolist(), ref, ref_logits, "70-token prompt")
    assert_logits_close(lg[0], ref_logits[-1])


def test_20_streams_8_steps(ti, oracle):
    """Teacher-forced with the oracle's tokens: every stream's logits at each of the 8 steps, and its argmax
    wherever the reference margin is wide."""
    B, P, S = 20, 4, 8
    w = fp16_weights(oracle, 17)
    prompts = [np.random.RandomState(100 + b).randint(0, CFG["vocab"], size=P).tolist() for b in range(B)]
    refs = [oracle_run(oracle, w, p, S + 1) for p in prompts]   # step s's input: token s - 1
    e = engine_with(ti, w, max_batch=B)
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
