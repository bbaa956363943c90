"""A Q4_1 engine (bits 4 | BITS_G32 | BITS_AFF) above 16 rows: prompt chunks and batched decode steps reach
gemm_w4a_kernel.  Weights are exact Q4_1 blocks, set through set_tensor_q1 and written dequantized into the oracle
model in place (as test_gpu_g32.py's engine tests do)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_g32 import G32_CFG as CFG, g32_weight, q1_weight

pytestmark = pytest.mark.gpu


def build(ti, oracle, aff, max_batch, seed):   # (engine: Q4_1 if aff else int4 group-32, oracle model), same weights
    from pyoracle import OracleModel, _OrModel
    V, H, NL, I = CFG["vocab"], CFG["hidden"], CFG["layers"], CFG["inter"]
    qd, kvd = CFG["heads"] * CFG["head_dim"], CFG["kv_heads"] * CFG["head_dim"]
    m = OracleModel(oracle, CFG, seed, 0.1)
    base, mm = m.weights(), C.cast(m.ptr, C.POINTER(_OrModel)).contents
    rng = np.random.RandomState(300 + aff)
    e = ti.Engine(V, H, NL, CFG["heads"], CFG["kv_heads"], CFG["head_dim"], I,
                  bits=4 | ti.BITS_G32 | (ti.BITS_AFF if aff else 0), max_seq=CFG["max_seq"], max_batch=max_batch,
                  rope_theta=CFG["rope_theta"], eps=CFG["eps"])
    e.set_tensor(ti.E_EMBED, 0, base["token_embeddings.weight"])
    e.set_tensor(ti.V_OUT_NORM, 0, base["norm.weight"])
    linears = [(ti.W_LM_HEAD, 0, mm.lm_head, H, V)]
    for l in range(NL):
        e.set_tensor(ti.V_ATTN_NORM, l, base[f"layers.{l}.attention_norm.weight"])
        e.set_tensor(ti.V_FFN_NORM, l, base[f"layers.{l}.ffn_norm.weight"])
        linears += [(ti.W_Q, l, mm.wq[l], H, qd), (ti.W_K, l, mm.wk[l], H, kvd), (ti.W_V, l, mm.wv[l], H, kvd),
                    (ti.W_O, l, mm.wo[l], qd, H), (ti.W_GATE, l, mm.wg[l], H, I), (ti.W_UP, l, mm.wu[l], H, I),
                    (ti.W_DOWN, l, mm.wd[l], I, H)]
    for slot, l, ptr, K, N in linears:
        if aff:
            q, d, mn, w, _ = q1_weight(rng, K, N)
            e.set_tensor_q1(slot, l, q, d, mn)
        else:
            q, d, w = g32_weight(rng, K, N, 4)
            e.set_tensor_q(slot, l, q, d)
        np.ctypeslib.as_array(ptr, shape=(K * N,))[:] = w.reshape(-1)   # the oracle's weight, in place
    return e, m


def test_prefill_vs_oracle(ti, oracle):
    """A 100-token prompt, then 3 greedy tokens: the oracle's tokens and last logits, in as many prompt chunks as an
    int4 group-32 engine takes (one; 16-row pieces take seven)."""
    prompt, chunks = np.random.RandomState(31).randint(0, CFG["vocab"], size=100).tolist(), {}
    e4, m4 = build(ti, oracle, 0, 1, 78)
    e4.generate([prompt], 1)
    chunks[0] = e4.counters()[1]
    e4.close(), m4.close()
    e, m = build(ti, oracle, 1, 1, 78)
    got, glg = e.generate([prompt], 3, want_logits=True)
    chunks[1] = e.counters()[1]
    e.close()
    for t in prompt:
        tok, lg = m.step(t)
    for ref in got[0].tolist():
        s, bar, last = np.sort(lg), 2e-3 * float(np.max(np.abs(lg))), lg
        assert s[-1] - s[-2] > 3 * bar, "reference margin too small"
        assert ref == tok
        tok, lg = m.step(tok)
    err = float(np.max(np.abs(glg[0].astype(np.float64) - last)))
    print(f"prompt chunks {chunks}, last logits off by {err:.3e} (bar {bar:.3e})")
    assert err <= bar and chunks[1] == chunks[0]


def test_batched_decode_vs_oracle(ti, oracle):   # 20 streams x 4 steps; test_engine_g32_batched_vs_oracle's bar
    from pyoracle import OracleModel
    B, (e, m0) = 20, build(ti, oracle, 1, 20, 81)
    models, weights = [m0] + [OracleModel(oracle, CFG, 81, 0.1) for _ in range(B - 1)], m0.weights()
    for m in models[1:]:
        m.set_weights(weights)
    e.set_prefill(0)
    toks, worst = [int(t) for t in np.random.RandomState(9).randint(0, CFG["vocab"], size=B)], 0.0
    for pos in range(4):
        lg = e.step(toks, [pos] * B)
        for i, m in enumerate(models):
            toks[i], ref_lg = m.step(toks[i])
            worst = max(worst, float(np.max(np.abs(lg[i].astype(np.float64) - ref_lg))) / float(np.max(np.abs(ref_lg))))
    e.close()
    print(f"worst relative logit error {worst:.3e}")
    assert worst <= 5e-3, worst
