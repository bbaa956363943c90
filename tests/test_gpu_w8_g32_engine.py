"""A Q8_0 engine (bits 8 | BITS_G32) above 16 rows: prompt chunks and batched decode steps reach gemm_w8_kernel's
group-32 instance.  Weights are exact group-32 blocks, set through set_tensor_q and written into the oracle model
in place (as test_gpu_g32.py's engine tests do for int4)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_g32 import G32_CFG as CFG, g32_weight

pytestmark = pytest.mark.gpu


def build(ti, oracle, bits, max_batch, seed):   # (engine with bits | G32, oracle model) with the same weights
    from pyoracle import OracleModel, _OrModel
    V, H, NL, I = CFG["vocab"], CFG["hidden"], CFG["layers"], CFG["inter"]
    qd, kvd = CFG["heads"] * CFG["head_dim"], CFG["kv_heads"] * CFG["head_dim"]
    m = OracleModel(oracle, CFG, seed, 0.1)
    base, mm = m.weights(), C.cast(m.ptr, C.POINTER(_OrModel)).contents
    rng = np.random.RandomState(300 + bits)
    e = ti.Engine(V, H, NL, CFG["heads"], CFG["kv_heads"], CFG["head_dim"], I, bits=bits | ti.BITS_G32,
                  max_seq=CFG["max_seq"], max_batch=max_batch, rope_theta=CFG["rope_theta"], eps=CFG["eps"])
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
        q, d, w = g32_weight(rng, K, N, bits)
        e.set_tensor_q(slot, l, q, d)
        np.ctypeslib.as_array(ptr, shape=(K * N,))[:] = w.reshape(-1)   # the oracle's weight, in place
    return e, m


def test_prefill_vs_oracle(ti, oracle):
    """A 100-token prompt, then 3 greedy tokens: the oracle's tokens and last logits, in as many prompt chunks as an
    int4 group-32 engine takes (one; 16-row pieces take seven).  Seed 78: every reference margin is 40x the bar."""
    prompt, chunks = np.random.RandomState(31).randint(0, CFG["vocab"], size=100).tolist(), {}
    for bits in (4, 8):
        e, m = build(ti, oracle, bits, 1, 78)
        got, glg = e.generate([prompt], 3, want_logits=True)
        chunks[bits] = e.counters()[1]
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
    assert err <= bar and chunks[8] == chunks[4]


def test_batched_decode_vs_oracle(ti, oracle):   # 20 streams x 4 steps; test_engine_g32_batched_vs_oracle's bar
    from pyoracle import OracleModel
    B, (e, m0) = 20, build(ti, oracle, 8, 20, 81)
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
