"""An MXFP4 engine (bits 4 | BITS_G32 | BITS_MX) on test_gpu_engine.py's GQA model MID: every linear weight is exact
MX blocks uploaded through set_tensor_mx and written dequantized into the oracle model in place.  Logits within
that file's TOL (2e-3 max|logit|), tokens equal wherever the reference margin exceeds 3 TOL; prompts and batched
steps run in 16-row chunks of the fused kernel, which ti_engine_counters counts."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_engine import MID, TOL, margin
from test_gpu_gemm_mx import E2M1

pytestmark = pytest.mark.gpu


def build(ti, oracle, max_batch, seed):   # (MX engine, oracle model) with the same weights
    from pyoracle import OracleModel, _OrModel
    V, H, NL, I = MID["vocab"], MID["hidden"], MID["layers"], MID["inter"]
    qd, kvd = MID["heads"] * MID["head_dim"], MID["kv_heads"] * MID["head_dim"]
    m = OracleModel(oracle, MID, seed, 0.1)
    base, mm = m.weights(), C.cast(m.ptr, C.POINTER(_OrModel)).contents
    rng = np.random.RandomState(seed)
    e = ti.Engine(V, H, NL, MID["heads"], MID["kv_heads"], MID["head_dim"], I, bits=4 | ti.BITS_G32 | ti.BITS_MX,
                  max_seq=MID["max_seq"], max_batch=max_batch, rope_theta=MID["rope_theta"], eps=MID["eps"])
    assert e.set_qkv_attn(1) == 0   # no fused QKV + attention launch on MX weights
    e.set_tensor(ti.E_EMBED, 0, base["token_embeddings.weight"])
    e.set_tensor(ti.V_OUT_NORM, 0, base["norm.weight"])
    linears = [(ti.W_LM_HEAD, 0, mm.lm_head, H, V)]
    for l in range(NL):
        e.set_tensor(ti.V_ATTN_NORM, l, base[f"layers.{l}.attention_norm.weight"])
        e.set_tensor(ti.V_FFN_NORM, l, base[f"layers.{l}.ffn_norm.weight"])
        linears += [(ti.W_Q, l, mm.wq[l], H, qd), (ti.W_K, l, mm.wk[l], H, kvd), (ti.W_V, l, mm.wv[l], H, kvd),
                    (ti.W_O, l, mm.wo[l], qd, H), (ti.W_GATE, l, mm.wg[l], H, I), (ti.W_UP, l, mm.wu[l], H, I),
                    (ti.W_DOWN, l, mm.wd[l], I, H)]
    for slot, l, ptr, K, N in linears:   # block scales within 4x of 0.1 / sqrt(K): weights of a trained model's size
        codes = rng.randint(0, 16, (K, N)).astype(np.uint8)
        sc = (127 + int(np.round(np.log2(0.1 / np.sqrt(K)))) + rng.randint(-1, 2, (K // 32, N))).astype(np.uint8)
        e.set_tensor_mx(slot, l, codes, sc)
        w = E2M1[codes] * np.exp2(sc.astype(np.float64) - 127).repeat(32, axis=0)
        np.ctypeslib.as_array(ptr, shape=(K * N,))[:] = w.astype(np.float32).reshape(-1)   # (exact) the oracle's weight
    return e, m


@pytest.mark.parametrize("n_prompt,chunks", [(1, 0), (100, 7)])   # 99 prefilled rows: seven 16-row chunks
def test_prompt_then_greedy_vs_oracle(ti, oracle, n_prompt, chunks):
    prompt = np.random.RandomState(31).randint(0, MID["vocab"], size=n_prompt).tolist()
    e, m = build(ti, oracle, 1, 78)
    got, glg = e.generate([prompt], 4, want_logits=True)
    assert e.counters()[1] == chunks
    e.close()
    for t in prompt:
        tok, lg = m.step(t)
    for i, g in enumerate(got[0].tolist()):
        last, wide = lg, margin(lg) > 3 * TOL * float(np.max(np.abs(lg)))
        assert g == tok or not wide, f"token {i}: gpu {g} ref {tok}"
        if g != tok:
            break   # (a narrow margin decided otherwise: the sequences part here)
        tok, lg = m.step(tok)
    else:
        err, bar = float(np.max(np.abs(glg[0].astype(np.float64) - last))), TOL * float(np.max(np.abs(last)))
        print(f"last logits off by {err:.3e} (bar {bar:.3e})")
        assert err <= bar
    m.close()


def test_batched_decode_vs_oracle(ti, oracle):   # 20 streams x 4 steps: two fused pieces (16 + 4 rows) per projection
    from pyoracle import OracleModel
    B, (e, m0) = 20, build(ti, oracle, 20, 81)
    models, weights = [m0] + [OracleModel(oracle, MID, 81, 0.1) for _ in range(B - 1)], m0.weights()
    for m in models[1:]:
        m.set_weights(weights)
    e.set_prefill(0)
    BITS = 4 | ti.BITS_G32 | ti.BITS_MX   # the route of a 20-row step: 16-row pieces of gemv_mx_kernel, no rows kernel
    assert ti.lib().ti_gemm_max_rows(BITS, ti.X_F32_RMSNORM, 512, 512) == 16
    assert ti.gemm_kernel_name(BITS, ti.X_F16, B, 512, 512).startswith("gemv_mx_kernel<")
    toks, worst = [int(t) for t in np.random.RandomState(9).randint(0, MID["vocab"], size=B)], 0.0
    for pos in range(4):
        lg = e.step(toks, [pos] * B)
        for i, m in enumerate(models):
            ref_t, ref_lg = m.step(toks[i])
            worst = max(worst, float(np.max(np.abs(lg[i].astype(np.float64) - ref_lg))) / float(np.max(np.abs(ref_lg))))
            assert int(np.argmax(lg[i])) == ref_t or margin(ref_lg) <= 3 * TOL * float(np.max(np.abs(ref_lg)))
            toks[i] = ref_t
    assert e.counters()[1] == 0   # (no prompt chunks: the rows went through the step)
    e.close()
    print(f"worst relative logit error {worst:.3e}")
    assert worst <= TOL, worst
