"""A Q4_K engine (bits 4 | BITS_G32 | BITS_KQ) on test_gpu_engine.py's GQA model MID: every linear weight is exact
super-blocks uploaded through set_tensor_kq, and the oracle model holds the dequantized values.  Logits within that
file's TOL (2e-3 max|logit|), tokens equal wherever the reference margin exceeds 3 TOL, prompt chunks counted."""
import numpy as np
import pytest

import test_gpu_mx_engine as mxe
from test_gpu_engine import MID, engine_for
from test_gpu_gemm_kq import dequant
from test_gpu_w16_rows_engine import SLOTS

pytestmark = pytest.mark.gpu
BITS = 4 | 32 | 512
TOP = {"token_embeddings.weight": "E_EMBED", "norm.weight": "V_OUT_NORM", "lm_head.weight": "W_LM_HEAD"}


def build(ti, oracle, max_batch, seed):   # (KQ engine, oracle model) with the same weights
    from pyoracle import OracleModel
    m, rng = OracleModel(oracle, MID, seed, 0.1), np.random.RandomState(seed)
    w, e = m.weights(), engine_for(ti, dict(MID, bits=BITS), max_batch=max_batch)
    assert e.set_qkv_attn(1) == 0   # no fused QKV + attention launch on Q4_K weights
    with pytest.raises(ti.TiError):  # fp32 values are not quantized into this format
        e.set_tensor(ti.W_Q, 0, w["layers.0.attention.q_proj.weight"])
    for name, a in w.items():
        p = name.split(".", 2)
        slot, l = (getattr(ti, SLOTS[p[2]]), int(p[1])) if p[0] == "layers" else (getattr(ti, TOP[name]), 0)
        if a.ndim == 1 or slot == ti.E_EMBED:
            e.set_tensor(slot, l, a)
            continue
        # blocks as a quantizer leaves them: dmin m near the middle of the block's range (dmin = 7.5 d, m within 2 of sc),
        # weights about 0.03; independent sc and m (test_gpu_gemm_kq.py) would offset every block by as much as its weights
        (K, N), q = a.shape, rng.randint(0, 16, a.shape)
        sc = rng.randint(0, 64, (K // 32, N))
        d = (rng.uniform(0.5, 1.5, (K // 256, N)) * 2e-4).astype(np.float16)
        blk = q, sc, np.clip(sc + rng.randint(-2, 3, sc.shape), 0, 63), d, (7.5 * d.astype(np.float32)).astype(np.float16)
        e.set_tensor_kq(slot, l, *blk)
        w[name] = dequant(*blk)[0]
    m.set_weights(w)
    return e, m


@pytest.mark.parametrize("body,args", [("test_prompt_then_greedy_vs_oracle", (1, 0)), ("test_prompt_then_greedy_vs_oracle", (100, 7)),
                                       ("test_batched_decode_vs_oracle", ())])
def test_vs_oracle(ti, oracle, monkeypatch, body, args):
    """test_gpu_mx_engine.py's bodies on this file's engine and model: a 1- and a 100-token prompt (99 prefilled rows, seven
    16-row chunks) then greedy decode, and 20 streams x 4 teacher-forced steps (16 + 4 rows) with the logit bar at each."""
    monkeypatch.setattr(mxe, "build", build)
    assert ti.lib().ti_gemm_max_rows(BITS, ti.X_F32_RMSNORM, 512, 512) == 16   # 16-row pieces, no rows kernel
    assert ti.gemm_kernel_name(BITS, ti.X_F16, 20, 512, 512).startswith("gemv_kq_kernel<")
    getattr(mxe, body)(ti, oracle, *args)
