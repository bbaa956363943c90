"""An MXFP4 engine created while gemm_set_mx_rows' switch is on (test_gpu_mx_engine.py's build on MID): a prompt runs
in one chunk and a 20-stream step in one launch per projection, both through gemm_mx_kernel, at that file's bars
(logits within TOL = 2e-3 max|logit|, tokens equal wherever the reference margin exceeds 3 TOL).  The switch is on for
this module only and restored behind it."""
import numpy as np
import pytest

from test_gpu_engine import MID, TOL, margin
from test_gpu_mx_engine import build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def mx_rows_on(ti):
    before = ti.gemm_set_mx_rows(True)
    yield
    ti.gemm_set_mx_rows(before)


def test_prompt_in_one_chunk_then_greedy_vs_oracle(ti, oracle):
    prompt = np.random.RandomState(31).randint(0, MID["vocab"], size=100).tolist()
    e, m = build(ti, oracle, 1, 78)
    got, glg = e.generate([prompt], 4, want_logits=True)
    assert e.counters()[1] == 1   # 99 prefilled rows: one chunk (16-row pieces take seven)
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


def test_batched_decode_vs_oracle(ti, oracle):   # 20 streams x 4 steps: one gemm_mx_kernel launch per projection
    from pyoracle import OracleModel
    B, (e, m0) = 20, build(ti, oracle, 20, 81)
    models, weights = [m0] + [OracleModel(oracle, MID, 81, 0.1) for _ in range(B - 1)], m0.weights()
    for m in models[1:]:
        m.set_weights(weights)
    e.set_prefill(0)
    assert ti.gemm_kernel_name(4 | ti.BITS_G32 | ti.BITS_MX, ti.X_F16, B, 512, 512) == "gemm_mx_kernel"
    toks, worst = [int(t) for t in np.random.RandomState(9).randint(0, MID["vocab"], size=B)], 0.0
    for pos in range(4):
        lg = e.step(toks, [pos] * B)
        for i, m in enumerate(models):
            toks[i], ref_lg = m.step(toks[i])
            worst = max(worst, float(np.max(np.abs(lg[i].astype(np.float64) - ref_lg))) / float(np.max(np.abs(ref_lg))))
    e.close()
    print(f"worst relative logit error {worst:.3e}")
    assert worst <= TOL, worst
