"""ti_sample_device on rows as ti_guide_step leaves them: all but n in {1, 2, 40} entries are -inf (bits
0xFF800000), against the NumPy statement of the sampler's contract (tests/sample_ref.py).

top_k in {1, n, n + 7, V} (n + 7 and V reach into the -inf entries: probability exactly 0, never drawn, whether a
sampler keeps them among its survivors, as the reference statement does, or drops them, as sample.hip does),
top_p in {1, 0.9}, V = 1000 and, for the workspace route of top_k = V > TI_SAMPLE_MAX_K, V = 5000.  Every launch
runs three draws placed with sample_ref.place_draw in the first, the middle and the last interval that kept
probability, so every case is decided (asserted, like the top-p cut): none is left out.  The token must be an
allowed one and its log-probability finite, besides matching the reference."""
from __future__ import annotations

import numpy as np
import pytest

import sample_edge_cases as E
import sample_ref as S

pytestmark = pytest.mark.gpu

f32 = np.float32
T = 0.8
WHICH = ("first", "middle", "last")


def masked_row(V, n, seed):
    r = np.random.RandomState(seed)
    allowed = np.sort(r.choice(V, n, replace=False))
    lg = np.full(V, -np.inf, f32)
    lg[allowed] = (r.standard_normal(n) * 2.0).astype(f32)
    return lg, allowed


@pytest.mark.parametrize("top_p", [1.0, 0.9])
@pytest.mark.parametrize("k_kind", ["one", "n", "n_plus_7", "V"])
@pytest.mark.parametrize("n", [1, 2, 40])
@pytest.mark.parametrize("V", [1000, 5000])
def test_masked_rows_match_the_reference(ti, V, n, k_kind, top_p):
    k = {"one": 1, "n": n, "n_plus_7": n + 7, "V": V}[k_kind]
    lg, allowed = masked_row(V, n, seed=V + 10 * n)
    cut = S.top_p_cut(S.survivors(lg, T, k), top_p)
    assert E.decidable_cut(cut), (cut.top_p_margin, cut.rank_gap)
    draws = np.array([S.place_draw(cut.row, w) for w in WHICH], f32)
    want = [S.draw(cut.row, u) for u in draws]
    assert all(d.decided for d in want), want
    M, L, D = len(WHICH), ti.lib(), ti.DeviceBuffer
    ld, dd, tok_d, lp_d = D.from_array(np.tile(lg, (M, 1))), D.from_array(draws), D(M * 4), D(M * 4)
    tok_d.upload(np.full(M, -7, np.int32))
    lp_d.upload(np.full(M, np.nan, f32))
    wsb = L.ti_sample_workspace_bytes(V, k)
    ws = D(M * wsb) if wsb else None
    ti.check(L.ti_sample_device_ws(ld.ptr, V, M, V, T, k, top_p, dd.ptr, tok_d.ptr, lp_d.ptr, ws.ptr if ws else None, None))
    ti.sync()
    toks, lps = tok_d.download(np.int32, M), lp_d.download(f32, M)
    for m in range(M):
        ctx = (V, n, k, top_p, WHICH[m], float(draws[m]))
        assert int(toks[m]) in allowed, ctx
        assert np.isfinite(lps[m]) and lps[m] <= 0.0, ctx
        E.assert_draw(toks[m], lps[m], want[m], False, ctx)
