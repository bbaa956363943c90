"""sample.hip against the NumPy statement of its contract (tests/sample_ref.py) where the Gaussian rows of
test_gpu_sample.py never go: more than kCand = 2048 keys at the threads' k-th maximum (the row-wide radix select
at top_k <= 1024 and its cross-wave tie bookkeeping), ties at every rank, zeros of both signs at the top-k cut, V
around the wave, thread-count and kCacheV boundaries, V = 1, the n < 16 tail of the sequential scan, a V that is
no multiple of 4 in the HBM workspace, ldl > V, and ti_sample_step's draw-index arithmetic on its own.

The cases, their rows and their placed top_p / draws are tests/sample_edge_cases.py (checked on the CPU by
test_sample_ref.py).  Every case runs five draws in one launch (M = 5 copies of the row): three placed in the
middle of a survivor's interval, u = 0 and u = 1.  The token must be the reference's, log p within
1e-5 * max(1, |log p|), -inf must be -inf.  Nothing is skipped: decidability (sample_ref.py) is asserted again
here for every draw.  Only a draw at u = 1 may have two stated answers -- the last running sum is 1 give or take
an ulp of the device's exp, and unless the last survivor with probability is token V - 1 or all survivors are
equal, the two sides of that boundary differ: (the last such survivor, its log p) or (V - 1, -inf / log p[V - 1]);
the device must give one of the two, bit-for-bit the rule of the reference either way.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import sample_edge_cases as E

pytestmark = pytest.mark.gpu

f32 = np.float32
M = 5
SLOTS = 32                                                    # TI_ARGMAX_SLOTS
LP_FILL = np.array([0xC2F6CDEF], np.uint32).view(f32)[0]      # a recognisable bit pattern


def launch(ti, r, ldl=None):
    """The case's five draws in one launch -> (tokens int32 [5], logprobs f32 [5]).  ldl > V: the padding holds
    +inf in the even rows and NaN in the odd ones."""
    c, L = r.case, ti.lib()
    ldl = ldl or c.V
    lg = np.empty((M, ldl), f32)
    lg[0::2, c.V:] = np.inf
    lg[1::2, c.V:] = np.nan
    lg[:, :c.V] = r.logits
    D = ti.DeviceBuffer
    ld, dd, tok_d, lp_d = D.from_array(lg), D.from_array(r.draws), D(M * 4), D(M * 4)
    tok_d.upload(np.full(M, -7, np.int32))
    lp_d.upload(np.full(M, LP_FILL, f32))
    wsb = L.ti_sample_workspace_bytes(c.V, c.k)
    assert (wsb > 0) == (c.k > E.MAX_K)
    ws = D(M * wsb) if wsb else None
    ti.check(L.ti_sample_device_ws(ld.ptr, ldl, M, c.V, float(c.T), c.k, float(r.top_p), dd.ptr, tok_d.ptr, lp_d.ptr,
                                   ws.ptr if ws else None, None))
    ti.sync()
    return tok_d.download(np.int32, M), lp_d.download(f32, M)


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_case_matches_the_reference(ti, name):
    r = E.realise(name)
    assert E.decidable_cut(r.cut), (r.cut.top_p_margin, r.cut.rank_gap)
    toks, lps = launch(ti, r)
    for m in range(M):
        E.assert_draw(toks[m], lps[m], r.want[m], m == M - 1, (name, m, float(r.draws[m]), float(r.top_p)))


@pytest.mark.parametrize("name", E.PAD_CASES)
def test_padding_between_rows_is_never_read(ti, name):
    """ldl = V + 37 with +inf / NaN between the rows: bit for bit the unpadded launch's results."""
    r = E.realise(name)
    toks, lps = launch(ti, r)
    toks_p, lps_p = launch(ti, r, ldl=r.case.V + E.PAD)
    assert np.array_equal(toks, toks_p), (toks, toks_p)
    assert np.array_equal(lps.view(np.uint32), lps_p.view(np.uint32)), (lps, lps_p)
    for m in range(M):
        E.assert_draw(toks_p[m], lps_p[m], r.want[m], m == M - 1, (name, m))


def key_of(tok):
    return (0xFFFFFFFF << 32) | (0xFFFFFFFF - tok)


@pytest.mark.parametrize("T,k", E.STEP_SETTINGS)
def test_sample_step_draw_index(ti, T, k):
    """ti_sample_step / ti_sample_step_ws alone: M = 3 streams, draw_stride 5, n_in = [1, 3, 6]; over the launches
    every stream passes t = (*step_ctr - advance) - (n_in[m] - 1) = -1, 0, a middle value, 4 and 5.  A live row
    writes the feedback key of the reference's token for draws[m * 5 + t] into slot 0 of its argmax slots and the
    log p into logprobs[m * 5 + t]; every other word of both buffers stays what it was filled with."""
    L, D = ti.lib(), ti.DeviceBuffer
    vp, i32, cf = C.c_void_p, C.c_int32, C.c_float
    L.ti_sample_step_ws.argtypes = [vp, i32, i32, i32, cf, i32, cf, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.ti_sample_step.argtypes = L.ti_sample_step_ws.argtypes[:14] + [vp]
    Ms, S, V = E.STEP_M, E.STEP_STRIDE, E.STEP_V
    logits, draws, want = E.step_rows(T, k)
    assert all(d.decided for d in want.values())
    ld, dd = D.from_array(logits), D.from_array(draws)
    n_in, ctr_d = D.from_array(np.array(E.STEP_N_IN, np.int32)), D(4)
    argmax, lps = D(8 * Ms * SLOTS), D(4 * Ms * S)
    keys0 = (np.arange(Ms * SLOTS, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(1)
    lps0 = np.full(Ms * S, LP_FILL, f32)
    wsb = L.ti_sample_workspace_bytes(V, k)
    assert (wsb > 0) == (k > E.MAX_K)
    ws = D(Ms * wsb) if wsb else None
    seen = set()
    for ctr, adv in E.STEP_LAUNCHES:
        ctr_d.upload(np.array([ctr], np.int32))
        argmax.upload(keys0)
        lps.upload(lps0)
        if ws:
            ti.check(L.ti_sample_step_ws(ld.ptr, V, Ms, V, T, k, 1.0, dd.ptr, S, ctr_d.ptr, adv, n_in.ptr, argmax.ptr,
                                         lps.ptr, ws.ptr, None))
        else:
            ti.check(L.ti_sample_step(ld.ptr, V, Ms, V, T, k, 1.0, dd.ptr, S, ctr_d.ptr, adv, n_in.ptr, argmax.ptr,
                                      lps.ptr, None))
        ti.sync()
        keys, got = argmax.download(np.uint64, Ms * SLOTS), lps.download(f32, Ms * S)
        want_keys, want_lps = keys0.copy(), lps0.copy()
        for m in range(Ms):
            t = E.step_t(ctr, adv, m)
            seen.add((m, t))
            if 0 <= t < S:
                d = want[m, t]
                assert int(keys[m * SLOTS]) == key_of(d.token), (ctr, adv, m, t, 0xFFFFFFFF - (int(keys[m * SLOTS]) & 0xFFFFFFFF), d)
                assert E.lp_matches(got[m * S + t], d.logprob), (ctr, adv, m, t, got[m * S + t], d)
                want_keys[m * SLOTS], want_lps[m * S + t] = keys[m * SLOTS], got[m * S + t]
        assert np.array_equal(keys, want_keys), (ctr, adv, "an argmax word of no live row changed")
        assert np.array_equal(got.view(np.uint32), want_lps.view(np.uint32)), (ctr, adv, "a logprobs word of no live row changed")
        assert ctr_d.download(np.int32, 1)[0] == ctr
    for m in range(Ms):
        assert {(m, -1), (m, 0), (m, S - 1), (m, S)} <= seen
    if ws:                                              # without a workspace: refused before any launch
        assert L.ti_sample_step(ld.ptr, V, Ms, V, T, k, 1.0, dd.ptr, S, ctr_d.ptr, 0, n_in.ptr, argmax.ptr, lps.ptr, None) == 1
