"""On-device sampling (ti_hip.h ti_sample_device / ti_sample_step, ti_engine_generate_sampled)
against the ORACLE's sampler (oracle/ti_oracle_sample.cpp: sample_next_token,
inference_engine.cpp:1554-1673, with the uniform draw given), which tests/test_sampling_oracle.py
pins to the compiled reference's own generate(include_logprobs) output.

Same logits and draw -> same token: the device sums the survivors' probabilities in index
order exactly as the reference's loops over all V do (the rest add exact zeros).  Its exp/log
are the device's (<= 1 ulp from glibc), so log-probabilities agree to 1e-5 and a token could
only differ when a draw lies within ~1e-6 of a cumulative boundary (not hit by these seeds).
Equal logits at the top-k cut: the device keeps the lowest indices, the reference whatever
libstdc++'s std::sort leaves there; test_device_sampler_tied_logits compares with the oracle in
every setting where the two agree and counts the ones where the reference's tie order differs,
and compares EVERY setting with tests/sample_ref.py, the NumPy statement of the documented tie
rule, at a placed top_p and placed draws (tests/test_gpu_sample_edges.py has the rows made for
that rule).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import sample_edge_cases as E

pytestmark = pytest.mark.gpu

f32 = np.float32


def dev(ti, a):
    return ti.DeviceBuffer.from_array(np.ascontiguousarray(a))


@pytest.mark.parametrize("V", [1000, 32000, 128256])
@pytest.mark.parametrize("T,k,p", [(1.0, 1, 1.0), (0.7, 40, 0.9), (1.0, 50, 1.0), (1.3, 1024, 0.95),
                                   (0.0, 8, 0.5), (1.0, 200, 0.0), (1.0, 1500, 1.0), (0.9, 2500, 0.97),
                                   (1.0, 4096, 0.9)])
def test_device_sampler_matches_oracle(ti, oracle, V, T, k, p):
    if k > V:
        pytest.skip("top_k above vocab")
    M = 6
    rng = np.random.RandomState(V + k)
    logits = (rng.standard_normal((M, V)) * 3).astype(f32)
    draws = rng.uniform(0, 1, M).astype(f32)
    draws[0] = 0.0            # the reference's u == 0 corner: index 0 at the first comparison
    draws[1] = 1.0            # the top of the range
    ld, dd = dev(ti, logits), dev(ti, draws)
    tok_d, lp_d = ti.DeviceBuffer(M * 4), ti.DeviceBuffer(M * 4)
    ti.check(ti.lib().ti_sample_device(ld.ptr, V, M, V, T, k, p, dd.ptr, tok_d.ptr, lp_d.ptr, None))
    ti.sync()
    got_t, got_lp = tok_d.download(np.int32, M), lp_d.download(f32, M)
    for m in range(M):
        want_t, want_lp = oracle.sample_token(logits[m], T, k, p, float(draws[m]))
        assert int(got_t[m]) == want_t, (m, int(got_t[m]), want_t)
        if np.isfinite(want_lp):
            assert abs(float(got_lp[m]) - want_lp) <= 1e-5 * max(1.0, abs(want_lp)), (m, got_lp[m], want_lp)
        else:
            assert not np.isfinite(got_lp[m])


def check_row_against_sample_ref(ti, logits, T, k, p):
    """One row under the documented tie rule: top_p placed next to p, three placed draws, u = 0 and u = 1."""
    top_p, draws, cut, want = E.realise_row(logits, T, k, p)
    assert E.decidable_cut(cut), (T, k, p, cut.top_p_margin, cut.rank_gap)
    M, V = len(draws), logits.size
    ld, dd = dev(ti, np.tile(logits, (M, 1))), dev(ti, draws)
    tok_d, lp_d = ti.DeviceBuffer(M * 4), ti.DeviceBuffer(M * 4)
    ti.check(ti.lib().ti_sample_device(ld.ptr, V, M, V, T, k, float(top_p), dd.ptr, tok_d.ptr, lp_d.ptr, None))
    ti.sync()
    got_t, got_lp = tok_d.download(np.int32, M), lp_d.download(f32, M)
    for m in range(M):
        E.assert_draw(got_t[m], got_lp[m], want[m], m == M - 1, (T, k, p, m, float(draws[m]), float(top_p)))


def test_device_sampler_tied_logits(ti, oracle):
    """The reference's plumbing logits (every value twice: lm_head repeats every 500 columns): the oracle where
    its tie order is the lowest indices, tests/sample_ref.py (lowest index first by definition) in every setting."""
    V = 1000
    lg = np.stack([oracle.plumbing_generate(V, 256, 4, [1, 15, 25, 35], s + 1)[1] for s in range(2)])
    ld = dev(ti, lg)
    agree = differ = 0
    for T, k, p in [(1.0, 2, 1.0), (1.0, 3, 1.0), (0.7, 40, 0.9), (2.0, 7, 0.99), (0.9, 9, 1.0), (1.0, 50, 0.9),
                    (1.3, 0, 0.95), (0.5, 1000, 0.5)]:
        if k == 0:
            continue                                     # the device sampler needs 1 <= k
        for row in lg:
            check_row_against_sample_ref(ti, row, T, k, p)
        # survivors under lowest-index-first ties vs the reference's std::sort order
        low = [set(np.lexsort((np.arange(V), -row))[:k].tolist()) for row in lg]
        ref = [set(np.flatnonzero(np.isfinite(np.log(oracle.sample_probs(row, 1.0, k, 1.0)))).tolist()) for row in lg]
        if low != ref:
            differ += 1
            continue
        draws = np.array([0.3, 0.8], f32)
        tok_d, lp_d, dd = ti.DeviceBuffer(2 * 4), ti.DeviceBuffer(2 * 4), dev(ti, draws)
        ti.check(ti.lib().ti_sample_device(ld.ptr, V, 2, V, T, k, p, dd.ptr, tok_d.ptr, lp_d.ptr, None))
        ti.sync()
        got_t, got_lp = tok_d.download(np.int32, 2), lp_d.download(f32, 2)
        for m in range(2):
            want_t, want_lp = oracle.sample_token(lg[m], T, k, p, float(draws[m]))
            assert int(got_t[m]) == want_t, (T, k, p, m, int(got_t[m]), want_t)
            assert abs(float(got_lp[m]) - want_lp) <= 1e-5 * max(1.0, abs(want_lp))
        agree += 1
    print(f"tied logits: {agree} settings compared, {differ} with a reference tie order other than lowest-index")
    assert agree >= 4


@pytest.mark.parametrize("V", [32000, 128256])
@pytest.mark.parametrize("T,k,p", [(1.0, 8192, 1.0), (0.8, 8192, 0.9), (1.0, -1, 0.95), (1.2, -1, 1.0),
                                   (1.0, 20000, 0.5)])
def test_device_sampler_any_top_k(ti, oracle, V, T, k, p):
    """top_k above TI_SAMPLE_MAX_K, up to V (the reference accepts any k,
    inference_engine.cpp:1585-1598): the survivors live in an HBM workspace
    (ti_sample_device_ws); same tokens and log-probs as the oracle sampler.  k = -1: k = V."""
    k = V if k < 0 else k
    M = 3
    rng = np.random.RandomState(V + k + 1)
    logits = (rng.standard_normal((M, V)) * 3).astype(f32)
    draws = rng.uniform(0, 1, M).astype(f32)
    draws[0] = 0.999
    L = ti.lib()
    L.ti_sample_workspace_bytes.restype = C.c_size_t
    L.ti_sample_workspace_bytes.argtypes = [C.c_int, C.c_int]
    wsb = L.ti_sample_workspace_bytes(V, k)
    assert wsb > 0 and L.ti_sample_workspace_bytes(V, 4096) == 0
    ws = ti.DeviceBuffer(M * wsb)
    ld, dd = dev(ti, logits), dev(ti, draws)
    tok_d, lp_d = ti.DeviceBuffer(M * 4), ti.DeviceBuffer(M * 4)
    # without a workspace: refused before any launch
    assert L.ti_sample_device(ld.ptr, V, M, V, T, k, p, dd.ptr, tok_d.ptr, lp_d.ptr, None) == 1
    ti.check(L.ti_sample_device_ws(ld.ptr, V, M, V, T, k, p, dd.ptr, tok_d.ptr, lp_d.ptr, ws.ptr, None))
    ti.sync()
    got_t, got_lp = tok_d.download(np.int32, M), lp_d.download(f32, M)
    for m in range(M):
        want_t, want_lp = oracle.sample_token(logits[m], T, k, p, float(draws[m]))
        assert int(got_t[m]) == want_t, (m, int(got_t[m]), want_t)
        assert abs(float(got_lp[m]) - want_lp) <= 1e-5 * max(1.0, abs(want_lp)), (m, got_lp[m], want_lp)


def test_device_sampler_rejects_bad_top_k(ti):
    L = ti.lib()
    rc = L.ti_sample_device(1, 1000, 1, 1000, 1.0, 0, 1.0, 1, 1, None, None)
    assert rc == 1
    rc = L.ti_sample_device(1, 5000, 1, 5000, 1.0, 5001, 1.0, 1, 1, None, None)
    assert rc == 1


CFGS = {
    # name: vocab, hidden, layers, heads, kv_heads, head_dim, inter, bits
    "mini_gqa_w4": (512, 256, 2, 4, 2, 64, 512, 4),
    "l2_shape_w4": (32000, 4096, 2, 32, 32, 128, 11008, 4),
}


@pytest.mark.parametrize("name,k", [("mini_gqa_w4", 40), ("l2_shape_w4", 40), ("l2_shape_w4", 9000)])
def test_engine_sampled_generate_matches_host_loop(ti, oracle, name, k):
    """The device loop with on-device sampling against ti_engine_step (the same kernels, logits
    to the host) + the oracle's sampler, fed the same draws: identical tokens and log-probs.  With
    prefill the prompt's KV comes from the batched kernels (rounding within the decode
    tolerance): the same tokens up to the first draw that lands across a moved boundary."""
    v, h, l, nh, nkv, hd, inter, bits = CFGS[name]
    T, p, new = 0.8, 0.9, 16
    prompt = [3, 17, 99, 5, 250, 7]
    draws = np.random.RandomState(5).uniform(0, 1, new).astype(f32)
    e = ti.Engine(v, h, l, nh, nkv, hd, inter, bits=bits, max_seq=128, max_batch=1)
    e.synth(0x7157, 0.1)
    e.set_prefill(0)
    got, got_lp = e.generate_sampled([prompt], new, T, k, p, draws)
    e.set_prefill(32)
    got_pf, got_pf_lp = e.generate_sampled([prompt], new, T, k, p, draws)
    # host loop: teacher-forced steps on a twin engine
    ref = ti.Engine(v, h, l, nh, nkv, hd, inter, bits=bits, max_seq=128, max_batch=1)
    ref.synth(0x7157, 0.1)
    toks, want, want_lp = list(prompt), [], []
    for pos in range(len(prompt) + new - 1):
        lg = ref.step([toks[pos]], [pos])[0]
        if pos >= len(prompt) - 1:
            t, lp = oracle.sample_token(lg, T, k, p, float(draws[len(want)]))
            want.append(t)
            want_lp.append(lp)
            toks.append(t)
    e.close()
    ref.close()
    assert got[0].tolist() == want
    np.testing.assert_allclose(got_lp[0], np.array(want_lp, f32), rtol=1e-5, atol=1e-5)
    # prefill: the prompt's KV from the batched kernels moves the logits within the decode
    # tolerance, which moves a draw across a cumulative boundary now and then; the sequences
    # agree up to the first such step (8 of 16 here) and the log-probs agree before it
    # (k = 9000: thousands of survivors put the draw boundaries closer than that tolerance, so
    # only the exact-kernel sequence above is compared)
    if k > 1000:
        return
    same = [a == b for a, b in zip(got_pf[0].tolist(), want)] + [False]
    j = same.index(False)
    assert j >= 4, (got_pf[0].tolist(), want)
    np.testing.assert_allclose(got_pf_lp[0][:j], np.array(want_lp, f32)[:j], atol=1e-2)
