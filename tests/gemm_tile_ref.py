"""Test helper: float64 references and compare rules for the epilogues of gemm_tile_kernel (int4 group-128
weights x fp16 rows, gemv.hip), shared by test_gpu_gemm_tile.py (the device's outputs) and test_gemm_tile_ref.py
(mutants of the float64 result, which every rule below must reject).

Every check_* asserts its rule at the project's bar and returns the worst error-to-bar ratio it saw, so the GPU
tests can report how much of each bar the kernel uses.
"""
from __future__ import annotations

import numpy as np

import kv8_ref as Q
from test_gpu_kernels import assert_close_dot

f16, f32, f64 = np.float16, np.float32, np.float64

# the bars (tests/test_gpu_kernels.py, tests/test_gpu_batched.py)
REL_STORE, REL_RESID = 2e-5, 5e-5
F16_BAR = dict(rtol=2e-3, atol=2e-3)
SILU_BAR = dict(rtol=3e-3, atol=2e-3)
Q_BAR = dict(rtol=1e-4, atol=1e-4)


def check_dot(got, ref, xa, wf, rel=REL_STORE):
    """fp32 outputs of a dot product: finite and within assert_close_dot's summation-order bound."""
    assert np.all(np.isfinite(got)), "non-finite output"
    assert_close_dot(got, ref, xa, wf, rel=rel)
    bound = rel * (np.abs(xa).astype(f64) @ np.abs(wf).astype(f64)) + 1e-6
    return float(np.max(np.abs(got.astype(f64) - ref) / bound))


def check_close(got, ref, rtol, atol, what=""):
    assert np.all(np.isfinite(got)), f"{what}: non-finite output"
    got = np.asarray(got, f64)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=what)
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref)))) if got.size else 0.0


def check_resid(after, before, ref, xa, wf):
    """In-place residual add: after - before is the product, once (REL_RESID covers the rounding of the add)."""
    assert np.all(np.isfinite(after)), "non-finite output"
    return check_dot(after.astype(f64) - before.astype(f64), ref, xa, wf, rel=REL_RESID)


def silu_mul64(g, u):
    return u * (g / (1 + np.exp(-g)))


def rope64(y, pos, cs, hd):
    """y float64 [M][heads * hd], rotated by the table the kernel reads: cs [max_seq][hd / 2][(cos, sin)], row m at
    pos[m]; pairs (2 i, 2 i + 1)."""
    M, n = y.shape
    yh = y.reshape(M, n // hd, hd // 2, 2)
    c = cs.astype(f64)[np.asarray(pos)]
    cos, sin = c[:, None, :, 0], c[:, None, :, 1]
    out = np.empty_like(yh)
    out[..., 0] = yh[..., 0] * cos - yh[..., 1] * sin
    out[..., 1] = yh[..., 1] * cos + yh[..., 0] * sin
    return out.reshape(M, n)


def kv_slots(pos, nkv, hd, max_seq, stride):
    """Element index [M][nkv][hd] of row m's slot in a cache [stream][kv head][max_seq][hd]: row m is stream m
    (stride elements apart), or with stride 0 (prefill) a row of the one stream."""
    pos = np.asarray(pos, np.int64)
    m = np.arange(pos.size, dtype=np.int64)[:, None, None]
    return m * stride + (np.arange(nkv)[None, :, None] * max_seq + pos[:, None, None]) * hd + np.arange(hd)[None, None, :]


def check_kv_f16(cache, want, idx, what):
    """cache: flat fp16; want float64 [M][nkv * hd] at element indices idx; every other element still zero."""
    written = np.zeros(cache.size, bool)
    written[idx] = True
    assert not cache[~written].any(), f"{what}: cache written outside the slots named by pos"
    return check_close(cache[idx].reshape(want.shape), want, what=what, **F16_BAR)


def check_kv_e4m3(cache, h, idx, what):
    """cache: flat e4m3 bytes, h: the flat fp16 cache of the same call (kv8_ref.append_ok's rule)."""
    written = np.zeros(cache.size, bool)
    written[idx] = True
    assert not cache[~written].any(), f"{what}: e4m3 cache written outside the slots named by pos"
    is_nb, must, equal = Q.append_ok(cache[idx], h[idx])
    assert is_nb.all(), f"{what}: a byte that is no neighbour code of its fp16 value"
    assert not (must & ~equal).any(), f"{what}: a wrong must-equal byte"
    assert must.mean() > 0.9, what
    return float(must.mean())


def order_key(v):
    u = np.asarray(v, f32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def check_argmax(keys, logits):
    """keys uint64 [M][slots]: the row's max key names NumPy's argmax (the lowest index among equal logits) and
    carries that logit's bits."""
    k = keys.max(axis=1)
    idx = (0xFFFFFFFF - (k & 0xFFFFFFFF)).astype(np.int64)
    np.testing.assert_array_equal(idx, np.argmax(logits, axis=1))
    np.testing.assert_array_equal(k >> 32, order_key(logits[np.arange(len(idx)), idx]))
    return idx


def splitk_sum_f32(x, wf, n_ks):
    """x fp16 [M][K] @ wf float64 [K][N] the way the last arriver merges: slice ks covers the 128-k groups
    [ks KT / n_ks, (ks + 1) KT / n_ks), every slice's partial rounded to fp32, the partials added in fp32 in slice
    order from 0.  (Each partial here is exact before its rounding: the emulation isolates the merge's error.)"""
    KT = x.shape[1] // 128
    total = np.zeros((x.shape[0], wf.shape[1]), f32)
    for ks in range(n_ks):
        a, b = ks * KT // n_ks * 128, (ks + 1) * KT // n_ks * 128
        total = total + (x[:, a:b].astype(f64) @ wf[a:b]).astype(f32)
    return total


# ------------------------------------------------------------------ inputs shared by the GPU and the CPU tests
def rows(M, K, seed):
    return np.random.RandomState(seed).standard_normal((M, K)).astype(f16)


def qkv_inputs(hd, nh, nkv, M, K, form):
    """One QKV_ROPE_KV case: fp32 weights (q, k, v), fp16 rows, positions, max_seq and the stream stride.
    form "prefill": one stream (stride 0), distinct positions in no row order; "batched": a stream per row."""
    rng = np.random.RandomState(hd + 7 * nh + M + K + (form == "prefill"))
    qd, kvd = nh * hd, nkv * hd
    ws = [(rng.standard_normal((K, n)) * 0.05).astype(f32) for n in (qd, kvd, kvd)]
    x = rng.standard_normal((M, K)).astype(f16)
    if form == "prefill":
        max_seq, stride = M + 7, 0
        pos = rng.permutation(max_seq)[:M].astype(np.int32)
    else:
        max_seq, stride = 20, nkv * 20 * hd
        pos = rng.randint(0, max_seq, size=M).astype(np.int32)
    return ws, x, pos, max_seq, stride
