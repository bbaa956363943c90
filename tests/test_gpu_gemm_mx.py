"""gemv_mx_kernel (MXFP4 blocks, 4 | BITS_G32 | BITS_MX) through ti_gemm_wq_a16 against float64 x_fp16 @ W with W the
exactly dequantized blocks, 2^(e - 127) e2m1(code).  e is drawn from [100, 140] per block (a wrong shift or bias is a
power-of-two error) and the codes run through all 16 nibbles at every (k % 128, n % 16) position of a tile over
16 tiles.  Bar: test_gpu_g32.py's fp32-summation bound of the Q4_0 instance, 2e-5 |x| @ |W| + 1e-6 (the MX kernel does
a subset of that kernel's fp32 operations), + 1e-3 |x| @ |W| behind the rms_norm prologue as there (one fp16 ulp of
the normalised row).  17 and 40 rows run as 16-row pieces.  The fp16-output epilogues draw e from [100, 124] so the
outputs stay finite in fp16, and are held to test_gpu_gemm_w8.py's bars."""
import functools

import numpy as np
import pytest

from test_gpu_g32 import assert_close_dot
from test_gpu_gemm_w8 import epilogue
from test_gpu_kernels import dev, gemm

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64
E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])


def mx_weight(rng, K, N, e_hi=140):
    k, n = np.arange(K)[:, None], np.arange(N)[None, :]
    codes = ((rng.randint(0, 16, (128, 16))[k % 128, n % 16] + k // 128 + n // 16) % 16).astype(np.uint8)
    e = rng.randint(100, e_hi + 1, (K // 32, N)).astype(np.uint8)
    return codes, e, E2M1[codes] * np.exp2(e.astype(f64) - 127).repeat(32, axis=0)


@functools.lru_cache(maxsize=None)
def weights(ti, K, N):
    codes, e, w = mx_weight(np.random.RandomState(K + N), K, N)
    return tuple(dev(ti, a) for a in ti.wpack_mx(codes, e)) + (w,)


def mx(ti, td, sd, xd, x_kind, M, N, K, ep, norm=None):
    gemm(ti, td, sd, 4 | ti.BITS_G32 | ti.BITS_MX, xd, x_kind, K, M, N, K, ep, norm_d=norm)


def check(y, xa, w, rel=2e-5):
    err, bound = np.abs(y.astype(f64) - xa.astype(f64) @ w), rel * (np.abs(xa.astype(f64)) @ np.abs(w)) + 1e-6
    print(f"worst error / bound {np.max(err / bound):.3f}")
    assert_close_dot(y, xa.astype(f64), w, rel)


def x_kinds(ti, oracle, rng, M, K):
    """(x kind, device x, device norm weight, the fp16-rounded rows the kernel multiplies, bound factor)"""
    x, nw = rng.standard_normal((M, K)).astype(f32), (1 + 0.1 * rng.standard_normal(K)).astype(f32)
    return [(ti.X_F32, dev(ti, x), None, x.astype(f16), 2e-5), (ti.X_F16, dev(ti, x.astype(f16)), None, x.astype(f16), 2e-5),
            (ti.X_F32_RMSNORM, dev(ti, 3 * x), dev(ti, nw), oracle.rms_norm(3 * x, nw).astype(f16), 2e-5 + 1e-3)]


@pytest.mark.parametrize("M", [1, 2, 3, 16, 17, 40])
@pytest.mark.parametrize("K,N", [(128, 16), (128, 48), (384, 16), (384, 48), (4096, 16), (4096, 48), (4096, 4096)])
def test_store_f32(ti, oracle, M, K, N):
    assert ti.gemm_kernel_name(4 | ti.BITS_G32 | ti.BITS_MX, ti.X_F16, M, N, K).startswith("gemv_mx_kernel<")
    td, sd, w = weights(ti, K, N)
    for kind, xd, nd, xa, rel in x_kinds(ti, oracle, np.random.RandomState(M), M, K):
        yd = dev(ti, np.full((M, N), -7.25, f32))
        mx(ti, td, sd, xd, kind, M, N, K, epilogue(ti, ti.EPI_STORE_F32, N, yd), nd)
        check(yd.download(f32, (M, N)), xa, w, rel)


def test_one_weight_per_block_at_each_position(ti):
    """Column n holds one non-zero weight per block, at position n: the nibble -> k mapping of every lane slot."""
    K, N, M = 256, 32, 2
    rng = np.random.RandomState(9)
    codes, e = np.zeros((K, N), np.uint8), rng.randint(100, 141, (K // 32, N)).astype(np.uint8)
    for n in range(N):
        codes[n::32, n] = rng.randint(1, 8, K // 32) | rng.choice([0, 8], K // 32)
    td, sd = (dev(ti, a) for a in ti.wpack_mx(codes, e))
    x, yd = rng.standard_normal((M, K)).astype(f16), ti.DeviceBuffer(M * N * 4)
    mx(ti, td, sd, dev(ti, x), ti.X_F16, M, N, K, epilogue(ti, ti.EPI_STORE_F32, N, yd))
    check(yd.download(f32, (M, N)), x, E2M1[codes] * np.exp2(e.astype(f64) - 127).repeat(32, axis=0))


@pytest.mark.parametrize("M", [1, 3, 40])   # 1: the one-row instances (f16 x RESID, rms_norm x SILU / QKV / LOGITS)
@pytest.mark.parametrize("kind", ["resid", "silu", "qkv", "argmax"])
def test_other_epilogues(ti, oracle, kind, M):
    rng, K = np.random.RandomState(7 + M), 256
    xs = x_kinds(ti, oracle, rng, M, K)
    if kind == "resid":   # RESID_F32 in place on fp16 rows
        N, (xk, xd, nd, xa, rel) = 2064, xs[1]
        codes, e, w = mx_weight(rng, K, N)
        td, sd = (dev(ti, a) for a in ti.wpack_mx(codes, e))
        r = rng.standard_normal((M, N)).astype(f32)
        rd = dev(ti, r)
        mx(ti, td, sd, xd, xk, M, N, K, epilogue(ti, ti.EPI_RESID_F32, N, rd))
        check(rd.download(f32, (M, N)) - r, xa, w, 5e-5)   # (+ the rounding of r + y)
        return
    xk, xd, nd, xa, rel = xs[2]
    xa = xa.astype(f64)
    if kind == "silu":   # gate / up interleaved by ti_wpack_mx_host's row map
        I = 1032
        (gc, ge, g), (uc, ue, u) = (mx_weight(rng, K, I, 124) for _ in range(2))
        t, s = ti.wpack_mx(gc, ge, 2 * I, ti.ROWS_INTERLEAVE8, 0)
        td, sd = (dev(ti, a) for a in ti.wpack_mx(uc, ue, 2 * I, ti.ROWS_INTERLEAVE8, 8, t, s))
        yd = ti.DeviceBuffer(M * I * 2)
        mx(ti, td, sd, xd, xk, M, 2 * I, K, epilogue(ti, ti.EPI_SILU_MUL_F16, I, yd), nd)
        gg, uu = xa @ g, xa @ u
        np.testing.assert_allclose(yd.download(f16, (M, I)).astype(f64), uu * (gg / (1 + np.exp(-gg))), rtol=3e-3, atol=2e-3)
    elif kind == "qkv":   # per-row positions, GQA, one fp16 cache per row: q, the appended rows, nothing else written
        hd, nh, nkv, max_seq, theta = 64, 4, 2, 32, 10000.0
        qd, kvd = nh * hd, nkv * hd
        ws, N = [mx_weight(rng, K, n, 124) for n in (qd, kvd, kvd)], qd + 2 * kvd
        t = s = None
        for (c, e, _), off in zip(ws, (0, qd, qd + kvd)):
            t, s = ti.wpack_mx(c, e, N, 0, off, t, s)
        pos, stride = rng.randint(0, max_seq, size=M).astype(np.int32), nkv * max_seq * hd
        qb, kc, vc = ti.DeviceBuffer(M * qd * 4), ti.DeviceBuffer(M * stride * 2), ti.DeviceBuffer(M * stride * 2)
        kc.zero(), vc.zero()
        posd, csd = dev(ti, pos), dev(ti, ti.rope_table(np.arange(max_seq, dtype=f32), hd, theta))
        ep = epilogue(ti, ti.EPI_QKV_ROPE_KV, qd, qb)
        ep.q_dim, ep.kv_dim, ep.head_dim, ep.max_seq, ep.kv_fp8 = qd, kvd, hd, max_seq, 0
        ep.pos, ep.rope_cs, ep.k_cache, ep.v_cache, ep.kv_stream_stride = posd.ptr, csd.ptr, kc.ptr, vc.ptr, stride
        mx(ti, dev(ti, t), dev(ti, s), xd, xk, M, N, K, ep, nd)
        q, k, v = (xa @ w[2] for w in ws)
        qgot, (kcache, vcache) = qb.download(f32, (M, qd)), (c.download(f16, (M, nkv, max_seq, hd)) for c in (kc, vc))
        written = np.zeros((M, nkv, max_seq, hd), bool)
        for m in range(M):
            p = np.array([pos[m]], f32)
            written[m, :, pos[m]] = True
            qr = oracle.apply_rope(q[m].astype(f32).reshape(1, nh, 1, hd), p, theta).reshape(-1)
            kr = oracle.apply_rope(k[m].astype(f32).reshape(1, nkv, 1, hd), p, theta).reshape(nkv, hd)
            np.testing.assert_allclose(qgot[m], qr, rtol=2e-3, atol=2e-3)
            np.testing.assert_allclose(kcache[m, :, pos[m]].astype(f32), kr, rtol=3e-3, atol=3e-3)
            np.testing.assert_allclose(vcache[m, :, pos[m]].astype(f32), v[m].reshape(nkv, hd), rtol=3e-3, atol=3e-3)
        assert not kcache[~written].any() and not vcache[~written].any()
    else:   # LOGITS_ARGMAX: the logits at the store bar, each row's key = the lowest index of its largest logit
        V = 4096
        td, sd, w = weights(ti, K, V)
        ld, am, ctr = ti.DeviceBuffer(M * V * 4), ti.DeviceBuffer(M * ti.ARGMAX_SLOTS * 8), dev(ti, np.array([7], np.int32))
        am.zero()
        ep = epilogue(ti, ti.EPI_LOGITS_ARGMAX, V, ld)
        ep.argmax, ep.step_ctr, ep.advance = am.ptr, ctr.ptr, 1
        mx(ti, td, sd, xd, xk, M, V, K, ep, nd)
        logits = ld.download(f32, (M, V))
        keys = am.download(np.uint64, (M, ti.ARGMAX_SLOTS)).max(axis=1)
        np.testing.assert_array_equal((0xFFFFFFFF - (keys & 0xFFFFFFFF)).astype(np.int64), np.argmax(logits, axis=1))
        assert ctr.download(np.int32, (1,))[0] == 8
        check(logits, xa, w, rel)


@pytest.mark.parametrize("K,N,row_map", [(128, 16, 0), (256, 48, 0), (256, 48, 1)])
def test_wsynth_device_matches_the_host_rule(ti, K, N, row_map):
    """ti_wsynth_device's MX branch (wsynth_mx_kernel) against ti_wpack_host of the same seeded values, byte for byte."""
    L, BITS, seed, tid = ti.lib(), 4 | ti.BITS_G32 | ti.BITS_MX, 77, 3
    n_total, off = (2 * N, 8) if row_map else (N + 16, 16)
    amp = np.float32(np.sqrt(np.float32(3.0))) / np.sqrt(np.float32(K))
    wd = ti.DeviceBuffer(K * N * 4)
    ti.check(L.ti_fill_uniform_f32(seed, tid, K * N, amp, 0.0, wd.ptr, None))   # (0 + amp * u: the kernel's values)
    want_t, want_s = ti.wpack_host(wd.download(f32, (K, N)), BITS, n_total, row_map=row_map, row_offset=off)
    td, sd = dev(ti, np.zeros_like(want_t)), dev(ti, np.zeros_like(want_s))
    ti.check(L.ti_wsynth_device(seed, tid, K, N, n_total, BITS, row_map, off, td.ptr, sd.ptr, None))
    ti.sync()
    assert np.array_equal(td.download(np.uint8, want_t.shape), want_t)
    assert np.array_equal(sd.download(np.uint16, want_s.shape), want_s)
