"""gemm_w4a_kernel (GGUF Q4_1 blocks, 4 | BITS_G32 | BITS_AFF, fp16 rows above 16) through ti_gemm_wq_a16 against
float64 x_fp16 @ (q d + m) from the integer q and the fp16 d and m.  q1_weight draws every block's d and m
independently, so a scale or minimum of the wrong block or output is a 10-50 % error.  STORE_F32 runs
test_gpu_gemm_w8.py's edges of M, K and N plus PLANS, the shapes whose plan picks the instances that grid does not
reach.  Bar: 2e-5 (|x| @ parts) + 1e-6 with q1_weight's parts, what test_gemm_q41_matches_exact_blocks holds the fused
kernel to (fp32 summation of the two terms only); plus a guard behind the output and a second launch giving the same
bits.  The other epilogues run M = 70 at test_gpu_gemm_w8.py's bars."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_g32 import q1_weight
from test_gpu_gemm_w8 import GUARD, epilogue
from test_gpu_kernels import dev, gemm

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64


def pack(ti, blocks, n_total=None, row_map=0):
    """Device (tiles, scales + minimums) of Q4_1 weights [(q, d, m, row_offset), ..] packed into N_total outputs."""
    L, bits = ti.lib(), 4 | ti.BITS_G32 | ti.BITS_AFF
    K, N = blocks[0][0].shape[0], n_total or blocks[0][0].shape[1]
    tiles = np.zeros(L.ti_wpack_tile_bytes(bits, K, N), np.uint8)
    scales = np.zeros(L.ti_wpack_scale_bytes(bits, K, N) // 2, np.uint16)
    for q, d, m, off in blocks:
        qa, da, ma = (np.ascontiguousarray(v) for v in (q, d.view(np.uint16), m.view(np.uint16)))
        ti.check(L.ti_wpack_q1_host(qa.ctypes.data, da.ctypes.data, ma.ctypes.data, K, q.shape[1], N, row_map, off,
                                    tiles.ctypes.data, scales.ctypes.data))
    return dev(ti, tiles), dev(ti, scales)


def w64(q, d, m):
    return q.astype(f64) * np.repeat(d.astype(f64), 32, axis=0) + np.repeat(m.astype(f64), 32, axis=0)


@functools.lru_cache(maxsize=None)
def weights(ti, K, N):
    """(tiles, scales on the device, W float64, parts) of one seeded weight, made once."""
    q, d, m, _, parts = q1_weight(np.random.RandomState(K + N), K, N)
    return pack(ti, [(q, d, m, 0)]) + (w64(q, d, m), parts.astype(f64))


def is_w4a(ti, M, N, K):
    assert ti.gemm_kernel_name(4 | ti.BITS_G32 | ti.BITS_AFF, ti.X_F16, M, N, K) == "gemm_w4a_kernel"
    plan = ti.gemm_w4a_plan(M, N, K)
    print(f"M={M} N={N} K={K}: (rb, tpw, kwaves, grid) = {plan}")
    return plan


def w4a(ti, td, sd, xd, M, N, K, ep):
    gemm(ti, td, sd, 4 | ti.BITS_G32 | ti.BITS_AFF, xd, ti.X_F16, K, M, N, K, ep)


def store_f32(ti, td, sd, xd, M, N, K):
    yd = dev(ti, np.full(M * N + GUARD, -7.25, f32))
    w4a(ti, td, sd, xd, M, N, K, epilogue(ti, ti.EPI_STORE_F32, N, yd))
    y = yd.download(f32, (M * N + GUARD,))
    yd.free()
    assert np.all(y[M * N:] == -7.25), "guard behind the output overwritten"
    return y[:M * N].reshape(M, N)


def assert_close(y, x, w, parts, rel=2e-5):
    err, bound = np.abs(y.astype(f64) - x.astype(f64) @ w), rel * (np.abs(x.astype(f64)) @ parts) + 1e-6
    print(f"worst error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"max err {err.max()} vs bound {bound[err > bound][:4]}"


GRID = [(M, K, N, None) for M in (17, 33, 64, 65, 130) for K in (128, 384, 4096) for N in (16, 80, 2064)]
PLANS = [(17, 128, 33280, (2, 2, 1)), (130, 384, 11264, (4, 2, 1)), (17, 512, 80, (2, 1, 4)), (130, 512, 4096, (4, 1, 2))]


@pytest.mark.parametrize("M,K,N,plan", GRID + PLANS)
def test_store_f32(ti, M, K, N, plan):
    assert is_w4a(ti, M, N, K)[:3] == plan or plan is None
    td, sd, w, parts = weights(ti, K, N)
    x = np.random.RandomState(M).standard_normal((M, K)).astype(f16)
    xd = dev(ti, x)
    y, again = (store_f32(ti, td, sd, xd, M, N, K) for _ in range(2))
    assert np.array_equal(y.view(np.uint32), again.view(np.uint32)), "a second launch gives other bits"
    assert_close(y, x, w, parts)


def qkv_case(ti, oracle, x, hd):
    """QKV_ROPE_KV, per-row positions, GQA, one fp16 cache per row: q, the appended rows, nothing else written."""
    (M, H), nh, nkv, max_seq, theta = x.shape, 4, 2, 32, 10000.0
    qd, kvd = nh * hd, nkv * hd
    N, rng = qd + 2 * kvd, np.random.RandomState(41 + hd)
    is_w4a(ti, M, N, H)
    ws = [q1_weight(rng, H, n)[:3] for n in (qd, kvd, kvd)]
    td, sd = pack(ti, [w + (off,) for w, off in zip(ws, (0, qd, qd + kvd))], n_total=N)
    pos, stride = rng.randint(0, max_seq, size=M).astype(np.int32), nkv * max_seq * hd
    qb, kc, vc = ti.DeviceBuffer(M * qd * 4), ti.DeviceBuffer(M * stride * 2), ti.DeviceBuffer(M * stride * 2)
    kc.zero(), vc.zero()
    posd, csd = dev(ti, pos), dev(ti, ti.rope_table(np.arange(max_seq, dtype=f32), hd, theta))
    ep = epilogue(ti, ti.EPI_QKV_ROPE_KV, qd, qb)
    ep.q_dim, ep.kv_dim, ep.head_dim, ep.max_seq, ep.kv_fp8 = qd, kvd, hd, max_seq, 0
    ep.pos, ep.rope_cs, ep.k_cache, ep.v_cache, ep.kv_stream_stride = posd.ptr, csd.ptr, kc.ptr, vc.ptr, stride
    w4a(ti, td, sd, dev(ti, x), M, N, H, ep)
    q, k, v = (x.astype(f64) @ w64(*w) for w in ws)
    qgot = qb.download(f32, (M, qd))
    kcache, vcache = (c.download(f16, (M, nkv, max_seq, hd)) for c in (kc, vc))
    written = np.zeros((M, nkv, max_seq, hd), bool)
    for m in range(M):
        p = np.array([pos[m]], f32)
        written[m, :, pos[m]] = True
        qr = oracle.apply_rope(q[m].astype(f32).reshape(1, nh, 1, hd), p, theta).reshape(-1)
        kr = oracle.apply_rope(k[m].astype(f32).reshape(1, nkv, 1, hd), p, theta).reshape(nkv, hd)
        np.testing.assert_allclose(qgot[m], qr, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(kcache[m, :, pos[m]].astype(f32), kr, rtol=2e-3, atol=2e-3)
        np.testing.assert_allclose(vcache[m, :, pos[m]].astype(f32), v[m].reshape(nkv, hd), rtol=2e-3, atol=2e-3)
    assert not kcache[~written].any() and not vcache[~written].any()


@pytest.mark.parametrize("kind", ["resid+f16", "silu", "qkv64", "qkv128", "argmax"])
def test_other_epilogues(ti, oracle, kind):
    M, rng = 70, np.random.RandomState(7)
    if kind == "resid+f16":   # RESID_F32 in place, then STORE_F16
        K, N = 4096, 2064
        is_w4a(ti, M, N, K)
        td, sd, w, parts = weights(ti, K, N)
        x, r = rng.standard_normal((M, K)).astype(f16), rng.standard_normal((M, N)).astype(f32)
        xd, rd, yd = dev(ti, x), dev(ti, r), ti.DeviceBuffer(M * N * 2)
        w4a(ti, td, sd, xd, M, N, K, epilogue(ti, ti.EPI_RESID_F32, N, rd))
        assert_close(rd.download(f32, (M, N)) - r, x, w, parts, rel=5e-5)
        w4a(ti, td, sd, xd, M, N, K, epilogue(ti, ti.EPI_STORE_F16, N, yd))
        np.testing.assert_allclose(yd.download(f16, (M, N)).astype(f64), x.astype(f64) @ w, rtol=2e-3, atol=2e-3)
    elif kind == "silu":   # gate / up interleaved by ti_wpack_q1_host's row_map
        K, I = 2048, 1032
        is_w4a(ti, M, 2 * I, K)
        g, u = (q1_weight(rng, K, I)[:3] for _ in range(2))
        td, sd = pack(ti, [g + (0,), u + (8,)], n_total=2 * I, row_map=ti.ROWS_INTERLEAVE8)
        x, yd = rng.standard_normal((M, K)).astype(f16), ti.DeviceBuffer(M * I * 2)
        w4a(ti, td, sd, dev(ti, x), M, 2 * I, K, epilogue(ti, ti.EPI_SILU_MUL_F16, I, yd))
        gg, uu = x.astype(f64) @ w64(*g), x.astype(f64) @ w64(*u)
        np.testing.assert_allclose(yd.download(f16, (M, I)).astype(f64), uu * (gg / (1 + np.exp(-gg))), rtol=3e-3, atol=2e-3)
    elif kind.startswith("qkv"):
        qkv_case(ti, oracle, rng.standard_normal((M, 256)).astype(f16), int(kind[3:]))
    else:   # LOGITS_ARGMAX: columns 37 and 3000 are the same blocks, aligned with row 5 -- equal bit for bit
        K, V, lo, hi = 256, 4096, 37, 3000
        is_w4a(ti, M, V, K)
        q, d, m, _, _ = q1_weight(rng, K, V)
        x = rng.standard_normal((M, K)).astype(f16)
        q[:, lo] = q[:, hi] = np.where(x[5] > 0, 15, 0)
        d[:, lo] = d[:, hi] = d.max()
        m[:, lo] = m[:, hi] = (-7.5 * d.max()).astype(f16)
        td, sd = pack(ti, [(q, d, m, 0)])
        ld, am = ti.DeviceBuffer(M * V * 4), ti.DeviceBuffer(M * ti.ARGMAX_SLOTS * 8)
        am.zero()
        ctr = dev(ti, np.array([7], np.int32))
        ep = epilogue(ti, ti.EPI_LOGITS_ARGMAX, V, ld)
        ep.argmax, ep.step_ctr, ep.advance = am.ptr, ctr.ptr, 1
        w4a(ti, td, sd, dev(ti, x), M, V, K, ep)
        logits = ld.download(f32, (M, V))
        keys = am.download(np.uint64, (M, ti.ARGMAX_SLOTS)).max(axis=1)
        idx = (0xFFFFFFFF - (keys & 0xFFFFFFFF)).astype(np.int64)
        np.testing.assert_array_equal(idx, np.argmax(logits, axis=1))
        assert logits[5, lo] == logits[5, hi] == logits[5].max() and idx[5] == lo
        assert ctr.download(np.int32, (1,))[0] == 8
        np.testing.assert_allclose(logits, x.astype(f64) @ w64(q, d, m), rtol=1e-4, atol=1e-4)


def test_unaligned_x_falls_back_to_pieces(ti):   # x 2 bytes off a 16-byte boundary: TI_OK (fused pieces), no refusal
    M, K, N = 40, 384, 80
    td, sd, w, parts = weights(ti, K, N)
    x = np.random.RandomState(3).standard_normal((M, K)).astype(f16)
    xd = dev(ti, np.concatenate([x.reshape(-1), x.reshape(-1)[-1:]]))
    assert_close(store_f32(ti, td, sd, xd, M, N, K), x, w, parts)
    xd.upload(np.concatenate([x.reshape(-1)[:1], x.reshape(-1)]))   # the same rows from byte 2 on
    assert_close(store_f32(ti, td, sd, SimpleNamespace(ptr=xd.ptr + 2), M, N, K), x, w, parts)
