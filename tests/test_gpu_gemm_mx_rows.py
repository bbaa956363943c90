"""gemm_mx_kernel (MXFP4 blocks, 4 | BITS_G32 | BITS_MX, fp16 rows above 16, the route switched on by
gemm_set_mx_rows) through ti_gemm_wq_a16 against float64 x_fp16 @ W with W the exactly dequantized blocks of
test_gpu_gemm_mx.py's mx_weight (e in [100, 140] per block, the codes cycling through all 16 nibbles at every tile
position).  STORE_F32 runs test_gpu_gemm_w8.py's edges of M, K and N plus PLANS, the shapes whose plan picks the
instances that grid does not reach.  Bar: the fused MX kernel's own, 2e-5 |x| @ |W| + 1e-6 (fp32 summation only: the
per-block arithmetic is the same, the k-wave sum is gemm_w4a_kernel's, which meets this bar); plus a guard behind the
output and a second launch giving the same bits.  The other epilogues run M = 70 at test_gpu_gemm_w8.py's bars, the
fp16-output ones with e <= 124 and LOGITS_ARGMAX's logits at the store bar (as test_gpu_gemm_mx.py: with e up to 140 an
absolute bar says nothing).  The switch is on for this module only and restored behind it."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_gemm_mx import E2M1, mx_weight
from test_gpu_gemm_w8 import GUARD, epilogue
from test_gpu_kernels import dev, gemm

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64


@pytest.fixture(scope="module", autouse=True)
def mx_rows_on(ti):
    before = ti.gemm_set_mx_rows(True)
    yield
    ti.gemm_set_mx_rows(before)


def pack(ti, blocks, n_total=None, row_map=0):
    """Device (tiles, scale bytes) of MX weights [(codes, e, row_offset), ..] packed into N_total outputs."""
    t = s = None
    for codes, e, off in blocks:
        t, s = ti.wpack_mx(codes, e, n_total or codes.shape[1], row_map, off, t, s)
    return dev(ti, t), dev(ti, s)


@functools.lru_cache(maxsize=None)
def weights(ti, K, N):
    """(tiles, scales on the device, W float64) of one seeded weight, made once."""
    codes, e, w = mx_weight(np.random.RandomState(K + N), K, N)
    return pack(ti, [(codes, e, 0)]) + (w,)


def is_mx(ti, M, N, K):
    assert ti.gemm_kernel_name(4 | ti.BITS_G32 | ti.BITS_MX, ti.X_F16, M, N, K) == "gemm_mx_kernel"
    plan = ti.gemm_mx_plan(M, N, K)
    print(f"M={M} N={N} K={K}: (rb, tpw, kwaves, grid) = {plan}")
    return plan


def mx(ti, td, sd, xd, M, N, K, ep):
    gemm(ti, td, sd, 4 | ti.BITS_G32 | ti.BITS_MX, xd, ti.X_F16, K, M, N, K, ep)


def store_f32(ti, td, sd, xd, M, N, K):
    yd = dev(ti, np.full(M * N + GUARD, -7.25, f32))
    mx(ti, td, sd, xd, M, N, K, epilogue(ti, ti.EPI_STORE_F32, N, yd))
    y = yd.download(f32, (M * N + GUARD,))
    yd.free()
    assert np.all(y[M * N:] == -7.25), "guard behind the output overwritten"
    return y[:M * N].reshape(M, N)


def assert_close(y, x, w, rel=2e-5):
    err, bound = np.abs(y.astype(f64) - x.astype(f64) @ w), rel * (np.abs(x.astype(f64)) @ np.abs(w)) + 1e-6
    print(f"worst error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"max err {err.max()} vs bound {bound[err > bound][:4]}"


GRID = [(M, K, N, None) for M in (17, 33, 64, 65, 130) for K in (128, 384, 4096) for N in (16, 80, 2064)]
PLANS = [(17, 128, 33280, (2, 2, 1)), (130, 384, 11264, (4, 2, 1)), (17, 512, 80, (2, 1, 4)), (130, 512, 4096, (4, 1, 2))]


@pytest.mark.parametrize("M,K,N,plan", GRID + PLANS)
def test_store_f32(ti, M, K, N, plan):
    assert is_mx(ti, M, N, K)[:3] == plan or plan is None
    td, sd, w = weights(ti, K, N)
    x = np.random.RandomState(M).standard_normal((M, K)).astype(f16)
    xd = dev(ti, x)
    y, again = (store_f32(ti, td, sd, xd, M, N, K) for _ in range(2))
    assert np.array_equal(y.view(np.uint32), again.view(np.uint32)), "a second launch gives other bits"
    assert_close(y, x, w)


def test_one_weight_per_block_at_each_position(ti):
    """Column n holds one non-zero weight per block, at position n: the nibble -> k mapping of every lane slot."""
    K, N, M = 256, 32, 17
    rng = np.random.RandomState(9)
    codes, e = np.zeros((K, N), np.uint8), rng.randint(100, 141, (K // 32, N)).astype(np.uint8)
    for n in range(N):
        codes[n::32, n] = rng.randint(1, 8, K // 32) | rng.choice([0, 8], K // 32)
    is_mx(ti, M, N, K)
    td, sd = pack(ti, [(codes, e, 0)])
    x = rng.standard_normal((M, K)).astype(f16)
    assert_close(store_f32(ti, td, sd, dev(ti, x), M, N, K), x, E2M1[codes] * np.exp2(e.astype(f64) - 127).repeat(32, axis=0))


def qkv_case(ti, oracle, x, hd):
    """QKV_ROPE_KV, per-row positions, GQA, one fp16 cache per row: q, the appended rows, nothing else written."""
    (M, H), nh, nkv, max_seq, theta = x.shape, 4, 2, 32, 10000.0
    qd, kvd = nh * hd, nkv * hd
    N, rng = qd + 2 * kvd, np.random.RandomState(41 + hd)
    is_mx(ti, M, N, H)
    ws = [mx_weight(rng, H, n, 124) for n in (qd, kvd, kvd)]
    td, sd = pack(ti, [w[:2] + (off,) for w, off in zip(ws, (0, qd, qd + kvd))], n_total=N)
    pos, stride = rng.randint(0, max_seq, size=M).astype(np.int32), nkv * max_seq * hd
    qb, kc, vc = ti.DeviceBuffer(M * qd * 4), ti.DeviceBuffer(M * stride * 2), ti.DeviceBuffer(M * stride * 2)
    kc.zero(), vc.zero()
    posd, csd = dev(ti, pos), dev(ti, ti.rope_table(np.arange(max_seq, dtype=f32), hd, theta))
    ep = epilogue(ti, ti.EPI_QKV_ROPE_KV, qd, qb)
    ep.q_dim, ep.kv_dim, ep.head_dim, ep.max_seq, ep.kv_fp8 = qd, kvd, hd, max_seq, 0
    ep.pos, ep.rope_cs, ep.k_cache, ep.v_cache, ep.kv_stream_stride = posd.ptr, csd.ptr, kc.ptr, vc.ptr, stride
    mx(ti, td, sd, dev(ti, x), M, N, H, ep)
    q, k, v = (x.astype(f64) @ w[2] for w in ws)
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
        is_mx(ti, M, N, K)
        codes, e, w = mx_weight(rng, K, N, 124)
        td, sd = pack(ti, [(codes, e, 0)])
        x, r = rng.standard_normal((M, K)).astype(f16), rng.standard_normal((M, N)).astype(f32)
        xd, rd, yd = dev(ti, x), dev(ti, r), ti.DeviceBuffer(M * N * 2)
        mx(ti, td, sd, xd, M, N, K, epilogue(ti, ti.EPI_RESID_F32, N, rd))
        assert_close(rd.download(f32, (M, N)) - r, x, w, rel=5e-5)
        mx(ti, td, sd, xd, M, N, K, epilogue(ti, ti.EPI_STORE_F16, N, yd))
        np.testing.assert_allclose(yd.download(f16, (M, N)).astype(f64), x.astype(f64) @ w, rtol=2e-3, atol=2e-3)
    elif kind == "silu":   # gate / up interleaved by ti_wpack_mx_host's row_map
        K, I = 2048, 1032
        is_mx(ti, M, 2 * I, K)
        g, u = (mx_weight(rng, K, I, 124) for _ in range(2))
        td, sd = pack(ti, [g[:2] + (0,), u[:2] + (8,)], n_total=2 * I, row_map=ti.ROWS_INTERLEAVE8)
        x, yd = rng.standard_normal((M, K)).astype(f16), ti.DeviceBuffer(M * I * 2)
        mx(ti, td, sd, dev(ti, x), M, 2 * I, K, epilogue(ti, ti.EPI_SILU_MUL_F16, I, yd))
        gg, uu = x.astype(f64) @ g[2], x.astype(f64) @ u[2]
        np.testing.assert_allclose(yd.download(f16, (M, I)).astype(f64), uu * (gg / (1 + np.exp(-gg))), rtol=3e-3, atol=2e-3)
    elif kind.startswith("qkv"):
        qkv_case(ti, oracle, rng.standard_normal((M, 256)).astype(f16), int(kind[3:]))
    else:   # LOGITS_ARGMAX: columns 37 and 3000 are the same blocks, aligned with row 5 -- equal bit for bit
        K, V, lo, hi = 256, 4096, 37, 3000
        is_mx(ti, M, V, K)
        codes, e, _ = mx_weight(rng, K, V)
        x = rng.standard_normal((M, K)).astype(f16)
        codes[:, lo] = codes[:, hi] = np.where(x[5] > 0, 7, 15)   # +6 / -6
        e[:, lo] = e[:, hi] = e.max()
        td, sd = pack(ti, [(codes, e, 0)])
        ld, am = ti.DeviceBuffer(M * V * 4), ti.DeviceBuffer(M * ti.ARGMAX_SLOTS * 8)
        am.zero()
        ctr = dev(ti, np.array([7], np.int32))
        ep = epilogue(ti, ti.EPI_LOGITS_ARGMAX, V, ld)
        ep.argmax, ep.step_ctr, ep.advance = am.ptr, ctr.ptr, 1
        mx(ti, td, sd, dev(ti, x), M, V, K, ep)
        logits = ld.download(f32, (M, V))
        keys = am.download(np.uint64, (M, ti.ARGMAX_SLOTS)).max(axis=1)
        idx = (0xFFFFFFFF - (keys & 0xFFFFFFFF)).astype(np.int64)
        np.testing.assert_array_equal(idx, np.argmax(logits, axis=1))
        assert logits[5, lo] == logits[5, hi] == logits[5].max() and idx[5] == lo
        assert ctr.download(np.int32, (1,))[0] == 8
        assert_close(logits, x, E2M1[codes] * np.exp2(e.astype(f64) - 127).repeat(32, axis=0))


def test_fallbacks_run_the_pieces(ti):
    """x 2 bytes off a 16-byte boundary: TI_OK (fused pieces), no refusal; the switch off: the pieces by name too."""
    M, K, N, BITS = 40, 384, 80, 4 | ti.BITS_G32 | ti.BITS_MX
    td, sd, w = weights(ti, K, N)
    x = np.random.RandomState(3).standard_normal((M, K)).astype(f16)
    xd = dev(ti, np.concatenate([x.reshape(-1), x.reshape(-1)[-1:]]))
    assert_close(store_f32(ti, td, sd, xd, M, N, K), x, w)
    xd.upload(np.concatenate([x.reshape(-1)[:1], x.reshape(-1)]))   # the same rows from byte 2 on
    assert_close(store_f32(ti, td, sd, SimpleNamespace(ptr=xd.ptr + 2), M, N, K), x, w)
    assert ti.gemm_set_mx_rows(False) is True
    try:
        assert ti.gemm_kernel_name(BITS, ti.X_F16, M, N, K).startswith("gemv_mx_kernel<")
        assert_close(store_f32(ti, td, sd, dev(ti, x), M, N, K), x, w)
    finally:
        ti.gemm_set_mx_rows(True)
