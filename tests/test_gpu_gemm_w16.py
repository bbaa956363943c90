"""gemm_w16_kernel (fp16 weights, fp16 rows, 17 .. TI_GEMM_MAX_ROWS rows) through ti_gemm_wq_a16 against float64,
x_fp16 @ W_fp16.  STORE_F32 runs test_gpu_gemm_w8.py's edges of M, K and N; that grid plans one tile per wave only,
and 4 k-waves only in 64-row workgroups, so PLANS adds the other instances the plan can choose.  Bar:
assert_close_dot's default rel 2e-5, test_gemm_store's bar for bits 16 (fp32 summation order only: an fp32 chain in
8-k pieces uses at most 0.45 % of it on these inputs); plus a guard behind the output and a second launch giving the
same bits.  The other epilogues run M = 70 at test_gpu_gemm_w8.py's bars.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import kv8_ref as Q
from test_gpu_gemm_w8 import GUARD, epilogue
from test_gpu_kernels import assert_close_dot, deq, dev, gemm

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64


@functools.lru_cache(maxsize=None)
def weights(ti, oracle, K, N):
    """(tiles on the device, W float64 [K][N]) of one seeded weight, made once."""
    w = (np.random.RandomState(K + N).standard_normal((K, N)) * 0.03).astype(f32)
    wf = deq(oracle, w, 16).astype(f64)
    wf.setflags(write=False)
    return dev(ti, ti.wpack_host(w, 16)[0]), wf


def is_w16(ti, M, N, K):
    assert ti.gemm_kernel_name(16, ti.X_F16, M, N, K) == "gemm_w16_kernel" and ti.gemm_w16_rows(M, N, K)
    plan = ti.gemm_w16_plan(M, N, K)
    print(f"M={M} N={N} K={K}: (rb, tpw, kwaves, grid) = {plan}")
    return plan


def w16(ti, td, xd, M, N, K, ep):
    gemm(ti, td, None, 16, xd, ti.X_F16, K, M, N, K, ep)


GRID = [(M, K, N, None) for M in (17, 33, 64, 65, 130) for K in (128, 384, 4096) for N in (16, 80, 2064)]
PLANS = [(17, 128, 33280, (2, 2, 1)), (130, 384, 11264, (4, 2, 1)), (17, 512, 80, (2, 1, 4))]   # tpw 2: a second round of workgroups otherwise


@pytest.mark.parametrize("M,K,N,plan", GRID + PLANS)
def test_store_f32(ti, oracle, M, K, N, plan):
    assert is_w16(ti, M, N, K)[:3] == plan or plan is None
    td, wf = weights(ti, oracle, K, N)
    x = np.random.RandomState(M).standard_normal((M, K)).astype(f16)
    xd, outs = dev(ti, x), []
    for _ in range(2):
        yd = dev(ti, np.full(M * N + GUARD, -7.25, f32))
        w16(ti, td, xd, M, N, K, epilogue(ti, ti.EPI_STORE_F32, N, yd))
        outs.append(yd.download(f32, (M * N + GUARD,)))
        yd.free()
    assert np.all(outs[0][M * N:] == -7.25), "guard behind the output overwritten"
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "a second launch gives other bits"
    assert_close_dot(outs[0][:M * N].reshape(M, N), x.astype(f64) @ wf, x.astype(f32), wf)


@pytest.mark.parametrize("K,N", [(512, 80), (4096, 2064)])
def test_resid_in_place_and_store_f16(ti, oracle, K, N):
    M = 70
    is_w16(ti, M, N, K)
    td, wf = weights(ti, oracle, K, N)
    rng = np.random.RandomState(7)
    x = rng.standard_normal((M, K)).astype(f16)
    ref, xd = x.astype(f64) @ wf, dev(ti, x)
    r = rng.standard_normal((M, N)).astype(f32)
    rd = dev(ti, r)
    w16(ti, td, xd, M, N, K, epilogue(ti, ti.EPI_RESID_F32, N, rd))
    assert_close_dot(rd.download(f32, (M, N)) - r, ref, x.astype(f32), wf, rel=5e-5)
    yd = ti.DeviceBuffer(M * N * 2)
    w16(ti, td, xd, M, N, K, epilogue(ti, ti.EPI_STORE_F16, N, yd))
    np.testing.assert_allclose(yd.download(f16, (M, N)).astype(f64), ref, rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("K,I", [(256, 40), (2048, 1032)])
def test_silu_mul_interleaved(ti, oracle, K, I):
    M = 70
    is_w16(ti, M, 2 * I, K)
    rng = np.random.RandomState(31)
    g, u = ((rng.standard_normal((K, I)) * 0.05).astype(f32) for _ in range(2))
    x = rng.standard_normal((M, K)).astype(f16)
    tiles, _ = ti.wpack_host(g, 16, n_total=2 * I, row_map=ti.ROWS_INTERLEAVE8, row_offset=0)
    ti.wpack_host(u, 16, n_total=2 * I, row_map=ti.ROWS_INTERLEAVE8, row_offset=8, tiles=tiles)
    yd = ti.DeviceBuffer(M * I * 2)
    w16(ti, dev(ti, tiles), dev(ti, x), M, 2 * I, K, epilogue(ti, ti.EPI_SILU_MUL_F16, I, yd))
    gg, uu = (x.astype(f64) @ deq(oracle, w, 16).astype(f64) for w in (g, u))
    np.testing.assert_allclose(yd.download(f16, (M, I)).astype(f64), uu * (gg / (1 + np.exp(-gg))), rtol=3e-3, atol=2e-3)


@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 4, 2)])
def test_qkv_rope_kv_append(ti, oracle, hd, nh, nkv):
    """Per-row positions, one cache per row (GQA): the fp16 cache against float64, then the same call into an
    e4m3 cache, whose bytes kv8_ref.append_ok judges against the fp16 rows."""
    M, H, max_seq, theta = 70, 256, 32, 10000.0
    qd, kvd = nh * hd, nkv * hd
    N = qd + 2 * kvd
    is_w16(ti, M, N, H)
    rng = np.random.RandomState(41 + hd)
    ws = [(rng.standard_normal((H, n)) * 0.05).astype(f32) for n in (qd, kvd, kvd)]
    tiles = None
    for w, off in zip(ws, (0, qd, qd + kvd)):
        tiles, _ = ti.wpack_host(w, 16, n_total=N, row_offset=off, tiles=tiles)
    x = rng.standard_normal((M, H)).astype(f16)
    pos = rng.randint(0, max_seq, size=M).astype(np.int32)
    stride = nkv * max_seq * hd
    td, xd, posd = dev(ti, tiles), dev(ti, x), dev(ti, pos)
    csd = dev(ti, ti.rope_table(np.arange(max_seq, dtype=f32), hd, theta))
    res = {}
    for fp8 in (0, 1):
        qb, kc, vc = ti.DeviceBuffer(M * qd * 4), ti.DeviceBuffer(M * stride * 2), ti.DeviceBuffer(M * stride * 2)
        kc.zero(), vc.zero()
        ep = epilogue(ti, ti.EPI_QKV_ROPE_KV, qd, qb)
        ep.q_dim, ep.kv_dim, ep.head_dim, ep.max_seq, ep.kv_fp8 = qd, kvd, hd, max_seq, fp8
        ep.pos, ep.rope_cs, ep.k_cache, ep.v_cache, ep.kv_stream_stride = posd.ptr, csd.ptr, kc.ptr, vc.ptr, stride
        w16(ti, td, xd, M, N, H, ep)
        dt = np.uint8 if fp8 else f16
        res[fp8] = [qb.download(f32, (M, qd))] + [c.download(dt, (M * stride * 2 // np.dtype(dt).itemsize,)) for c in (kc, vc)]
    q, k, v = (x.astype(f64) @ deq(oracle, w, 16).astype(f64) for w in ws)
    qgot = res[0][0]
    kcache, vcache = (res[0][i].reshape(M, nkv, max_seq, hd) for i in (1, 2))
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
    assert np.array_equal(res[1][0], qgot)
    for i, name in ((1, "K"), (2, "V")):
        h = res[0][i].reshape(M, nkv, max_seq, hd)
        assert not res[1][i][M * stride:].any(), f"{name}: bytes past the e4m3 cache written"
        b = res[1][i][:M * stride].reshape(M, nkv, max_seq, hd)
        assert not b[~written].any(), f"{name}: e4m3 cache written outside the appended rows"
        is_nb, must, equal = Q.append_ok(b[written], h[written])
        assert is_nb.all() and not (must & ~equal).any() and must.mean() > 0.9, name


def test_logits_argmax_lowest_index_wins(ti, oracle):
    """Columns 37 and 3000 carry the same weights, aligned with row 5: its two top logits are equal bit for bit."""
    M, K, V, lo, hi = 70, 256, 4096, 37, 3000
    is_w16(ti, M, V, K)
    rng = np.random.RandomState(51)
    w = (rng.standard_normal((K, V)) * 0.05).astype(f32)
    x = rng.standard_normal((M, K)).astype(f16)
    w[:, lo] = w[:, hi] = 0.5 * x[5].astype(f32) / np.linalg.norm(x[5].astype(f32))
    ld, am = ti.DeviceBuffer(M * V * 4), ti.DeviceBuffer(M * ti.ARGMAX_SLOTS * 8)
    am.zero()
    ctr = dev(ti, np.array([7], np.int32))
    ep = epilogue(ti, ti.EPI_LOGITS_ARGMAX, V, ld)
    ep.argmax, ep.step_ctr, ep.advance = am.ptr, ctr.ptr, 1
    w16(ti, dev(ti, ti.wpack_host(w, 16)[0]), dev(ti, x), M, V, K, ep)
    logits = ld.download(f32, (M, V))
    keys = am.download(np.uint64, (M, ti.ARGMAX_SLOTS)).max(axis=1)
    idx = (0xFFFFFFFF - (keys & 0xFFFFFFFF)).astype(np.int64)
    np.testing.assert_array_equal(idx, np.argmax(logits, axis=1))
    assert logits[5, lo] == logits[5, hi] == logits[5].max() and idx[5] == lo
    assert ctr.download(np.int32, (1,))[0] == 8
    np.testing.assert_allclose(logits, x.astype(f64) @ deq(oracle, w, 16).astype(f64), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("ldx,packed", [(132, 0), (128, 1)], ids=["unaligned-ldx", "out_packed"])
def test_refusals(ti, ldx, packed):
    """Nothing else serves fp16 weights above 16 rows: what the kernel cannot take is TI_ERR_UNSUPPORTED."""
    M, K, N = 20, 128, 128
    td, xd, yd = ti.DeviceBuffer(K * N * 2), ti.DeviceBuffer(M * ldx * 2), ti.DeviceBuffer(M * N * 2)
    ep = epilogue(ti, ti.EPI_STORE_F16, N, yd)
    ep.out_packed = packed
    rc = ti.lib().ti_gemm_wq_a16(td.ptr, None, 16, xd.ptr, ti.X_F16, ldx, None, 1e-5, M, N, K, C.byref(ep), None)
    assert rc == 3, ti.lib().ti_last_error()   # TI_ERR_UNSUPPORTED
