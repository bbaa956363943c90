"""gemv_kq_kernel (Q4_K super-blocks, 4 | BITS_G32 | BITS_KQ) through ti_gemm_wq_a16 against float64 x_fp16 @ W with
W = (float(d) sc) q - float(dmin) m in float64.  q runs through all 16 nibbles at every (k % 128, n % 16) position of
a tile, sc and m are drawn from 0..63 and d, dmin per (row, super-block).  Bar: the Q4_1 instance's fp32-summation
bound, 2e-5 |x| @ (|d sc q| + |dmin m|) + 1e-6, + 1e-3 of the same behind the rms_norm prologue (worst measured: 0.013)."""
import functools

import numpy as np
import pytest

import test_gpu_gemm_mx as mxt
from test_gpu_gemm_w8 import epilogue
from test_gpu_kernels import dev, gemm
from test_kq_pack import unpack

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64


def kq_weight(rng, K, N, amp=1.0):
    """(blocks, W, |d sc q| + |dmin m|): d about amp 1e-3, dmin about amp 8e-3 (weights up to about amp in size)."""
    k, n = np.arange(K)[:, None], np.arange(N)[None, :]
    q = ((rng.randint(0, 16, (128, 16))[k % 128, n % 16] + k // 128 + n // 16) % 16).astype(np.uint8)
    sc, m = (rng.randint(0, 64, (K // 32, N)).astype(np.uint8) for _ in range(2))
    d, dmin = ((rng.uniform(0.5, 2.0, (K // 256, N)) * s * amp).astype(f16) for s in (1e-3, 8e-3))
    return (q, sc, m, d, dmin) + dequant(q, sc, m, d, dmin)


def dequant(q, sc, m, d, dmin):
    pos = (d.astype(f64).repeat(8, axis=0) * sc).repeat(32, axis=0) * q
    neg = (dmin.astype(f64).repeat(8, axis=0) * m).repeat(32, axis=0)
    return pos - neg, np.abs(pos) + np.abs(neg)


@functools.lru_cache(maxsize=None)
def weights(ti, K, N):
    *blk, w, wa = kq_weight(np.random.RandomState(K + N), K, N)
    return tuple(dev(ti, a) for a in ti.wpack_kq(*blk)) + (w, wa)


def kq(ti, td, sd, xd, x_kind, M, N, K, ep, norm=None):
    gemm(ti, td, sd, 4 | ti.BITS_G32 | ti.BITS_KQ, xd, x_kind, K, M, N, K, ep, norm_d=norm)


def check(y, xa, w, wa, rel=2e-5):
    err, bound = np.abs(y.astype(f64) - xa.astype(f64) @ w), rel * (np.abs(xa.astype(f64)) @ wa) + 1e-6
    print(f"worst error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"max err {err.max()} vs bound {bound[err > bound][:4]}"


@pytest.mark.parametrize("M", [1, 2, 3, 16, 17, 40])
@pytest.mark.parametrize("K,N", [(K, N) for K in (256, 512, 768, 4096) for N in (16, 48)] + [(4096, 4096)])
def test_store_f32(ti, oracle, M, K, N):
    assert ti.gemm_kernel_name(4 | ti.BITS_G32 | ti.BITS_KQ, ti.X_F16, M, N, K).startswith("gemv_kq_kernel<")
    td, sd, w, wa = weights(ti, K, N)
    for kind, xd, nd, xa, rel in mxt.x_kinds(ti, oracle, np.random.RandomState(M), M, K):
        yd = dev(ti, np.full((M, N), -7.25, f32))
        kq(ti, td, sd, xd, kind, M, N, K, epilogue(ti, ti.EPI_STORE_F32, N, yd), nd)
        check(yd.download(f32, (M, N)), xa, w, wa, rel)


@pytest.mark.parametrize("which", ["weight", "minimum"])
def test_one_term_at_each_position(ti, which):
    """weight: column n holds one non-zero q per block, at position n, and m = 0 (the nibble -> k map of every lane
    slot).  minimum: sc = 0 and column n has one non-zero m, in sub-block n % 16 (the 6-bit field -> block map)."""
    K, N, M = 512, 32, 2
    rng = np.random.RandomState(9)
    q, sc, m, d, dmin, _, _ = kq_weight(rng, K, N)
    if which == "weight":
        q, m = np.where(np.arange(K)[:, None] % 32 == np.arange(N), np.maximum(q, 1), 0).astype(np.uint8), 0 * m
    else:
        sc, m = 0 * sc, np.where(np.arange(K // 32)[:, None] == np.arange(N) % 16, np.maximum(m, 1), 0).astype(np.uint8)
    td, sd = (dev(ti, a) for a in ti.wpack_kq(q, sc, m, d, dmin))
    x, yd = rng.standard_normal((M, K)).astype(f16), ti.DeviceBuffer(M * N * 4)
    kq(ti, td, sd, dev(ti, x), ti.X_F16, M, N, K, epilogue(ti, ti.EPI_STORE_F32, N, yd))
    check(yd.download(f32, (M, N)), x, *dequant(q, sc, m, d, dmin))


@pytest.mark.parametrize("M", [1, 3, 40])   # 1: the one-row instances (f16 x RESID, rms_norm x SILU / QKV / LOGITS)
@pytest.mark.parametrize("kind", ["resid", "silu", "qkv", "argmax"])
def test_other_epilogues(ti, oracle, monkeypatch, kind, M):
    """test_gpu_gemm_mx.py's epilogue cases at its bars (its check bounds by |x| @ |W|, no more than this file's) on
    Q4_K blocks: its generator, packer, launcher and cached weights are swapped for this file's, the blocks travelling
    where the MX codes do.  Its fp16-output cases (they pass an e_hi) get weights a quarter the size."""
    def weight(rng, K, N, e_hi=None):
        *blk, w, _ = kq_weight(rng, K, N, 0.25 if e_hi else 1.0)
        return tuple(blk), None, w
    monkeypatch.setattr(mxt, "mx_weight", weight)
    monkeypatch.setattr(mxt, "mx", kq)
    monkeypatch.setattr(mxt, "weights", lambda ti, K, N: weights(ti, K, N)[:3])
    monkeypatch.setattr(ti, "wpack_mx", lambda blk, _, *a: ti.wpack_kq(*blk, *a))
    mxt.test_other_epilogues(ti, oracle, kind, M)


def test_wsynth_device_blocks(ti):
    """ti_wsynth_device's seeded blocks decode to finite weights of about 1 / sqrt(K), and the kernel meets the bar on them."""
    K, N, M, BITS = 512, 48, 3, 4 | ti.BITS_G32 | ti.BITS_KQ
    L = ti.lib()
    td, sd = ti.DeviceBuffer(L.ti_wpack_tile_bytes(BITS, K, N)), ti.DeviceBuffer(L.ti_wpack_scale_bytes(BITS, K, N))
    ti.check(L.ti_wsynth_device(77, 3, K, N, N, BITS, 0, 0, td.ptr, sd.ptr, None))
    ti.sync()
    w, wa = dequant(*unpack(*(b.download(np.uint8, (b.nbytes,)) for b in (td, sd)), K, N))
    assert np.isfinite(w).all() and 0.5 / np.sqrt(K) < w.std() < 2 / np.sqrt(K) and abs(w.mean()) < 0.2 / np.sqrt(K)
    x, yd = np.random.RandomState(1).standard_normal((M, K)).astype(f16), ti.DeviceBuffer(M * N * 4)
    kq(ti, td, sd, dev(ti, x), ti.X_F16, M, N, K, epilogue(ti, ti.EPI_STORE_F32, N, yd))
    check(yd.download(f32, (M, N)), x, w, wa)
