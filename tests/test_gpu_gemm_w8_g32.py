"""gemm_w8_kernel's group-32 instance (GGUF Q8_0 blocks, 8 | BITS_G32, fp16 rows above 16) through ti_gemm_wq_a16
against float64 x_fp16 @ (d q) with exact blocks: g32_weight draws every block scale per (block, column) from
U(0.5, 1.5) amp, so a scale of the wrong block or output is a 10-50 % error.  Shapes and bars are
test_gpu_gemm_w8.py's (rel 2e-5: fp32 summation order only, what Q8_0 meets at 40 rows on the fused pieces)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_g32 import assert_close_dot, g32_weight, pack_g32
from test_gpu_gemm_w8 import GUARD, epilogue
from test_gpu_kernels import dev, gemm

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64


@functools.lru_cache(maxsize=None)
def weights(ti, K, N):
    q, d, w = g32_weight(np.random.RandomState(K + N), K, N, 8)
    return pack_g32(ti, q, d, 8) + (w,)


def case(ti, M, K, N):
    bits = 8 | ti.BITS_G32
    assert ti.gemm_kernel_name(bits, ti.X_F16, M, N, K) == "gemm_w8_kernel"
    print(f"M={M} N={N} K={K}: (rb, tpw, kwaves, grid) = {ti.gemm_w8_plan(M, N, K, bits=bits)}")
    return (bits,) + weights(ti, K, N)


def store_f32(ti, bits, td, sd, xd, M, K, N):
    yd = dev(ti, np.full(M * N + GUARD, -7.25, f32))
    gemm(ti, td, sd, bits, xd, ti.X_F16, K, M, N, K, epilogue(ti, ti.EPI_STORE_F32, N, yd))
    y = yd.download(f32, (M * N + GUARD,))
    yd.free()
    assert np.all(y[M * N:] == -7.25), "guard behind the output overwritten"
    return y[:M * N].reshape(M, N)


@pytest.mark.parametrize("M,K,N", [(M, K, N) for M in (17, 33, 64, 65, 130) for K in (128, 384, 4096)
                                   for N in (16, 80, 2064)] + [(17, 128, 33024), (130, 384, 11008)])
def test_store_f32(ti, M, K, N):
    bits, td, sd, w = case(ti, M, K, N)
    x = np.random.RandomState(M).standard_normal((M, K)).astype(f16)
    xd = dev(ti, x)
    y, again = (store_f32(ti, bits, td, sd, xd, M, K, N) for _ in range(2))
    assert np.array_equal(y.view(np.uint32), again.view(np.uint32)), "a second launch gives other bits"
    assert_close_dot(y, x.astype(f32), w)


def test_resid_in_place_and_store_f16(ti):
    M, K, N = 70, 4096, 2064
    bits, td, sd, w = case(ti, M, K, N)
    rng = np.random.RandomState(7)
    x, r = rng.standard_normal((M, K)).astype(f16), rng.standard_normal((M, N)).astype(f32)
    xd, rd, yd = dev(ti, x), dev(ti, r), ti.DeviceBuffer(M * N * 2)
    gemm(ti, td, sd, bits, xd, ti.X_F16, K, M, N, K, epilogue(ti, ti.EPI_RESID_F32, N, rd))
    assert_close_dot(rd.download(f32, (M, N)) - r, x.astype(f32), w, rel=5e-5)
    gemm(ti, td, sd, bits, xd, ti.X_F16, K, M, N, K, epilogue(ti, ti.EPI_STORE_F16, N, yd))
    np.testing.assert_allclose(yd.download(f16, (M, N)).astype(f64), x.astype(f64) @ w.astype(f64), rtol=2e-3, atol=2e-3)


def test_unaligned_x_falls_back_to_pieces(ti):   # x 2 bytes off a 16-byte boundary: TI_OK (fused pieces), no refusal
    M, K, N = 40, 384, 80
    bits, td, sd, w = case(ti, M, K, N)
    x = np.random.RandomState(3).standard_normal((M, K)).astype(f16)
    xd = dev(ti, np.concatenate([x.reshape(-1), x.reshape(-1)[-1:]]))
    assert_close_dot(store_f32(ti, bits, td, sd, xd, M, K, N), x.astype(f32), w)
    xd.upload(np.concatenate([x.reshape(-1)[:1], x.reshape(-1)]))   # the same rows from byte 2 on
    assert_close_dot(store_f32(ti, bits, td, sd, SimpleNamespace(ptr=xd.ptr + 2), M, K, N), x.astype(f32), w)
