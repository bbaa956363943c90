"""The TI_EPI_QKV_ROPE_KV epilogue writing an e4m3 cache (ti_epilogue.kv_fp8 = 1) on the four kernels that
append K / V -- the fused kernel (M = 1), the register-fragment batched kernel (gemv_mbr_kernel, 8 int4
rows), the batched-rows kernel (packed int4 rows) and the tile kernel (int4 rows from 65 on) -- and
ti_fill_kv_uniform_f8.

Each case runs ti_gemm_wq_a16 twice on the same inputs, kv_fp8 0 and 1, into caches pre-filled with 0xA5:
  q is bit-identical between the two calls;
  every cache byte the call does not own keeps 0xA5 (the e4m3 cache sits in a buffer of the fp16 cache's
  size, so a store at the fp16 element size would land inside the buffer and show);
  per written element, with h the fp16-cache value of the same element: the epilogue converts its fp32
  value x, and |x - h| <= 2^-11 |h|, so the byte decodes to one of the two e4m3 neighbours of clamp(h), and
  equals kv8_ref.quantize(h) whenever h is further than 2^-10 |h| from the midpoint of those neighbours
  (kv8_ref.append_ok; no element is left out).
The weights carry columns scaled up (values beyond +-448: the clamp) and down (e4m3 subnormals and zero).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import kv8_ref as Q

pytestmark = pytest.mark.gpu

f16, f32 = np.float16, np.float32
PAT = 0xA5
K_IN = 512
THETA = 10000.0


def dev(ti, a):
    return ti.DeviceBuffer.from_array(np.ascontiguousarray(a))


def patterned(ti, nbytes):
    b = ti.DeviceBuffer(nbytes)
    ti.check(ti.lib().ti_memset(b.ptr, PAT, nbytes, None))
    return b


# (label, bits, M, x kind, kernel name prefix)
KERNELS = [("fused-int4", 4, 1, "f16", "gemv_wq_kernel"), ("fused-int8", 8, 1, "f16", "gemv_wq_kernel"),
           ("mbr-int4", 4, 8, "f16", "gemv_mbr_kernel"),
           ("rows-int4", 4, 32, "packed", "gemm_rows_kernel"), ("tile-int4", 4, 128, "f16", "gemm_tile_kernel")]
SHAPES = [(4, 2, 64), (2, 2, 128)]      # heads, kv_heads, head_dim


@pytest.mark.parametrize("shared", [False, True], ids=["per-stream", "stride0"])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES, ids=["h4-kv2-hd64", "h2-kv2-hd128"])
@pytest.mark.parametrize("label,bits,M,xk,kernel", KERNELS, ids=[k[0] for k in KERNELS])
def test_append_e4m3(ti, label, bits, M, xk, kernel, nh, nkv, hd, shared):
    L = ti.lib()
    qd, kvd = nh * hd, nkv * hd
    N = qd + 2 * kvd
    max_seq = 160
    x_kind = ti.X_F16_PACKED if xk == "packed" else ti.X_F16
    assert ti.gemm_kernel_name(bits, x_kind, M, N, K_IN).startswith(kernel)
    rng = np.random.RandomState(1000 * M + hd + bits)
    ws = [(rng.standard_normal((K_IN, n)) * 0.5).astype(f32) for n in (qd, kvd, kvd)]
    for w in ws[1:]:
        w[:, -8:] *= 60.0        # |y| far beyond 448: the clamp
        w[:, :8] *= 1e-3         # |y| around 2^-9: e4m3 subnormals and zero
    tiles = scales = None
    for w, off in zip(ws, (0, qd, qd + kvd)):
        tiles, scales = ti.wpack_host(w, bits, n_total=N, row_offset=off, tiles=tiles, scales=scales)
    x = rng.standard_normal((M, K_IN)).astype(f16)
    pos = (rng.permutation(max_seq)[:M] if shared else rng.randint(0, max_seq, size=M)).astype(np.int32)
    cs = ti.rope_table(np.arange(max_seq, dtype=f32), hd, THETA)
    S = 1 if shared else M
    slot = nkv * max_seq * hd                       # elements of one stream's cache
    stride = 0 if shared else slot
    xd = dev(ti, ti.pack_rows(x) if xk == "packed" else x)
    td, sd, posd, csd = dev(ti, tiles), dev(ti, scales), dev(ti, pos), dev(ti, cs)
    res = {}
    for fp8 in (0, 1):
        qbuf = patterned(ti, M * qd * 4)
        kc, vc = patterned(ti, S * slot * 2), patterned(ti, S * slot * 2)      # the fp16 size for both formats
        ep = ti.Epilogue()
        ep.kind, ep.ldo, ep.out = ti.EPI_QKV_ROPE_KV, qd, qbuf.ptr
        ep.q_dim, ep.kv_dim, ep.head_dim, ep.max_seq = qd, kvd, hd, max_seq
        ep.pos, ep.rope_cs, ep.k_cache, ep.v_cache, ep.kv_stream_stride = posd.ptr, csd.ptr, kc.ptr, vc.ptr, stride
        ep.kv_fp8 = fp8
        ti.check(L.ti_gemm_wq_a16(td.ptr, sd.ptr, bits, xd.ptr, x_kind, K_IN, None, 1e-5, M, N, K_IN, C.byref(ep), None))
        ti.sync()
        res[fp8] = (qbuf.download(np.uint32, (M, qd)), kc.download(np.uint8, (S * slot * 2,)),
                    vc.download(np.uint8, (S * slot * 2,)))
        for b in (qbuf, kc, vc):
            b.free()
    assert np.array_equal(res[0][0], res[1][0]), "q differs between kv_fp8 0 and 1"
    written = np.zeros((S, nkv, max_seq, hd), bool)
    for m in range(M):
        written[m if not shared else 0, :, pos[m]] = True
    n_clamped = n_sub = 0
    for name, i in (("K", 1), ("V", 2)):
        h = res[0][i].view(f16).reshape(S, nkv, max_seq, hd)
        raw8 = res[1][i]
        assert np.all(raw8[S * slot:] == PAT), f"{name}: bytes past the e4m3 cache written (fp16-sized stores?)"
        b = raw8[:S * slot].reshape(S, nkv, max_seq, hd)
        assert np.all(b[~written] == PAT), f"{name}: e4m3 cache written outside the appended rows"
        assert np.all(h.view(np.uint16)[~written] == PAT * 0x0101), f"{name}: fp16 cache written outside the rows"
        hw, bw = h[written], b[written]
        assert np.all(np.isfinite(hw))
        is_nb, must, equal = Q.append_ok(bw, hw)
        assert is_nb.all(), (f"{name}: {np.count_nonzero(~is_nb)} bytes are no e4m3 neighbour of the fp16 value, e.g. "
                             f"h {hw[~is_nb][:4].tolist()} -> {[hex(v) for v in bw[~is_nb][:4]]}")
        bad = must & ~equal
        assert not bad.any(), (f"{name}: {np.count_nonzero(bad)} bytes differ from quantize(h) away from a tie, e.g. "
                               f"h {hw[bad][:4].tolist()} -> {[hex(v) for v in bw[bad][:4]]}, want "
                               f"{[hex(v) for v in Q.quantize(hw[bad][:4])]}")
        assert must.mean() > 0.9                   # the exact comparison covers nearly every element
        n_clamped += int(np.count_nonzero(np.abs(hw.astype(f32)) > 448))
        n_sub += int(np.count_nonzero(np.abs(hw.astype(f32)) < 2.0 ** -6))
    assert n_clamped > 0 and n_sub > 0             # the inputs reach the clamp and the subnormals


@pytest.mark.parametrize("kvh,hd", [(2, 64), (3, 128)])
def test_fill_kv_uniform_f8(ti, kvh, hd):
    """ti_fill_kv_uniform_f8: exactly quantize() of the fp16 fill of the same seed; n = 37 of 64 rows, the
    rest (and the second half of an fp16-sized buffer) untouched."""
    L = ti.lib()
    n, max_seq, seed, tid = 37, 64, 77, 0x100003
    elems = kvh * max_seq * hd
    a, b = patterned(ti, elems * 2), patterned(ti, elems * 2)
    ti.check(L.ti_fill_kv_uniform(seed, tid, n, kvh, hd, max_seq, a.ptr, None))
    ti.check(L.ti_fill_kv_uniform_f8(seed, tid, n, kvh, hd, max_seq, b.ptr, None))
    ti.sync()
    h = a.download(f16, (kvh, max_seq, hd))
    raw = b.download(np.uint8, (elems * 2,))
    assert np.all(raw[elems:] == PAT)
    got = raw[:elems].reshape(kvh, max_seq, hd)
    assert np.all(got[:, n:] == PAT) and np.all(h.view(np.uint16)[:, n:] == PAT * 0x0101)
    assert np.array_equal(got[:, :n], Q.quantize(h[:, :n]))
    assert len(np.unique(got[:, :n])) > 100        # U(-1, 1): most codes below 1 occur
