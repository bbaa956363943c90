"""gemv_mbr_kernel<1, NTL>, the kernel every projection of an int4 engine takes at 3..16 streams, at
every tile count per workgroup (NTL 1..8, with the ragged NTL / NTL - 1 split), its K edges and
every epilogue, through the ti_hip.h C-ABI against a float64 reference.

Every case first asserts the kernel (ti_gemm_kernel_name) and the plan (ti_gemm_mb_plan: workgroups
and tiles per workgroup, and from them how many workgroups hold NTL - 1 and NTL tiles) it exists
for, on 256 CUs: a changed dispatch fails the case instead of testing another instance.

Tolerances as in test_gpu_kernels.py / test_gpu_batched.py: the expected values are float64 sums
over the same fp16 activations and the oracle's dequantized int4 weights, so fp32 outputs differ by
summation order only (|err| <= 2e-5 * sum_k |x_k w_k| + 1e-6; 5e-5 for the residual add, whose
difference from the residual loses bits), fp16 outputs by their rounding (2e-3; SiLU * up 3e-3),
RoPE'd q and logits 1e-4, appended K / V 2e-3.
"""
from __future__ import annotations

import ctypes as C
from collections import Counter

import numpy as np
import pytest

from test_gpu_kernels import assert_close_dot, deq, dev

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64

SENT = np.float32(-12345.678)        # fills every output before the call
SENT16 = np.uint16(0xA5A5)
THETA = 10000.0


# ------------------------------------------------------------------ plan and inputs
def mb_plan(T, M, N, K):
    g, n = C.c_int(), C.c_int()
    rc = T.lib().ti_gemm_mb_plan(4, M, N, K, C.byref(g), C.byref(n))
    return (g.value, n.value) if rc == 0 else None


def tile_ranges(N, grid):
    """Workgroup b's tiles [t0, t1) (ti_hip.h, ti_gemm_mb_plan)."""
    NT = N // 16
    return [(b * NT // grid, (b + 1) * NT // grid) for b in range(grid)]


def expect_plan(T, M, N, K, grid, ntl, split):
    """The call takes gemv_mbr_kernel with `grid` workgroups of at most `ntl` tiles; split maps
    tiles per workgroup to the number of such workgroups."""
    assert T.gemm_kernel_name(4, T.X_F16, M, N, K) == "gemv_mbr_kernel"
    assert mb_plan(T, M, N, K) == (grid, ntl)
    assert Counter(t1 - t0 for t0, t1 in tile_ranges(N, grid)) == split


def weights(rng, K, N, std=0.03):
    """Columns of unlike magnitude (unlike group scales: a scale or a column taken from a neighbour
    shows far above the bound)."""
    return (rng.standard_normal((K, N)) * std * (0.5 + 1.5 * rng.random_sample(N))).astype(f32)


def store_case(T, oracle, M, N, K):
    """(x fp16 [M][K], packed tiles, scales, dequantized weights [K][N], float64 expectation) of a
    plain store case; the same arrays for the GPU cases and the CPU sensitivity test."""
    rng = np.random.RandomState(M * 7 + K + N)
    w = weights(rng, K, N)
    x = rng.standard_normal((M, K)).astype(f16)
    tiles, scales = T.wpack_host(w, 4)
    wf = deq(oracle, w, 4)
    return x, tiles, scales, wf, x.astype(f64) @ wf.astype(f64)


def launch(ti, td, sd, xd, ldx, M, N, K, ep):
    ti.check(ti.lib().ti_gemm_wq_a16(td.ptr, sd.ptr, 4, xd.ptr, ti.X_F16, ldx, None, 1e-5, M, N, K, C.byref(ep), None))
    ti.sync()


def padded_rows(x, ldx):
    """x in rows of ldx elements; the pad holds values that would wreck any sum that read them."""
    out = np.full((x.shape[0], ldx), 3e4, x.dtype)
    out[:, :x.shape[1]] = x
    return out


def sentinel_f32(rows, ld):
    return np.full((rows, ld), SENT, f32)


def assert_untouched(buf, M, N, sent, what="output"):
    """Rows >= M and columns >= N of a [rows][ld] output keep the fill."""
    assert np.all(buf[M:] == sent), f"{what}: rows >= M written"
    assert np.all(buf[:M, N:] == sent), f"{what}: columns >= N written"


def check_store(ti, oracle, M, N, K, ldx=None, ldo=None):
    ldx, ldo = ldx or K, ldo or N
    x, tiles, scales, wf, ref = store_case(ti, oracle, M, N, K)
    yd = dev(ti, sentinel_f32(M + 3, ldo))
    ep = ti.Epilogue()
    ep.kind, ep.ldo, ep.out = ti.EPI_STORE_F32, ldo, yd.ptr
    launch(ti, dev(ti, tiles), dev(ti, scales), dev(ti, padded_rows(x, ldx)), ldx, M, N, K, ep)
    y = yd.download(f32, (M + 3, ldo))
    assert_untouched(y, M, N, SENT)
    assert_close_dot(y[:M, :N], ref, x.astype(f32), wf)


# ------------------------------------------------------------------ tile counts, K edges (fp32 store)
def n_of(j):
    """256 (j - 1) + 37 tiles: on 256 CUs 219 workgroups of j - 1 tiles and 37 of j."""
    return 16 * (256 * (j - 1) + 37)


@pytest.mark.parametrize("M,j", [(13, j) for j in range(1, 9)] + [(3, 8), (16, 8)])
def test_tiles_per_workgroup(ti, oracle, M, j):
    """NTL = j = 1..8 at K = 384 (three of the eight waves hold a k-tile)."""
    N, K = n_of(j), 384
    if j == 1:
        expect_plan(ti, M, N, K, 37, 1, {1: 37})
    else:
        expect_plan(ti, M, N, K, 256, j, {j - 1: 219, j: 37})
    check_store(ti, oracle, M, N, K)


def test_grid_past_the_cu_count(ti, oracle):
    """2100 tiles are more than 8 per workgroup on 256 CUs: the grid grows to 263 (4 of 7, 259 of 8)."""
    M, N, K = 13, 33600, 128
    expect_plan(ti, M, N, K, 263, 8, {7: 4, 8: 259})
    check_store(ti, oracle, M, N, K)


# K = 128: one k-tile, seven waves idle; 1152: a second chunk with one live wave; 2304: three
# chunks, the odd tail of the two-at-a-time loop; 4096: the served hidden size
@pytest.mark.parametrize("K", [128, 384, 1152, 2304, 4096])
def test_k_edges_ragged_tiles(ti, oracle, K):
    M, N = 13, 4800
    expect_plan(ti, M, N, K, 256, 2, {1: 212, 2: 44})
    check_store(ti, oracle, M, N, K)


@pytest.mark.parametrize("K,N,grid", [(32896, 48, 3), (65408, 32, 2)])
def test_k_edges_long_rows(ti, oracle, K, N, grid):
    """K / 128 = 257: 514 scale pieces, the second piece per thread is used; K / 128 = 511: the
    longest row the ABI takes.  One tile per workgroup (the scales of more would not fit)."""
    M = 13
    expect_plan(ti, M, N, K, grid, 1, {1: grid})
    check_store(ti, oracle, M, N, K)


def test_row_stride(ti, oracle):
    M, N, K = 13, 4800, 384
    expect_plan(ti, M, N, K, 256, 2, {1: 212, 2: 44})
    check_store(ti, oracle, M, N, K, ldx=K + 8)


def test_untouched_memory(ti, oracle):
    """ldo > N and rows past M: nothing but the M x N block is written (at NTL 6, 5 rows)."""
    M, N, K = 5, n_of(6), 384
    expect_plan(ti, M, N, K, 256, 6, {5: 219, 6: 37})
    check_store(ti, oracle, M, N, K, ldo=N + 24)


# ------------------------------------------------------------------ epilogues (M = 13, ragged NTL 3)
EM, EK, EN = 13, 384, n_of(3)


def expect_epilogue_plan(ti, N=EN):
    expect_plan(ti, EM, N, EK, 256, 3, {2: 219, 3: 37})


def test_store_f16(ti, oracle):
    expect_epilogue_plan(ti)
    x, tiles, scales, wf, ref = store_case(ti, oracle, EM, EN, EK)
    ldo = EN + 8
    yd = dev(ti, np.full((EM + 3, ldo), SENT16, np.uint16))
    ep = ti.Epilogue()
    ep.kind, ep.ldo, ep.out = ti.EPI_STORE_F16, ldo, yd.ptr
    launch(ti, dev(ti, tiles), dev(ti, scales), dev(ti, x), EK, EM, EN, EK, ep)
    y = yd.download(np.uint16, (EM + 3, ldo))
    assert_untouched(y, EM, EN, SENT16)
    np.testing.assert_allclose(np.ascontiguousarray(y[:EM, :EN]).view(f16).astype(f64), ref, rtol=2e-3, atol=2e-3)


def test_resid_f32_in_place(ti, oracle):
    expect_epilogue_plan(ti)
    x, tiles, scales, wf, ref = store_case(ti, oracle, EM, EN, EK)
    ldo = EN + 8
    r = np.random.RandomState(3).standard_normal((EM + 3, ldo)).astype(f32)
    rd = dev(ti, r)
    ep = ti.Epilogue()
    ep.kind, ep.ldo, ep.out = ti.EPI_RESID_F32, ldo, rd.ptr
    launch(ti, dev(ti, tiles), dev(ti, scales), dev(ti, x), EK, EM, EN, EK, ep)
    y = rd.download(f32, (EM + 3, ldo))
    assert np.array_equal(y[EM:].view(np.uint32), r[EM:].view(np.uint32)), "rows >= M written"
    assert np.array_equal(y[:EM, EN:].view(np.uint32), r[:EM, EN:].view(np.uint32)), "columns >= N written"
    assert_close_dot(y[:EM, :EN] - r[:EM, :EN], ref, x.astype(f32), wf, rel=5e-5)


def test_silu_mul_f16(ti, oracle):
    """gate / up interleaved by 8 per tile: N = 2 I outputs of the GEMM, I of the epilogue."""
    expect_epilogue_plan(ti)
    I = EN // 2
    rng = np.random.RandomState(31)
    g, u = weights(rng, EK, I, 0.1), weights(rng, EK, I, 0.1)
    x = rng.standard_normal((EM, EK)).astype(f16)
    tiles, scales = ti.wpack_host(g, 4, n_total=2 * I, row_map=ti.ROWS_INTERLEAVE8, row_offset=0)
    ti.wpack_host(u, 4, n_total=2 * I, row_map=ti.ROWS_INTERLEAVE8, row_offset=8, tiles=tiles, scales=scales)
    ldo = I + 8
    yd = dev(ti, np.full((EM + 3, ldo), SENT16, np.uint16))
    ep = ti.Epilogue()
    ep.kind, ep.ldo, ep.out = ti.EPI_SILU_MUL_F16, ldo, yd.ptr
    launch(ti, dev(ti, tiles), dev(ti, scales), dev(ti, x), EK, EM, 2 * I, EK, ep)
    y = yd.download(np.uint16, (EM + 3, ldo))
    assert_untouched(y, EM, I, SENT16)
    xa = x.astype(f64)
    gg, uu = xa @ deq(oracle, g, 4).astype(f64), xa @ deq(oracle, u, 4).astype(f64)
    np.testing.assert_allclose(np.ascontiguousarray(y[:EM, :I]).view(f16).astype(f64), uu * (gg / (1 + np.exp(-gg))),
                               rtol=3e-3, atol=2e-3)


def rope64(v, cs):
    """Pairs (2 i, 2 i + 1) of the last axis rotated by cs[i] = (cos, sin), in float64."""
    c, s = cs[:, 0].astype(f64), cs[:, 1].astype(f64)
    out = np.empty_like(v, dtype=f64)
    out[..., 0::2] = v[..., 0::2] * c - v[..., 1::2] * s
    out[..., 1::2] = v[..., 1::2] * c + v[..., 0::2] * s
    return out


# 32 q / 8 kv heads x 128: 384 tiles, 128 workgroups of 1 and 128 of 2; 96 q / 24 kv heads x 64: 576
# tiles, 192 workgroups of 2 and 64 of 3
@pytest.mark.parametrize("shared", [False, True], ids=["per-stream", "stride0"])
@pytest.mark.parametrize("hd,nh,nkv,ntl,split", [(128, 32, 8, 2, {1: 128, 2: 128}), (64, 96, 24, 3, {2: 192, 3: 64})],
                         ids=["hd128", "hd64"])
def test_qkv_rope_kv_append(ti, oracle, hd, nh, nkv, ntl, split, shared):
    M, H, max_seq = EM, EK, 24
    qd, kvd = nh * hd, nkv * hd
    N = qd + 2 * kvd
    expect_plan(ti, M, N, H, 256, ntl, split)
    rng = np.random.RandomState(41 + hd + nh)
    ws = [weights(rng, H, n, 0.05) for n in (qd, kvd, kvd)]
    tiles = scales = None
    for w, off in zip(ws, (0, qd, qd + kvd)):
        tiles, scales = ti.wpack_host(w, 4, n_total=N, row_offset=off, tiles=tiles, scales=scales)
    x = rng.standard_normal((M, H)).astype(f16)
    pos = (rng.permutation(max_seq)[:M] if shared else rng.randint(0, max_seq, size=M)).astype(np.int32)
    cs = ti.rope_table(np.arange(max_seq, dtype=f32), hd, THETA)
    S = 1 if shared else M
    slot = nkv * max_seq * hd
    ldo = qd + 8
    qbuf = dev(ti, sentinel_f32(M + 3, ldo))
    kc, vc = (dev(ti, np.full(S * slot, SENT16, np.uint16)) for _ in range(2))
    posd, csd = dev(ti, pos), dev(ti, cs)
    ep = ti.Epilogue()
    ep.kind, ep.ldo, ep.out = ti.EPI_QKV_ROPE_KV, ldo, qbuf.ptr
    ep.q_dim, ep.kv_dim, ep.head_dim, ep.max_seq = qd, kvd, hd, max_seq
    ep.pos, ep.rope_cs, ep.k_cache, ep.v_cache = posd.ptr, csd.ptr, kc.ptr, vc.ptr
    ep.kv_stream_stride = 0 if shared else slot
    launch(ti, dev(ti, tiles), dev(ti, scales), dev(ti, x), H, M, N, H, ep)
    q, k, v = (x.astype(f64) @ deq(oracle, w, 4).astype(f64) for w in ws)
    qgot = qbuf.download(f32, (M + 3, ldo))
    assert_untouched(qgot, M, qd, SENT, "q")
    kraw = kc.download(np.uint16, (S, nkv, max_seq, hd))
    vraw = vc.download(np.uint16, (S, nkv, max_seq, hd))
    written = np.zeros((S, max_seq), bool)
    for m in range(M):
        s = 0 if shared else m
        written[s, pos[m]] = True
        qr = rope64(q[m].reshape(nh, hd), cs[pos[m]])
        kr = rope64(k[m].reshape(nkv, hd), cs[pos[m]])
        np.testing.assert_allclose(qgot[m, :qd].astype(f64), qr.reshape(-1), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(kraw[s, :, pos[m]].view(f16).astype(f64), kr, rtol=2e-3, atol=2e-3)
        np.testing.assert_allclose(vraw[s, :, pos[m]].view(f16).astype(f64), v[m].reshape(nkv, hd), rtol=2e-3, atol=2e-3)
    # the pair order and the table are the reference's (the oracle's RoPE of row 0, fp32)
    p0 = np.array([pos[0]], f32)
    np.testing.assert_allclose(oracle.apply_rope(q[0].astype(f32).reshape(1, nh, 1, hd), p0, THETA).reshape(-1),
                               rope64(q[0].reshape(nh, hd), cs[pos[0]]).reshape(-1), rtol=1e-5, atol=1e-5)
    for name, raw in (("K", kraw), ("V", vraw)):
        other = raw.transpose(0, 2, 1, 3)[~written]
        assert np.all(other == SENT16), f"{name} cache: slots other than pos[m] written"


def run_logits(ti, w, x, M, V, K, advance, ctr0):
    tiles, scales = ti.wpack_host(w, 4)
    ldo = V + 8
    ld = dev(ti, sentinel_f32(M + 3, ldo))
    am = ti.DeviceBuffer((M + 3) * ti.ARGMAX_SLOTS * 8)
    am.zero()
    ctr = dev(ti, np.array([ctr0], np.int32))
    ep = ti.Epilogue()
    ep.kind, ep.ldo, ep.out, ep.argmax, ep.step_ctr, ep.advance = ti.EPI_LOGITS_ARGMAX, ldo, ld.ptr, am.ptr, ctr.ptr, advance
    launch(ti, dev(ti, tiles), dev(ti, scales), dev(ti, x), K, M, V, K, ep)
    lg = ld.download(f32, (M + 3, ldo))
    assert_untouched(lg, M, V, SENT, "logits")
    keys = am.download(np.uint64, (M + 3, ti.ARGMAX_SLOTS))
    assert not keys[M:].any(), "argmax rows >= M written"
    assert ctr.download(np.int32, (1,))[0] == ctr0 + advance, "step_ctr not advanced exactly once"
    idx = (0xFFFFFFFF - (keys[:M].max(axis=1) & 0xFFFFFFFF)).astype(np.int64)
    return np.ascontiguousarray(lg[:M, :V]), idx


def test_logits_argmax(ti, oracle):
    expect_epilogue_plan(ti)
    rng = np.random.RandomState(51)
    w = weights(rng, EK, EN, 0.05)
    x = rng.standard_normal((EM, EK)).astype(f16)
    lg, idx = run_logits(ti, w, x, EM, EN, EK, advance=2, ctr0=7)
    np.testing.assert_array_equal(idx, np.argmax(lg, axis=1))
    np.testing.assert_allclose(lg, x.astype(f64) @ deq(oracle, w, 4).astype(f64), rtol=1e-4, atol=1e-4)


def test_logits_argmax_tie_across_workgroups(ti, oracle):
    """Two identical weight columns, each row's maximum, in the third (last) tiles of workgroups 6 and
    166 (one argmax slot, 6 = 166 mod 32: the atomicMax decides) -- bit-equal logits, the lower index wins."""
    expect_epilogue_plan(ti)
    ranges = tile_ranges(EN, 256)
    assert ranges[6][1] - ranges[6][0] == 3 and ranges[166][1] - ranges[166][0] == 3
    n1, n2 = 16 * (ranges[6][1] - 1) + 9, 16 * (ranges[166][1] - 1) + 2
    assert n1 < n2
    rng = np.random.RandomState(53)
    w = weights(rng, EK, EN, 0.05)
    x = rng.standard_normal((EM, EK)).astype(f16)
    x[:, :128] = np.abs(x[:, :128])          # every row's sum over the first k-group is large and positive
    col = np.zeros(EK, f32)
    col[:128] = 1.0
    w[:, n1] = w[:, n2] = col
    lg, idx = run_logits(ti, w, x, EM, EN, EK, advance=1, ctr0=0)
    ref = x.astype(f64) @ deq(oracle, w, 4).astype(f64)
    np.testing.assert_allclose(lg, ref, rtol=1e-4, atol=1e-4)
    assert np.all(np.argmax(ref, axis=1) == n1) and np.all(ref[:, n1] == ref[:, n2])   # the case is a tie at the top
    assert np.array_equal(lg[:, n1].view(np.uint32), lg[:, n2].view(np.uint32)), "tied logits differ in bits"
    np.testing.assert_array_equal(idx, np.full(EM, n1))
