"""gemm_tile_kernel (int4 group-128 weights x fp16 rows: every projection from 65 rows, wide outputs from 17)
through ti_gemm_wq_a16 against float64: x_fp16 @ dequant(W), the weights the oracle dequantises.

Every case asserts the kernel's name and the plan it means to run (ti_gemm_tile_plan: row-waves, tiles per wave,
k-slices; the plan depends on the CU count, the shapes below are those of the MI355X's 256), hands the engine's
split-K workspace over with only its tickets zeroed (the partial blocks hold NaN), keeps a byte pattern behind every
output, launches twice from identical inputs and requires identical bits, finite outputs and re-armed tickets.

Rows: 65 (one row past a 64-row wave block), 100 (a partial second block), 129 (one row into a third).  Columns:
N = 1072 is 67 tiles, so the last column block of an 8-tile workgroup holds 3 real tiles; the 2 / 3 / 4-tile plans
run N = 10256 / 20496 / 30736 (641 / 1281 / 1921 tiles, ragged last blocks as well).  K = 640 never splits (5
groups); K = 2048 splits in 2 and K = 3200 in 3 slices of 8, 8 and 9 groups, neither a multiple of the merge's 4
slices per round trip (splitk_merge's CH at one tile per wave), so its clamp of the slice index runs.

Bars, the project's own (gemm_tile_ref.py): STORE_F32 assert_close_dot's default, RESID rel 5e-5, fp16 stores rtol =
atol = 2e-3, SiLU rtol 3e-3 / atol 2e-3, q and logits rtol = atol = 1e-4; e4m3 appends by kv8_ref.append_ok.

Plans this chip offers under the size cap (M <= 260, K <= 4096, M K N <= 2^31):
  * one row-wave (wmr 1) only.  tile_shape charges a workgroup 16 wmr + 8 tpw per round of workgroups, and a
    128-row workgroup never saves a round the 64-row one needs here; test_plan_coverage scans ti_gemm_tile_plan
    over the cap and finds no wmr 2 plan (the planner model gives the first one at 577 rows), so wmr 2 is not in
    the required set.
  * split K only at (wmr 1, tpw 1): a call splits when its one-slice grid is at most 64 workgroups, which is one
    round, where the cheapest shape is always 64 rows x 64 columns.  So "split" below means tpw 1.
  * out_packed is accepted on tile-kernel shapes (the dispatcher asks for a batched kernel, not the rows kernel):
    the per-element route writes TI_X_F16_PACKED order, pinned here through unpack_rows.
  * test_batched_fold_producer_consumer's row-major consumers (N = 25600 at 17 / 32 / 45 / 64 rows) do take
    gemm_tile_kernel, at one tile per wave and a 4e-3 bar; test_folded_input adds the tpw 4 path (its rms share
    is computed after the stream) and a tpw 1 case at RESID's bar.

Measured on an MI355X when this file was written (48 tests, 5.4 s; test_plan_coverage prints them again): worst
error / bar, unsplit | split -- STORE_F32 0.002 | 0.001, RESID 0.001 | < 0.001, STORE_F16 0.160 | 0.194, SiLU 0.142 |
0.156, QKV 0.192 | 0.216 (q 0.003 | 0.009, K 0.191 | 0.210, V 0.192 | 0.216: the fp16 rounding), logits 0.002 |
0.005, folded input 0.001; e4m3 must-equal share 0.975 .. 0.978.  No case is near its bar, so the NumPy emulation
of the slice-order sum (gemm_tile_ref.splitk_sum_f32) is only needed by test_gemm_tile_ref.py, which shows that
sum inside the one-slice bar.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import gemm_tile_ref as R
from test_gpu_kernels import deq, dev, gemm

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64
WS_BYTES = 16 << 20
TICKET_BYTES = 256 * 1024   # TI_SPLITK_TICKET_BYTES
GUARD, PAT = 256, 0xA5       # bytes behind every output, and their value
FILL = -7.25                 # what an output element holds before the launch
KINDS = ("store_f32", "resid", "store_f16", "silu", "qkv", "logits")

CASES = []    # (kind, M, N, K) of every parametrised case below: test_plan_coverage reads their plans
SEEN = set()  # (kind, wmr, tpw, split) of the cases that ran
RATIO = {}    # (kind, split) -> worst error / bar of the cases that ran


def case(kind, M, K, N, want, *more):
    CASES.append((kind, M, N, K))
    return pytest.param(M, K, N, want, *more, id="-".join(str(v) for v in (M, K, N) + more))


@pytest.fixture(scope="module")
def ws(ti):
    return ti.DeviceBuffer(WS_BYTES)


def arm(ti, ws):
    """The workspace as its owner must hand it over: tickets zero; the partial blocks hold NaN (0xFF bytes)."""
    L = ti.lib()
    ti.check(L.ti_memset(ws.ptr, 0, TICKET_BYTES, None))
    ti.check(L.ti_memset(ws.ptr + TICKET_BYTES, 0xFF, WS_BYTES - TICKET_BYTES, None))
    ti.sync()


def tile_plan(ti, M, N, K):
    v = [C.c_int() for _ in range(3)]
    rc = ti.lib().ti_gemm_tile_plan(4, M, N, K, WS_BYTES, *[C.byref(x) for x in v])
    return tuple(x.value for x in v) if rc == 0 else None


def plan_of(ti, kind, M, N, K, want):
    assert ti.gemm_kernel_name(4, ti.X_F16, M, N, K) == "gemm_tile_kernel"
    p = tile_plan(ti, M, N, K)
    print(f"{kind} M={M} N={N} K={K}: (wmr, tpw, n_ks) = {p}")
    assert p == want, f"the planner moved this case: {p}, meant {want}"
    SEEN.add((kind, p[0], p[1], p[2] > 1))
    return p


def note(kind, p, ratio):
    key = (kind, p[2] > 1)
    RATIO[key] = max(RATIO.get(key, 0.0), ratio)
    print(f"    worst error / bar {ratio:.3f}")


def guarded(ti, a):
    raw = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.full(GUARD, PAT, np.uint8)])
    return dev(ti, raw)


def body(buf, dtype, shape):
    raw = buf.download(np.uint8, (buf.nbytes,))
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    assert n + GUARD == raw.size
    assert np.all(raw[n:] == PAT), "bytes behind the buffer overwritten"
    buf.free()
    return raw[:n].view(dtype).reshape(shape)


def epilogue(ti, kind, ldo, out):
    ep = ti.Epilogue()
    ep.kind, ep.ldo, ep.out = kind, ldo, out.ptr
    return ep


def launch(ti, ws, td, sd, xd, M, N, K, ep):
    ep.splitk_ws, ep.splitk_bytes = ws.ptr, WS_BYTES
    gemm(ti, td, sd, 4, xd, ti.X_F16, K, M, N, K, ep)
    assert not ws.download(np.int32, (TICKET_BYTES // 4,)).any(), "split-K tickets not re-armed"


def twice(once):
    a, b = once(), once()
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes(), "a second launch gives other bits"
    return a


def same_bits(a, b):
    return a.tobytes() == np.ascontiguousarray(b).tobytes()


@functools.lru_cache(maxsize=8)
def weights(ti, oracle, K, N):
    """(tiles, scales on the device, dequantised W float64 [K][N]) of one seeded weight."""
    w = (np.random.RandomState(K + N).standard_normal((K, N)) * 0.03).astype(f32)
    tiles, scales = ti.wpack_host(w, 4)
    wf = deq(oracle, w, 4).astype(f64)
    wf.setflags(write=False)
    return dev(ti, tiles), dev(ti, scales), wf


@functools.lru_cache(maxsize=4)
def silu_weights(ti, oracle, K, I):
    rng = np.random.RandomState(K + I)
    g, u = ((rng.standard_normal((K, I)) * 0.05).astype(f32) for _ in range(2))
    tiles, scales = ti.wpack_host(g, 4, n_total=2 * I, row_map=ti.ROWS_INTERLEAVE8, row_offset=0)
    ti.wpack_host(u, 4, n_total=2 * I, row_map=ti.ROWS_INTERLEAVE8, row_offset=8, tiles=tiles, scales=scales)
    return dev(ti, tiles), dev(ti, scales), deq(oracle, g, 4).astype(f64), deq(oracle, u, 4).astype(f64)


# ------------------------------------------------------------------ STORE_F32, STORE_F16, RESID_F32
def run_store(ti, oracle, ws, kind, M, K, N, want, pad=0, packed=0):
    """pad: ldo = N + pad, the gap columns keep their pattern.  packed: TI_X_F16_PACKED order (STORE_F16)."""
    p = plan_of(ti, kind, M, N, K, want)
    td, sd, wf = weights(ti, oracle, K, N)
    x = R.rows(M, K, M + K)
    xd, ref = dev(ti, x), x.astype(f64) @ wf
    ldo, dt = N + pad, f16 if kind == "store_f16" else f32
    Mp = (M + 15) // 16 * 16 if packed else M
    init = np.full((Mp, ldo), FILL, dt)
    if kind == "resid":
        init[:, :N] = np.random.RandomState(N + M).standard_normal((M, N)).astype(f32)
    arm(ti, ws)

    def once():
        od = guarded(ti, init)                    # (RESID: a fresh residual copy for each launch)
        ep = epilogue(ti, {"store_f32": ti.EPI_STORE_F32, "store_f16": ti.EPI_STORE_F16, "resid": ti.EPI_RESID_F32}[kind],
                      ldo, od)
        ep.out_packed = packed
        launch(ti, ws, td, sd, xd, M, N, K, ep)
        return (body(od, dt, (Mp, ldo)),)

    (got,) = twice(once)
    if packed:
        flat = got.reshape(-1)
        mm, kk = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
        live = np.zeros(flat.size, bool)
        live[ti.packed_index(mm, kk, N)] = True
        assert same_bits(flat[~live], np.full(int((~live).sum()), FILL, dt)), "padding rows of the packed output written"
        got = ti.unpack_rows(flat, M, N)
    assert same_bits(got[:, N:], init[:, N:]), "gap columns of the padded ldo overwritten"
    got = got[:, :N]
    if kind == "store_f32":
        ratio = R.check_dot(got, ref, x.astype(f32), wf)
    elif kind == "resid":
        ratio = R.check_resid(got, init[:, :N], ref, x.astype(f32), wf)
    else:
        ratio = R.check_close(got, ref, **R.F16_BAR)
    note(kind, p, ratio)


@pytest.mark.parametrize("M,K,N,want", [
    case("store_f32", 65, 640, 1072, (1, 1, 1)), case("store_f32", 100, 640, 1072, (1, 1, 1)),
    case("store_f32", 129, 640, 1072, (1, 1, 1)),
    case("store_f32", 129, 384, 10256, (1, 2, 1)), case("store_f32", 129, 384, 20496, (1, 3, 1)),
    case("store_f32", 129, 384, 30736, (1, 4, 1)),
    case("store_f32", 65, 2048, 1072, (1, 1, 2)), case("store_f32", 100, 3200, 1072, (1, 1, 3)),
    case("store_f32", 129, 3200, 1072, (1, 1, 3))])
def test_store_f32(ti, oracle, ws, M, K, N, want):
    run_store(ti, oracle, ws, "store_f32", M, K, N, want)


@pytest.mark.parametrize("M,K,N,want", [case("store_f32", 100, 640, 1072, (1, 1, 1)),
                                        case("store_f32", 100, 2048, 1072, (1, 1, 2))])
def test_store_f32_padded_ldo(ti, oracle, ws, M, K, N, want):
    run_store(ti, oracle, ws, "store_f32", M, K, N, want, pad=16)


@pytest.mark.parametrize("M,K,N,want,pad", [
    case("resid", 65, 640, 1072, (1, 1, 1), 0), case("resid", 100, 640, 1072, (1, 1, 1), 16),
    case("resid", 129, 640, 1072, (1, 1, 1), 0), case("resid", 129, 384, 10256, (1, 2, 1), 0),
    case("resid", 65, 2048, 1072, (1, 1, 2), 0), case("resid", 100, 3200, 1072, (1, 1, 3), 16),
    case("resid", 129, 3200, 1072, (1, 1, 3), 0)])
def test_resid_in_place(ti, oracle, ws, M, K, N, want, pad):
    """The engine's O and down projections: with a split, only the last arriver reads the residual and adds the
    slice sum to it, once."""
    run_store(ti, oracle, ws, "resid", M, K, N, want, pad=pad)


@pytest.mark.parametrize("M,K,N,want,pad", [
    case("store_f16", 65, 640, 1072, (1, 1, 1), 0), case("store_f16", 100, 640, 1072, (1, 1, 1), 16),
    case("store_f16", 129, 640, 1072, (1, 1, 1), 0), case("store_f16", 100, 2048, 1072, (1, 1, 2), 16),
    case("store_f16", 129, 3200, 1072, (1, 1, 3), 0)])
def test_store_f16(ti, oracle, ws, M, K, N, want, pad):
    run_store(ti, oracle, ws, "store_f16", M, K, N, want, pad=pad)


def test_store_f16_packed(ti, oracle, ws):
    """out_packed on a tile-kernel shape: the per-element route writes TI_X_F16_PACKED order; the rows that pad
    the last 16-row block keep their pattern."""
    run_store(ti, oracle, ws, "store_f16", 100, 640, 1152, (1, 1, 1), packed=1)


# ------------------------------------------------------------------ SILU_MUL_F16
def run_silu(ti, oracle, ws, M, K, I, want, packed=0):
    p = plan_of(ti, "silu", M, 2 * I, K, want)
    td, sd, gf, uf = silu_weights(ti, oracle, K, I)
    x = R.rows(M, K, M + K + 1)
    xd = dev(ti, x)
    ref = R.silu_mul64(x.astype(f64) @ gf, x.astype(f64) @ uf)
    Mp = (M + 15) // 16 * 16 if packed else M
    init = np.full((Mp, I), FILL, f16)
    arm(ti, ws)

    def once():
        od = guarded(ti, init)
        ep = epilogue(ti, ti.EPI_SILU_MUL_F16, I, od)
        ep.out_packed = packed
        launch(ti, ws, td, sd, xd, M, 2 * I, K, ep)
        return (body(od, f16, (Mp, I)),)

    (got,) = twice(once)
    if packed:
        flat = got.reshape(-1)
        mm, kk = np.meshgrid(np.arange(M), np.arange(I), indexing="ij")
        live = np.zeros(flat.size, bool)
        live[ti.packed_index(mm, kk, I)] = True
        assert same_bits(flat[~live], np.full(int((~live).sum()), FILL, f16)), "padding rows of the packed output written"
        got = ti.unpack_rows(flat, M, I)
    note("silu", p, R.check_close(got, ref, **R.SILU_BAR))


@pytest.mark.parametrize("M,K,N,want", [
    case("silu", 65, 640, 1072, (1, 1, 1)), case("silu", 100, 640, 1072, (1, 1, 1)),
    case("silu", 129, 640, 1072, (1, 1, 1)), case("silu", 129, 384, 30736, (1, 4, 1)),
    case("silu", 65, 2048, 1072, (1, 1, 2)), case("silu", 129, 3200, 1072, (1, 1, 3))])
def test_silu_mul_interleaved(ti, oracle, ws, M, K, N, want):
    """Gate and up rows interleaved by 8 per weight tile; N / 2 outputs through the wave's LDS block."""
    run_silu(ti, oracle, ws, M, K, N // 2, want)


def test_silu_mul_packed(ti, oracle, ws):
    """out_packed: SiLU * up per element, in TI_X_F16_PACKED order (ragged rows: 77 of 80)."""
    run_silu(ti, oracle, ws, 77, 640, 640, (1, 1, 1), packed=1)


# ------------------------------------------------------------------ QKV_ROPE_KV
def qkv(hd, nh, nkv, M, K, form, want):
    CASES.append(("qkv", M, (nh + 2 * nkv) * hd, K))
    return pytest.param(hd, nh, nkv, M, K, form, want, id=f"hd{hd}-{nh}q{nkv}kv-{M}-{K}-{form}")


# head_dim 64 with 9 query heads on 3 KV heads: 60 tiles, the last 8-tile column block half empty
@pytest.mark.parametrize("hd,nh,nkv,M,K,form,want", [
    qkv(64, 9, 3, 65, 640, "batched", (1, 1, 1)), qkv(64, 9, 3, 100, 640, "prefill", (1, 1, 1)),
    qkv(64, 9, 3, 129, 640, "batched", (1, 1, 1)), qkv(128, 4, 2, 129, 640, "prefill", (1, 1, 1)),
    qkv(128, 4, 2, 65, 2048, "batched", (1, 1, 2)), qkv(64, 9, 3, 100, 3200, "prefill", (1, 1, 3)),
    qkv(64, 9, 3, 129, 3200, "batched", (1, 1, 3))])
def test_qkv_rope_kv(ti, oracle, ws, hd, nh, nkv, M, K, form, want):
    """Both engine forms (prefill: one stream, kv_stream_stride 0, distinct positions in no row order; batched: a
    stream per row), GQA.  The fp16 cache against float64 RoPE with the table the kernel reads; then the same call
    into an e4m3 cache, judged against the fp16 rows; q bit-identical between the two.  Every slot pos does not
    name stays zero."""
    qd, kvd = nh * hd, nkv * hd
    N = qd + 2 * kvd
    p = plan_of(ti, "qkv", M, N, K, want)
    wsrc, x, pos, max_seq, stride = R.qkv_inputs(hd, nh, nkv, M, K, form)
    tiles = scales = None
    for w, off in zip(wsrc, (0, qd, qd + kvd)):
        tiles, scales = ti.wpack_host(w, 4, n_total=N, row_offset=off, tiles=tiles, scales=scales)
    td, sd, xd, posd = dev(ti, tiles), dev(ti, scales), dev(ti, x), dev(ti, pos)
    cs = ti.rope_table(np.arange(max_seq, dtype=f32), hd, 10000.0)
    csd = dev(ti, cs)
    n_cache = M * stride if stride else nkv * max_seq * hd
    arm(ti, ws)
    res = {}
    for fp8 in (0, 1):
        dt = np.uint8 if fp8 else np.uint16

        def once():
            qb = guarded(ti, np.full((M, qd), FILL, f32))
            kc, vc = guarded(ti, np.zeros(n_cache, dt)), guarded(ti, np.zeros(n_cache, dt))
            ep = epilogue(ti, ti.EPI_QKV_ROPE_KV, qd, qb)
            ep.q_dim, ep.kv_dim, ep.head_dim, ep.max_seq, ep.kv_fp8 = qd, kvd, hd, max_seq, fp8
            ep.pos, ep.rope_cs, ep.k_cache, ep.v_cache, ep.kv_stream_stride = posd.ptr, csd.ptr, kc.ptr, vc.ptr, stride
            launch(ti, ws, td, sd, xd, M, N, K, ep)
            return body(qb, f32, (M, qd)), body(kc, dt, (n_cache,)), body(vc, dt, (n_cache,))

        res[fp8] = twice(once)
    q, k, v = (x.astype(f64) @ deq(oracle, w, 4).astype(f64) for w in wsrc)
    idx = R.kv_slots(pos, nkv, hd, max_seq, stride)
    kh, vh = res[0][1].view(f16), res[0][2].view(f16)
    ratios = (R.check_close(res[0][0], R.rope64(q, pos, cs, hd), what="q", **R.Q_BAR),
              R.check_kv_f16(kh, R.rope64(k, pos, cs, hd), idx, "K"), R.check_kv_f16(vh, v, idx, "V"))
    print(f"    q, K, V error / bar: {ratios[0]:.3f} {ratios[1]:.3f} {ratios[2]:.3f}")
    assert same_bits(res[1][0], res[0][0]), "q differs between the fp16 and the e4m3 call"
    must = [R.check_kv_e4m3(res[1][1], kh, idx, "K"), R.check_kv_e4m3(res[1][2], vh, idx, "V")]
    print(f"    e4m3 must-equal share K {must[0]:.3f} V {must[1]:.3f}")
    note("qkv", p, max(ratios))


# ------------------------------------------------------------------ LOGITS_ARGMAX
def run_logits(ti, oracle, ws, M, K, V, want, ties=()):
    """ties: (row, low column, high column): both columns get the same weights, aligned with the row."""
    p = plan_of(ti, "logits", M, V, K, want)
    x = R.rows(M, K, M + K + 2)
    if ties:
        w = (np.random.RandomState(V).standard_normal((K, V)) * 0.03).astype(f32)
        for row, lo, hi in ties:
            w[:, lo] = w[:, hi] = 0.5 * x[row].astype(f32) / np.linalg.norm(x[row].astype(f32))
        tiles, scales = ti.wpack_host(w, 4)
        td, sd, wf = dev(ti, tiles), dev(ti, scales), deq(oracle, w, 4).astype(f64)
    else:
        td, sd, wf = weights(ti, oracle, K, V)
    xd = dev(ti, x)
    arm(ti, ws)

    def once():
        ld, am = guarded(ti, np.full((M, V), FILL, f32)), guarded(ti, np.zeros((M, ti.ARGMAX_SLOTS), np.uint64))
        ctr = guarded(ti, np.array([7], np.int32))
        ep = epilogue(ti, ti.EPI_LOGITS_ARGMAX, V, ld)
        ep.argmax, ep.step_ctr, ep.advance = am.ptr, ctr.ptr, 3
        launch(ti, ws, td, sd, xd, M, V, K, ep)
        # (a row's key is the max over its slots; which slot a workgroup uses is its blockIdx's, and with a
        # split K the workgroup that arrives last runs the epilogue: the slots differ from launch to launch)
        return (body(ld, f32, (M, V)), body(am, np.uint64, (M, ti.ARGMAX_SLOTS)).max(axis=1, keepdims=True),
                body(ctr, np.int32, (1,)))

    logits, keys, ctr = twice(once)
    assert ctr[0] == 10, "step_ctr must advance by `advance` once per call"
    idx = R.check_argmax(keys, logits)
    for row, lo, hi in ties:
        assert logits[row, lo] == logits[row, hi] == logits[row].max() and idx[row] == lo
    note("logits", p, R.check_close(logits, x.astype(f64) @ wf, what="logits", **R.Q_BAR))


@pytest.mark.parametrize("M,K,N,want", [
    case("logits", 65, 640, 1072, (1, 1, 1)), case("logits", 100, 640, 1072, (1, 1, 1)),
    case("logits", 129, 640, 1072, (1, 1, 1)), case("logits", 65, 2048, 1072, (1, 1, 2)),
    case("logits", 100, 3200, 1072, (1, 1, 3))])
def test_logits_argmax(ti, oracle, ws, M, K, N, want):
    run_logits(ti, oracle, ws, M, K, N, want)


CASES.append(("logits", 129, 10256, 256))


def test_logits_argmax_ties(ti, oracle, ws):
    """Row 5: columns 37 and 9000, in different column blocks (workgroups); row 70: columns 3 and 25, the two
    tiles of one wave (2 tiles per wave).  The lowest index wins both."""
    run_logits(ti, oracle, ws, 129, 256, 10256, (1, 2, 1), ties=((5, 37, 9000), (70, 3, 25)))


# ------------------------------------------------------------------ folded input (17..64 rows, wide outputs)
@pytest.mark.parametrize("M,K,N,want", [(40, 640, 25600, (1, 1, 1)), (40, 256, 98320, (1, 4, 1))],
                         ids=["tpw1", "tpw4"])
def test_folded_input(ti, oracle, ws, M, K, N, want):
    """ss_in on the tile kernel: x = fp16(h * nw) and 70 partial sums of h^2 per row (TI_FOLD_SS_ROWS rows each;
    more than one round of 64 partials per row, the rows past M hold NaN), y = (W . x) / sqrt(sum ss / K + eps).
    With 4 tiles per wave the share of the sums is read after the stream, otherwise before it."""
    p = plan_of(ti, "fold", M, N, K, want)
    td, sd, wf = weights(ti, oracle, K, N)
    rng = np.random.RandomState(M + N)
    h = (rng.standard_normal((M, K)) * 2).astype(f32)
    x = (h * (1 + 0.1 * rng.standard_normal(K)).astype(f32)).astype(f16)
    n_ss, eps = 70, 1e-5
    ss = np.full((n_ss, 64), np.nan, f32)
    for b, cols in enumerate(np.array_split(np.arange(K), n_ss)):
        ss[b, :M] = (h[:, cols].astype(f64) ** 2).sum(axis=1)
    rms = np.sqrt(ss[:, :M].astype(f64).sum(axis=0) / K + eps)
    xd, ssd = dev(ti, x), dev(ti, ss)
    arm(ti, ws)

    def once():
        od = guarded(ti, np.full((M, N), FILL, f32))
        ep = epilogue(ti, ti.EPI_STORE_F32, N, od)
        ep.ss_in, ep.n_ss = ssd.ptr, n_ss
        launch(ti, ws, td, sd, xd, M, N, K, ep)
        return (body(od, f32, (M, N)),)

    (got,) = twice(once)
    xs = x.astype(f64) / rms[:, None]
    ratio = R.check_dot(got, xs @ wf, xs, wf, rel=R.REL_RESID)
    print(f"    worst error / bar {ratio:.3f}")


def test_fold_producer_consumer_shapes_take_the_tile_kernel(ti):
    """test_gpu_batched.py's test_batched_fold_producer_consumer: its row-major consumers run this kernel."""
    for M in (17, 32, 45, 64):
        name = ti.gemm_kernel_name(4, ti.X_F16, M, 25600, 1024)
        print(f"M={M} N=25600 K=1024: {name} {tile_plan(ti, M, 25600, 1024)}")
        assert name == "gemm_tile_kernel" and tile_plan(ti, M, 25600, 1024) == (1, 1, 1)


# ------------------------------------------------------------------ plan coverage
def test_plan_coverage(ti):
    """The cases above, by their plans: 1 to 4 tiles per wave for STORE_F32, split and unsplit K for every
    epilogue kind.  wmr 2 is not required: the scan below finds none under the size cap (module docstring)."""
    have = {(kind,) + tile_plan(ti, M, N, K) for kind, M, N, K in CASES}
    for row in sorted(have):
        print(row)
    ran = {s for s in SEEN if s[0] in KINDS}                   # (every case that ran is one counted here)
    assert ran <= {(kind, wmr, tpw, ks > 1) for kind, wmr, tpw, ks in have}, ran
    assert {tpw for kind, wmr, tpw, ks in have if kind == "store_f32" and ks == 1} == {1, 2, 3, 4}
    for kind in KINDS:
        assert {ks > 1 for k, wmr, tpw, ks in have if k == kind} == {False, True}, kind
    assert {3} <= {ks for kind, wmr, tpw, ks in have}          # ragged slices: 25 groups in 3
    wmrs = set()
    for M in (65, 100, 129, 192, 256, 260):
        for K in (128, 640, 4096):
            for N in range(16, (1 << 31) // (M * K) + 1, 16):
                wmrs.add(tile_plan(ti, M, N, K)[0])
    assert wmrs == {1}, "the planner now offers two row-waves under the size cap: add cases for them"
    for (kind, split), ratio in sorted(RATIO.items()):
        print(f"{kind:10s} {'split' if split else 'unsplit':8s} worst error / bar {ratio:.3f}")
