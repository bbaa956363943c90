"""CPU self-tests of tests/gemm_tile_ref.py: the compare rules of test_gpu_gemm_tile.py accept the float64 result
rounded the way the kernel stores it, and reject each way gemm_tile_kernel could be subtly wrong (one mutant of
the float64 result per rule).  Also: the e4m3 cases' reference rows alone meet append_ok's must-equal share, the
slice-order fp32 sum of a split K stays inside the one-slice bar, and ti_gemm_tile_plan answers for exactly the
calls ti_gemm_wq_a16 gives the tile kernel."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import gemm_tile_ref as R
import kv8_ref as Q
from test_gpu_kernels import deq

f16, f32, f64 = np.float16, np.float32, np.float64
M, K, N = 129, 640, 1072          # test_gpu_gemm_tile.py's edge shape: three 64-row blocks, 67 tiles
FILL = -7.25


@pytest.fixture(scope="module")
def prod(oracle):
    """x, dequantised W, their float64 product, a residual."""
    rng = np.random.RandomState(3)
    wf = deq(oracle, (rng.standard_normal((K, N)) * 0.03).astype(f32), 4).astype(f64)
    x = R.rows(M, K, 4)
    return x, wf, x.astype(f64) @ wf, rng.standard_normal((M, N)).astype(f32)


def slice_dropped(ref, x, wf):
    """k-slice 1 of 2 (groups 2..4) missing from the 64 x 16 block of rows 64..127, tile 5."""
    out = ref.copy()
    out[64:128, 80:96] -= x[64:128, 256:].astype(f64) @ wf[256:, 80:96]
    return out


def last_row_old(ref, x, wf):
    out = ref.copy()
    out[M - 1] = FILL
    return out


def last_tile_unwritten(ref, x, wf):
    out = ref.copy()
    out[:, N - 16:] = FILL
    return out


MUTANTS = [slice_dropped, last_row_old, last_tile_unwritten]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_store_and_resid_rules_reject(prod, mutant):
    x, wf, ref, r = prod
    xa = x.astype(f32)
    assert R.check_dot(ref.astype(f32), ref, xa, wf) < 1
    assert R.check_resid(r + ref.astype(f32), r, ref, xa, wf) < 1
    wrong = mutant(ref, x, wf)
    with pytest.raises(AssertionError):
        R.check_dot(wrong.astype(f32), ref, xa, wf)
    with pytest.raises(AssertionError):                       # (an unwritten residual element keeps r: + 0)
        R.check_resid(r + np.where(wrong == FILL, 0, wrong).astype(f32), r, ref, xa, wf)


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("bar", [R.F16_BAR, R.Q_BAR], ids=["fp16", "logits"])
def test_store_f16_and_logits_rules_reject(prod, mutant, bar):
    x, wf, ref, _ = prod
    dt = f16 if bar is R.F16_BAR else f32
    assert R.check_close(ref.astype(dt), ref, **bar) < 1
    with pytest.raises(AssertionError):
        R.check_close(mutant(ref, x, wf).astype(dt), ref, **bar)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_silu_rule_rejects(prod, mutant):
    """Gate = the first 536 columns, up = the rest; the mutant hits the gate (block, row) or the up half (tile)."""
    x, wf, ref, _ = prod
    want = R.silu_mul64(ref[:, :N // 2], ref[:, N // 2:])
    assert R.check_close(want.astype(f16), want, **R.SILU_BAR) < 1
    wrong = mutant(ref, x, wf)
    with pytest.raises(AssertionError):
        R.check_close(R.silu_mul64(wrong[:, :N // 2], wrong[:, N // 2:]).astype(f16), want, **R.SILU_BAR)


def test_resid_rule_rejects_a_second_add(prod):
    x, wf, ref, r = prod
    with pytest.raises(AssertionError):
        R.check_resid(r + r + ref.astype(f32), r, ref, x.astype(f32), wf)
    with pytest.raises(AssertionError):                       # ... and the product added twice
        R.check_resid(r + 2 * ref.astype(f32), r, ref, x.astype(f32), wf)
    with pytest.raises(AssertionError, match="non-finite"):   # a partial block no slice wrote (NaN workspace)
        R.check_resid(r + np.where(np.arange(N) == 7, np.nan, ref).astype(f32), r, ref, x.astype(f32), wf)


def test_splitk_sum_is_in_the_one_slice_error_class(prod):
    """n_ks fp32 partials added in slice order: at most n_ks - 1 more roundings of the running sum, far inside
    assert_close_dot's bound (which allows 2e-5 of sum |x w|: hundreds of roundings)."""
    x, wf, ref, _ = prod
    for n_ks in (2, 3, 5):
        assert R.check_dot(R.splitk_sum_f32(x, wf, n_ks), ref, x.astype(f32), wf) < 0.05


QKV_CASES = [(64, 9, 3, 100, 640, "prefill"), (128, 4, 2, 65, 640, "batched")]


def qkv_ref(ti_host, oracle, hd, nh, nkv, Mq, Kq, form):
    ws, x, pos, max_seq, stride = R.qkv_inputs(hd, nh, nkv, Mq, Kq, form)
    cs = ti_host.rope_table(np.arange(max_seq, dtype=f32), hd, 10000.0)
    q, k, v = (x.astype(f64) @ deq(oracle, w, 4).astype(f64) for w in ws)
    n_cache = Mq * stride if stride else nkv * max_seq * hd
    return q, k, v, pos, cs, max_seq, stride, n_cache


def cache_of(rows, idx, n_cache):
    c = np.zeros(n_cache, f16)
    c[idx] = rows.reshape(idx.shape).astype(f16)
    return c


@pytest.mark.parametrize("hd,nh,nkv,Mq,Kq,form", QKV_CASES)
def test_qkv_rules_reject(ti_host, oracle, hd, nh, nkv, Mq, Kq, form):
    q, k, v, pos, cs, max_seq, stride, n_cache = qkv_ref(ti_host, oracle, hd, nh, nkv, Mq, Kq, form)
    idx = R.kv_slots(pos, nkv, hd, max_seq, stride)
    assert np.unique(idx).size == idx.size                   # no two rows share a slot
    qr, kr = R.rope64(q, pos, cs, hd), R.rope64(k, pos, cs, hd)
    assert R.check_close(qr.astype(f32), qr, what="q", **R.Q_BAR) < 1
    assert R.check_kv_f16(cache_of(kr, idx, n_cache), kr, idx, "K") < 1
    assert R.check_kv_f16(cache_of(v, idx, n_cache), v, idx, "V") < 1
    # RoPE with the neighbouring row's position
    near = np.roll(pos, 1)
    assert np.all(near != pos) or form == "batched"
    with pytest.raises(AssertionError):
        R.check_close(R.rope64(q, near, cs, hd).astype(f32), qr, what="q", **R.Q_BAR)
    with pytest.raises(AssertionError):
        R.check_kv_f16(cache_of(R.rope64(k, near, cs, hd), idx, n_cache), kr, idx, "K")
    # one row's slot written at pos + 1 (a row whose next slot exists and is no other row's)
    row = next(i for i in range(Mq) if pos[i] + 1 < max_seq and (stride or pos[i] + 1 not in pos))
    moved = pos.copy()
    moved[row] += 1
    for rows, name in ((kr, "K"), (v, "V")):
        with pytest.raises(AssertionError, match="outside the slots"):
            R.check_kv_f16(cache_of(rows, R.kv_slots(moved, nkv, hd, max_seq, stride), n_cache), rows, idx, name)
        h = cache_of(rows, idx, n_cache)
        with pytest.raises(AssertionError, match="outside the slots"):
            R.check_kv_e4m3(Q.quantize(cache_of(rows, R.kv_slots(moved, nkv, hd, max_seq, stride), n_cache)), h, idx, name)


@pytest.mark.parametrize("hd,nh,nkv,Mq,Kq,form", [
    (64, 9, 3, 65, 640, "batched"), (64, 9, 3, 100, 640, "prefill"), (64, 9, 3, 129, 640, "batched"),
    (128, 4, 2, 129, 640, "prefill"), (128, 4, 2, 65, 2048, "batched"), (64, 9, 3, 100, 3200, "prefill"),
    (64, 9, 3, 129, 3200, "batched")])
def test_e4m3_reference_rows_meet_the_must_equal_share(ti_host, oracle, hd, nh, nkv, Mq, Kq, form):
    """Every QKV case of test_gpu_gemm_tile.py: the fp16 rounding of the float64 rows, quantised by the model,
    passes append_ok with must.mean() > 0.9 -- the cap is met by the reference alone; a byte one code off fails."""
    q, k, v, pos, cs, max_seq, stride, n_cache = qkv_ref(ti_host, oracle, hd, nh, nkv, Mq, Kq, form)
    idx = R.kv_slots(pos, nkv, hd, max_seq, stride)
    for rows, name in ((R.rope64(k, pos, cs, hd), "K"), (v, "V")):
        h = cache_of(rows, idx, n_cache)
        b = Q.quantize(h)
        assert R.check_kv_e4m3(b, h, idx, name) > 0.9
        b[idx[0, 0, 0]] += 2                                   # two codes up: no neighbour of its fp16 value
        with pytest.raises(AssertionError):
            R.check_kv_e4m3(b, h, idx, name)


def test_argmax_rule_rejects_the_higher_index():
    logits = np.random.RandomState(9).standard_normal((3, 64)).astype(f32)
    logits[1, 5] = logits[1, 40] = 9.0
    key = lambda row, i: (int(R.order_key(logits[row, i])) << 32) | (0xFFFFFFFF - i)
    keys = np.zeros((3, 32), np.uint64)
    for row in range(3):
        keys[row, row + 3] = key(row, int(np.argmax(logits[row])))
    keys[1, 9] = key(1, 40)                                   # the other slot holds the tie's higher index: below
    assert R.check_argmax(keys, logits).tolist() == [int(np.argmax(r)) for r in logits] and np.argmax(logits[1]) == 5
    wrong = keys.copy()
    wrong[1, 4] = 0                                           # only the higher index arrived
    with pytest.raises(AssertionError):
        R.check_argmax(wrong, logits)
    wrong = keys.copy()
    wrong[0, 3] = key(0, int(np.argmax(logits[0]))) ^ (1 << 32)   # the right index with another logit's bits
    with pytest.raises(AssertionError):
        R.check_argmax(wrong, logits)


def test_tile_plan_answers_for_the_tile_kernel_calls(ti_host):
    """ti_gemm_tile_plan succeeds exactly where ti_gemm_kernel_name says gemm_tile_kernel: from 65 rows, and for
    17..64 rows of a wide output (which it used to refuse)."""
    L = ti_host.lib()
    v = [C.c_int() for _ in range(3)]
    for Mr in (16, 17, 32, 33, 40, 64, 65, 129):
        for Nc in (512, 16368, 16384, 21248, 25600, 98320):
            name = ti_host.gemm_kernel_name(4, ti_host.X_F16, Mr, Nc, 1024)
            rc = L.ti_gemm_tile_plan(4, Mr, Nc, 1024, 0, *[C.byref(x) for x in v])
            assert (rc == 0) == (name == "gemm_tile_kernel"), (Mr, Nc, name, rc)
            if rc == 0:
                assert v[0].value in (1, 2) and 1 <= v[1].value <= 4 and v[2].value == 1
    assert L.ti_gemm_tile_plan(4 | ti_host.BITS_G32, 40, 25600, 1024, 0, *[C.byref(x) for x in v]) != 0
