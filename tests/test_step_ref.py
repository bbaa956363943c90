"""CPU self-tests of tests/step_ref.py: the models against hand-written cases, and the compare helpers shown to
reject each way ti_step_begin / ti_kv_copy_slots could be subtly wrong (one mutant of the model per rule).  The
GPU tests that use the same models and helpers: test_gpu_step_begin.py, test_gpu_kv_copy.py."""
from __future__ import annotations

import numpy as np
import pytest

import step_ref as R
from step_ref import (SLOTS, StepCase, StepModel, assert_step_equal, double_rounding_input, kv_copy_ref, logit_key,
                      sampled_key, step_begin_ref)

f16, f32 = np.float16, np.float32


def keys_row(*pairs):
    """One argmax row: (slot, key) pairs, every other slot 0."""
    row = np.zeros(SLOTS, np.uint64)
    for slot, key in pairs:
        row[slot] = key
    return row


def small_case(**kw):
    """M = 3, vocab 5, hidden 4: emb[t][i] = 10 t + i; rows fed from keys for tokens 4, 2, 0."""
    emb = (10 * np.arange(5)[:, None] + np.arange(4)[None, :]).astype(f16)
    argmax = np.stack([keys_row((3, logit_key(1.5, 4)), (9, logit_key(1.25, 1))),
                       keys_row((0, logit_key(-2.0, 2))),
                       keys_row((31, logit_key(0.5, 0)), (30, logit_key(0.25, 3)))])
    c = StepCase(argmax=argmax, base_pos=[7, 0, 100], s=2, emb=emb, in_tokens=np.array([[1, 1, 1], [3, 3, 3], [2, 2, 2]], np.int32),
                 n_in=np.array([0, 1, 2], np.int32), out_stride=3, out_tokens=np.full((3, 3), -9, np.int32))
    return c.at(**kw) if kw else c


# ------------------------------------------------------------------ keys
def test_key_encodings():
    assert logit_key(0.0, 0) == (0x80000000 << 32) | 0xFFFFFFFF
    assert logit_key(1.0, 3) == (0xBF800000 << 32) | 0xFFFFFFFC
    assert logit_key(-1.0, 3) == (0x407FFFFF << 32) | 0xFFFFFFFC
    assert sampled_key(5) == 0xFFFFFFFFFFFFFFFA
    vals = [-np.inf, -3.0, -1e-30, -0.0, 0.0, 1e-30, 2.0, np.inf]
    ks = [logit_key(v, 7) for v in vals]
    assert ks == sorted(ks) and len(set(ks)) == len(ks)          # order-preserving; -0.0 just below +0.0
    assert logit_key(1.0, 3) > logit_key(1.0, 7)                  # equal values: the lower index wins
    assert all(sampled_key(t) > logit_key(np.inf, 0) for t in (0, 5, 0x7FFFFFFF))
    assert all(logit_key(v, i) > 0 for v in vals for i in (0, 0x7FFFFFFF))   # 0 = "no key" stays below all
    assert [R.key_token(k) for k in (0, sampled_key(5), logit_key(-1.0, 12), 0xFFFFFFFF)] == [-1, 5, 12, 0]


# ------------------------------------------------------------------ step begin
def test_model_feedback_prompt_and_record():
    r = step_begin_ref(small_case())
    # s = 2: rows 0 and 1 are past their prompts (0 and 1 tokens) and feed back 4 and 2; row 2's prompt has 2
    # tokens, so it feeds back too (s == n_in): token 0
    assert r.tokens.tolist() == [4, 2, 0]
    assert r.h.tolist() == [[40, 41, 42, 43], [20, 21, 22, 23], [0, 1, 2, 3]] and r.h.dtype == f32
    assert r.pos.tolist() == [9, 2, 102]
    assert r.out_tokens.tolist() == [[-9, -9, 4], [-9, 2, -9], [0, -9, -9]]
    assert not r.argmax.any() and r.argmax.shape == (3, SLOTS)
    assert r.fold_x is None and r.fold_ss is None
    r = step_begin_ref(small_case(s=1))        # row 2 still in its prompt: in_tokens[2][1], nothing recorded
    assert r.tokens.tolist() == [4, 2, 2] and r.out_tokens.tolist() == [[-9, 4, -9], [2, -9, -9], [-9, -9, -9]]
    r = step_begin_ref(small_case(s=3))        # row 0: s - n_in == out_stride, not recorded
    assert r.out_tokens.tolist() == [[-9, -9, -9], [-9, -9, 2], [-9, 0, -9]]
    r = step_begin_ref(small_case(n_in=None, in_tokens=None))   # NULL n_in: every row feeds back, index s
    assert r.tokens.tolist() == [4, 2, 0] and r.out_tokens.tolist() == [[-9, -9, 4], [-9, -9, 2], [-9, -9, 0]]
    assert step_begin_ref(small_case(out_tokens=None)).out_tokens is None


def test_model_clamp_and_empty_row():
    c = small_case(s=0, n_in=np.array([1, 1, 0], np.int32), in_tokens=np.array([[-1], [5], [0]], np.int32))
    c.argmax[2] = 0
    r = step_begin_ref(c)
    assert r.tokens.tolist() == [0, 0, 0] and r.h.tolist() == [[0, 1, 2, 3]] * 3
    assert r.out_tokens.tolist() == [[-9] * 3, [-9] * 3, [-1, -9, -9]]     # the key's token, unclamped
    c.argmax[2] = keys_row((5, logit_key(1.0, 5)))                          # index == vocab
    r = step_begin_ref(c)
    assert r.tokens[2] == 0 and r.out_tokens[2, 0] == 5


def test_model_placeholder_and_fold():
    c = StepCase(argmax=np.zeros((1, SLOTS), np.uint64), base_pos=[0], s=0, hidden=103, placeholder_first=37)
    h = step_begin_ref(c).h[0]
    assert h.dtype == f32 and h[0] == f32(0.1) * f32(37) and h[62] == f32(0.1) * f32(99) and h[63] == 0 and h[102] == f32(0.1) * f32(39)
    assert step_begin_ref(c.at(s=2)).h[0][:3].tolist() == [0, f32(0.1), f32(0.1) * f32(2)]
    emb = np.array([[1.5, -2.0, 0.25, 3.0]], f16)
    w = np.array([2.0, 0.5, -4.0, 1.0 / 3.0], f32)
    r = step_begin_ref(StepCase(argmax=keys_row((0, logit_key(0.0, 0)))[None], base_pos=[0], s=0, emb=emb, fold_w=w))
    assert r.fold_x.dtype == f16 and r.fold_x.tolist() == [[3.0, -1.0, -1.0, float(f16(f32(3.0) * f32(1.0 / 3.0)))]]
    assert r.fold_ss.dtype == np.float64 and r.fold_ss.tolist() == [1.5 ** 2 + 4 + 0.0625 + 9]


class TieHighest(StepModel):
    def row_key(self, slots):
        best = max(int(k) >> 32 for k in slots)
        return min(int(k) for k in slots if int(k) >> 32 == best)


class NoClamp(StepModel):
    def gather_token(self, tok, vocab):
        return tok

    def emb_row(self, c, tok):   # what lies around the table: not row 0
        return c.emb[tok].astype(f32) if 0 <= tok < c.vocab else np.full(c.hidden, 777, f32)


class PosNoBase(StepModel):
    def pos(self, base, s):
        return s


class NotCleared(StepModel):
    def cleared(self, slots):
        return slots.copy()


class StrideInclusive(StepModel):
    def record_index(self, s, nin, out_stride):
        return s - nin if 0 <= s - nin <= out_stride else None


class StrideShort(StepModel):
    def record_index(self, s, nin, out_stride):
        return s - nin if 0 <= s - nin < out_stride - 1 else None


class PromptRecords(StepModel):
    def record_index(self, s, nin, out_stride):
        return s if s < nin and s < out_stride else StepModel.record_index(self, s, nin, out_stride)


class SsFirstStripe(StepModel):
    def fold_ss(self, h):
        return float(np.sum(h[:2048].astype(np.float64) ** 2))


class FoldF64(StepModel):
    def fold_x(self, h, w):
        return (h.astype(np.float64) * w.astype(np.float64)).astype(f16)


def fold_case(hidden, emb_row=None, fold_w=None):
    rng = np.random.RandomState(hidden)
    emb = rng.standard_normal((2, hidden)).astype(f16)
    if emb_row is not None:
        emb[1] = emb_row
    w = (1 + 0.1 * rng.standard_normal(hidden)).astype(f32) if fold_w is None else fold_w
    return StepCase(argmax=keys_row((4, logit_key(0.0, 1)))[None], base_pos=[0], s=0, emb=emb, fold_w=w)


def mutant_cases():
    tie = small_case()
    tie.argmax[0] = keys_row((2, logit_key(1.5, 7)), (20, logit_key(1.5, 3)), (21, logit_key(1.25, 0)))
    tie = tie.at(emb=np.arange(8 * 4).reshape(8, 4).astype(f16))
    clamp = small_case(s=0, n_in=np.array([1, 1, 0], np.int32), in_tokens=np.array([[-1], [5], [0]], np.int32))
    clamp.argmax[2] = 0
    v, w = double_rounding_input()
    assert v.size >= 4, "no double-rounding input found"
    return [
        ("tie goes to the highest index", TieHighest, tie),
        ("the clamp is missing", NoClamp, clamp),
        ("pos without base_pos", PosNoBase, small_case()),
        ("slots not cleared", NotCleared, small_case()),
        ("out_stride bound one too far", StrideInclusive, small_case(s=3)),
        ("out_stride bound one too near", StrideShort, small_case(s=2)),
        ("a prompt step writes out_tokens", PromptRecords, small_case(s=1)),
        ("fold_ss over the first 2048 elements only", SsFirstStripe, fold_case(2056)),
        ("fold_x rounded from a float64 product", FoldF64, fold_case(4, v[:4], w[:4])),
    ]


MUTANTS = mutant_cases()


@pytest.mark.parametrize("name,mutant,case", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_compare_rejects_mutant(name, mutant, case):
    ref = step_begin_ref(case)
    assert_step_equal(step_begin_ref(case), ref)                 # the model agrees with itself ...
    wrong = mutant().run(case)
    with pytest.raises(AssertionError):                          # ... and the mutant's result is rejected
        assert_step_equal(wrong, ref)
    # the mutant differs from the model in its own rule only: on a case the rule does not decide, it passes
    plain = fold_case(8) if case.fold_w is not None else small_case(n_in=None, in_tokens=None, s=0, base_pos=[0, 0, 0])
    if mutant not in (NotCleared, StrideShort):                  # (these two differ on every feedback step)
        assert_step_equal(mutant().run(plain), step_begin_ref(plain))


def test_double_rounding_input_exists():
    v, w = double_rounding_input()
    assert v.size >= 4
    once = (v.astype(np.float64) * w.astype(np.float64)).astype(f16)
    twice = (v.astype(f32) * w).astype(f16)
    assert np.all(once != twice) and np.all(np.isfinite(once))
    # one fp16 ulp apart: the fp32 product sits on an fp16 rounding boundary the exact product misses
    assert np.all(np.abs(once.view(np.int16).astype(int) - twice.view(np.int16).astype(int)) == 1)


def test_compare_is_exact_where_it_should_be():
    case = fold_case(2056)
    ref = step_begin_ref(case)

    def changed(field, fn):
        r = step_begin_ref(case)
        setattr(r, field, fn(getattr(r, field)))
        return r

    def flip_last(a):
        b = a.copy()
        b.reshape(-1).view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])[-1] ^= 1
        return b

    for field in ("h", "pos", "argmax", "fold_x"):
        with pytest.raises(AssertionError, match=field):
            assert_step_equal(changed(field, flip_last), ref)
    assert_step_equal(changed("fold_ss", lambda s: (s * (1 + 5e-6)).astype(f32)), ref)      # fp32 from a device
    for bad in (lambda s: s * (1 + 2e-5), lambda s: s * (1 - 2e-5), lambda s: s * np.nan):
        with pytest.raises(AssertionError, match="fold_ss"):
            assert_step_equal(changed("fold_ss", bad), ref)
    with pytest.raises(AssertionError, match="fold_x"):
        assert_step_equal(changed("fold_x", lambda x: None), ref)
    zero = step_begin_ref(case.at(emb=np.zeros_like(case.emb)))
    minus = step_begin_ref(case.at(emb=-np.zeros_like(case.emb)))
    with pytest.raises(AssertionError, match="h"):               # -0.0 is not +0.0: bits, not values
        assert_step_equal(minus, zero)


# ------------------------------------------------------------------ KV slot copy
def test_kv_copy_model():
    b = [np.arange(40, dtype=np.uint16), np.arange(100, 140, dtype=np.uint16)]
    keep = [x.copy() for x in b]
    out = kv_copy_ref(b, 2, 21, rows=2, row_pitch=8, row_elems=3)
    assert all(np.array_equal(x, k) for x, k in zip(b, keep))    # inputs untouched
    want = np.arange(40)
    want[21:24], want[29:32] = [2, 3, 4], [10, 11, 12]
    assert out[0].tolist() == want.tolist() and out[1].tolist() == (want + 100).tolist()
    assert out[0].dtype == np.uint16
    # source read whole before any write: overlapping rows take the old values
    o = kv_copy_ref([np.arange(12, dtype=np.uint16)], 0, 2, rows=2, row_pitch=4, row_elems=4)[0]
    assert o.tolist() == [0, 1, 0, 1, 2, 3, 4, 5, 6, 7, 10, 11]
    assert [x.tolist() for x in kv_copy_ref(b, 0, 8, rows=2, row_pitch=8, row_elems=0)] == [k.tolist() for k in keep]


def test_index_hash_has_no_near_repeats():
    h = R.index_hash(300000, salt=3)
    assert h.dtype == np.uint16
    for start in (0, 65536, 131072):
        assert np.unique(h[start:start + 65536]).size == 65536
    for shift in (1, 8, 2048, 65536, 131080):                          # a copy landing `shift` away shows
        assert np.count_nonzero(h[shift:] == h[:-shift]) < 16
    assert np.count_nonzero(h[:65536] == h[65536:131072]) < 16          # windows differ
    assert np.count_nonzero(h[:65536] == R.index_hash(65536, salt=4)) < 16   # buffers differ


def copy_ignores_pitch(buffers, src_off, dst_off, rows, row_pitch, row_elems):
    return kv_copy_ref(buffers, src_off, dst_off, rows, row_elems, row_elems)


def copy_whole_stripes_only(buffers, src_off, dst_off, rows, row_pitch, row_elems):
    return kv_copy_ref(buffers, src_off, dst_off, rows, row_pitch, row_elems // 2048 * 2048)


@pytest.mark.parametrize("chunks", [1, 255, 256, 257])
@pytest.mark.parametrize("mutant", [copy_ignores_pitch, copy_whole_stripes_only])
def test_buffers_compare_rejects_copy_mutant(mutant, chunks):
    row_elems, rows = 8 * chunks, 2
    pitch = row_elems + 8
    n = 8 + 2 * rows * pitch + 16
    bufs = [R.index_hash(n, t) for t in range(2)]
    args = (8, 8 + rows * pitch + 8, rows, pitch, row_elems)
    ref = kv_copy_ref(bufs, *args)
    R.assert_buffers_equal(kv_copy_ref(bufs, *args), ref)
    if mutant is copy_whole_stripes_only and chunks == 256:      # a whole stripe: the mutant is right here
        R.assert_buffers_equal(mutant(bufs, *args), ref)
        return
    with pytest.raises(AssertionError, match="buffer 0"):
        R.assert_buffers_equal(mutant(bufs, *args), ref)
