"""The reference side of test_gpu_kv8_prefill_attn.py, on the CPU.

The "codes" case gives every finite e4m3 byte as a V value (kv8_prefill_cases.codes_inputs) and asks each
output element to equal its code's value within attn_ref.indicator_bound.  Shown here with attn_ref.attend
over kv8_ref.decode(bytes): a kernel that flushed the e4m3 subnormals to zero, dropped the sign bit or read
the bytes with the fnuz exponent bias would leave that bound at some output element -- so within each head
the largest value is small enough for the subnormal codes to show beside the 2^-18 max|ref[h]| term.
The K path has no isolated case; the `random` cases' K bytes hold every subnormal code, checked here.
"""
from __future__ import annotations

import numpy as np
import pytest

import attn_ref as A
import kv8_prefill_cases as K8
import kv8_ref as Q

f16, f32, f64 = np.float16, np.float32, np.float64


def _flush_subnormals(v):
    v = v.copy()
    v[np.abs(v.astype(f64)) < 2.0 ** -6] = 0          # e4m3's smallest normal is 2^-6
    return v


WRONG = {"subnormals flushed": _flush_subnormals,
         "sign dropped": lambda v: np.abs(v),
         "fnuz bias": None}


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("sign", [0, 1])
def test_codes_reference_is_the_code_value(hd, sign):
    q, kb, vb, want = K8.codes_inputs(hd, sign)
    codes = set(int(c) for c in np.unique(vb[0, :, 0]))
    assert codes == {c | (0x80 if sign else 0) for c in range(127)}           # every finite code of that sign
    ref, _ = A.attend(q, Q.decode(kb), Q.decode(vb), K8.CODES_POS, K8.CODES_KVH)
    # the softmax weights sum to 1: float64 attention returns the value itself (to float64 rounding)
    assert np.all(np.abs(ref - want) <= 1e-12 * np.maximum(np.abs(want), 1e-30) + 1e-300)
    assert np.all(np.abs(ref - want) / A.indicator_bound(want) < 1e-6)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("wrong", list(WRONG))
def test_codes_case_sees_a_wrong_widening(hd, wrong):
    sign = 1 if wrong == "sign dropped" else 0
    q, kb, vb, want = K8.codes_inputs(hd, sign)
    good = Q.decode(vb)
    bad = Q.decode_fnuz(vb) if wrong == "fnuz bias" else WRONG[wrong](good)
    got, _ = A.attend(q, Q.decode(kb), bad, K8.CODES_POS, K8.CODES_KVH)
    over = np.abs(got - want) / A.indicator_bound(want)
    assert over.max() > 1.0, f"{wrong}: stays within the bound ({over.max():.3g})"
    if wrong == "subnormals flushed":
        # each of the 7 subnormal codes on its own leaves the bound (head 0 holds codes 0 .. 31)
        for code in range(1, 8):
            assert over[:, 0, code].min() > 1.0, code


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("wrong", list(WRONG))
def test_k_side_faults_leave_the_bound(hd, wrong):
    """The same three faults on the K bytes of the smallest `indicator` chunk case move the softmax enough to
    leave indicator_bound: what the GPU cases rest on for the K path."""
    G = 1
    M, pos = 40, np.arange(40, dtype=np.int32)
    q, kb, vb, ref = K8.quantised("flat", "indicator", M, K8.KVH * G, K8.KVH, hd, 48, pos, 0)
    kgood = Q.decode(kb)
    kbad = Q.decode_fnuz(kb) if wrong == "fnuz bias" else WRONG[wrong](kgood)
    got, _ = A.attend(q, kbad, Q.decode(vb), pos, K8.KVH * G)
    over = np.abs(got - ref) / A.indicator_bound(ref)
    assert over.max() > 1.0, f"{wrong}: stays within the bound ({over.max():.3g})"


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("G", [2, 4])
def test_random_cases_hold_every_subnormal_code_in_k(hd, G):
    """The K bytes (rows the chunk uses) of the GPU module's `random` cases, G 4 per-wave and G 2 shared-K/V."""
    q, kb, vb, ref = K8.quantised("flat", "random", K8.M0, K8.KVH * G, K8.KVH, hd, K8.SEQ0, K8.POS0, K8.RANDOM_SEED)
    used = kb[0, :, :K8.M0]
    for kvh in range(K8.KVH):
        have = set(int(c) for c in np.unique(used[kvh]))
        missing = [hex(c) for c in K8.SUBNORMAL_CODES if c not in have]
        assert not missing, f"kv-head {kvh}: K lacks the subnormal codes {missing}"
    assert np.all(kb[0, :, K8.M0:] == Q.NAN_BYTE)
