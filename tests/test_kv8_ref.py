"""The e4m3 helpers of tests/kv8_ref.py (CPU): what the GPU tests of the 8-bit KV cache compare with.

`quantize` is torch's CPU conversion to float8_e4m3fn behind an explicit clamp; the bytes pinned below
were observed with it and are what the format (include/ti_hip.h TI_BITS_KV8: round to nearest even of
min(max(x, -448), 448)) prescribes: 1.0625 and 1.1875 are ties between mantissas (to even: down to
1.0, up to 1.25), 17 a tie at a wider step (to 16), 460 is clamped, 2^-10 is the tie between 0 and the
smallest subnormal 2^-9 (to even: 0), 1e-3 lies above it.
"""
from __future__ import annotations

import numpy as np
import pytest

import attn_ref as A
import kv8_ref as Q

f16, f32, f64 = np.float16, np.float32, np.float64


def test_round_trip_of_the_254_finite_codes():
    codes = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], np.uint8)
    assert codes.size == 254
    vals = Q.decode(codes)
    assert vals.dtype == f16 and np.all(np.isfinite(vals))
    assert np.array_equal(Q.quantize(vals), codes)              # -0 keeps its sign: 0x80
    assert float(vals.astype(f64).max()) == 448.0 and float(vals.astype(f64).min()) == -448.0
    assert float(Q.decode(np.array([0x01], np.uint8))[0]) == 2.0 ** -9
    assert np.all(np.isnan(Q.decode(np.array([0x7F, 0xFF], np.uint8))))
    # ascending codes are ascending values (what `neighbours` is built on)
    assert np.all(np.diff(Q.decode(np.arange(0x7F, dtype=np.uint8)).astype(f64)) > 0)


@pytest.mark.parametrize("x,byte", [(1.0625, 0x38), (1.1875, 0x3A), (17.0, 0x58), (460.0, 0x7E), (2.0 ** -10, 0x00),
                                    (1e-3, 0x01), (-3.3, 0xC5), (500.0, 0x7E), (-1e9, 0xFE)])
def test_pinned_bytes(x, byte):
    assert int(Q.quantize(np.array([x], f32))[0]) == byte


def test_fnuz_reading_halves_every_value():
    codes = np.arange(0x7F, dtype=np.uint8)
    assert np.array_equal(Q.decode_fnuz(codes).astype(f64) * 2.0, Q.decode(codes).astype(f64))


def test_neighbours_and_append_rule():
    h = np.array([1.0, 1.06, 1.0625, 1.07, -3.3, 460.0, -70000.0, 0.0, 1e-3, 2.0 ** -10, 3e-4], f64)
    lo, hi = Q.neighbours(h)
    assert lo.tolist() == [1.0, 1.0, 1.0, 1.0, -3.5, 448.0, -448.0, 0.0, 0.0, 0.0, 0.0]
    assert hi.tolist() == [1.0, 1.125, 1.125, 1.125, -3.25, 448.0, -448.0, 0.0, 2.0 ** -9, 2.0 ** -9, 2.0 ** -9]
    is_nb, must, equal = Q.append_ok(Q.quantize(h), h)
    assert is_nb.all() and equal.all()
    # at a tie (1.0625, 2^-10) either neighbour is allowed; everywhere else the byte is quantize(h)'s
    assert must.tolist() == [True, True, False, True, True, True, True, True, True, False, True]
    # the other neighbour of a tie passes, of a non-tie fails; a byte two steps away is no neighbour
    is_nb, must, equal = Q.append_ok(np.array([0x39, 0x39, 0x3A], np.uint8), np.array([1.0625, 1.06, 1.06]))
    assert is_nb.tolist() == [True, True, False] and must.tolist() == [False, True, True]
    assert equal.tolist() == [False, False, False]


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("wrong", ["K", "V", "both"])
def test_reference_sees_the_wrong_exponent_bias(hd, wrong):
    """`flat` keys, `indicator` values, L = 64: the float64 reference over the bytes read with MI300's bias
    leaves `indicator_bound` around the one over the bytes read as OCP e4m3 -- halved values halve every
    output element; halved keys flatten the softmax.  Every head sees it."""
    heads, kvh, L = 4, 2, 64
    pos = np.array([L - 1], np.int32)
    q, kc, vc = A.make_inputs("flat", "indicator", 1, heads, kvh, hd, L + 1, pos, seed=0)
    kb, vb = Q.quantize(kc), Q.quantize(vc)
    assert np.array_equal(Q.decode(vb), vc)                     # indicator values are exact in e4m3
    good, _ = A.attend(q, Q.decode(kb), Q.decode(vb), pos, heads)
    bad, _ = A.attend(q, Q.decode_fnuz(kb) if wrong != "V" else Q.decode(kb),
                      Q.decode_fnuz(vb) if wrong != "K" else Q.decode(vb), pos, heads)
    over = np.abs(bad - good) / A.indicator_bound(good)
    assert np.all(over.max(axis=-1) >= 10), f"{wrong}: only {over.max(axis=-1).min():.1f} x the bound"
