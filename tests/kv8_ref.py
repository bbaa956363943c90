"""Test helper: the e4m3 KV cache format (TI_BITS_KV8, include/ti_hip.h) on the CPU.

One byte per element, OCP e4m3fn (1 sign, 4 exponent bits with bias 7, 3 mantissa bits; 0x7F / 0xFF are
NaN, no infinities, largest finite 448), no scale:
    byte = round-to-nearest-even e4m3 of min(max(x, -448), 448)
`quantize` is torch's CPU conversion behind an explicit clamp (unclamped, it turns 500 into NaN);
`decode` is exact, since every e4m3 value is an fp16 value.  `decode_fnuz` reads the same bytes with
the e4m3fnuz bias of 8 (MI300's format): every value halved -- what a kernel built on the wrong
conversion would see, used to show that the GPU tests' reference notices it.

`neighbours` / `append_ok` state what an appended byte may be when the test knows the fp16 rounding h of
the fp32 value the epilogue converted: the two values differ by at most 2^-11 |h| (fp16 has 11
significant bits), so the byte decodes to one of the two e4m3 neighbours of clamp(h), and equals
quantize(h) whenever h lies further than 2^-10 |h| from the midpoint of those neighbours.
"""
from __future__ import annotations

import numpy as np
import torch

f16, f32, f64 = np.float16, np.float32, np.float64
E4M3_MAX = 448.0
NAN_BYTE = 0x7F


def quantize(x) -> np.ndarray:
    """float array -> uint8 e4m3 bytes (clamp to +-448, round to nearest even, subnormals included)."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=f32)).clamp(-E4M3_MAX, E4M3_MAX)
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()


def decode(u8) -> np.ndarray:
    """uint8 e4m3 bytes -> float16, exactly (0x7F / 0xFF -> NaN)."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(u8), dtype=np.uint8))
    return t.view(torch.float8_e4m3fn).to(torch.float16).numpy().copy()


def decode_fnuz(u8) -> np.ndarray:
    """The same bytes read with the e4m3fnuz exponent bias (8 instead of 7): every value halved."""
    return (decode(u8).astype(f32) * f32(0.5)).astype(f16)


# the 127 non-negative finite values, ascending (code c < 0x7F decodes to _GRID[c])
_GRID = decode(np.arange(0x7F, dtype=np.uint8)).astype(f64)


def neighbours(h):
    """h (any float array) -> (lo, hi) float64: the largest e4m3 value <= clamp(h) and the smallest >=
    clamp(h) (equal where clamp(h) is an e4m3 value)."""
    c = np.clip(np.asarray(h, f64), -E4M3_MAX, E4M3_MAX)
    a = np.abs(c)
    i_hi = np.searchsorted(_GRID, a, side="left")          # first grid value >= a
    i_lo = np.where(_GRID[i_hi] == a, i_hi, i_hi - 1)
    lo_a, hi_a = _GRID[i_lo], _GRID[i_hi]
    neg = c < 0
    return np.where(neg, -hi_a, lo_a), np.where(neg, -lo_a, hi_a)


def append_ok(byte, h):
    """byte (uint8 array written by an append), h (the fp16-cache value of the same element) ->
    (is_neighbour, must_equal, equal): boolean arrays.  The rule: is_neighbour everywhere, and equal
    wherever must_equal (module docstring)."""
    h64 = np.asarray(h, f64)
    got = decode(byte).astype(f64)
    lo, hi = neighbours(h64)
    is_nb = (got == lo) | (got == hi)
    c = np.clip(h64, -E4M3_MAX, E4M3_MAX)
    # (clamp(h) itself an e4m3 value: lo == hi, no midpoint near, the byte is that value's)
    must = (lo == hi) | (np.abs(c - 0.5 * (lo + hi)) > 2.0 ** -10 * np.abs(h64))
    equal = np.asarray(byte, np.uint8) == quantize(h64.astype(f32))
    return is_nb, must, equal
