"""Test helper: the inputs of the ti_attn_prefill_f8 tests (test_gpu_kv8_prefill_attn.py on the GPU,
test_kv8_prefill_ref.py for the reference side on the CPU).  numpy / torch-CPU only.

`quantised` is attn_ref.make_inputs(..., shared=True) with K and V turned into e4m3 bytes by
kv8_ref.quantize, 0x7F (e4m3 NaN) in every cache row past the chunk's largest position, and the float64
reference attn_ref.attend over kv8_ref.decode of those very bytes.

`codes_inputs` is the "codes" case: kv_heads 4, G 1, M 40, pos 0 .. 39.  V element (kv-head i, key j, dim d)
is the e4m3 value of code (32 i + d mod 32) mod 127, the same for every key, optionally with the sign bit
set: the four heads cover the 127 non-negative finite codes (and 0x80 | code the negative ones), and since
the softmax weights sum to 1 every output element IS its code's value.  K is the quantised `flat` K.
"""
from __future__ import annotations

import numpy as np

import attn_ref as A
import kv8_ref as Q

f16, f32, f64 = np.float16, np.float32, np.float64

RING = 8                                   # the deepest ring (in blocks) of any e4m3 instance (prefill_attn.hip)
KVH = 2
M0 = max(288, 2 * 16 * RING + 32)          # two full rounds of every ring plus a block tail
SEQ0 = M0 + 32
POS0 = np.arange(M0, dtype=np.int32)
RANDOM_SEED = 1                            # the `random` cases' seed: their K bytes hold every subnormal code
SUBNORMAL_CODES = list(range(0x01, 0x08)) + list(range(0x81, 0x88))

CODES_KVH, CODES_M, CODES_SEQ = 4, 40, 48
CODES_POS = np.arange(CODES_M, dtype=np.int32)


def quantised(kind, values, M, heads, kvh, hd, max_seq, pos, seed):
    """-> q fp32 [M][heads * hd], kb, vb uint8 [1][kvh][max_seq][hd] (0x7F past max(pos)), ref [M][heads][hd] f64"""
    pos = np.asarray(pos, np.int32)
    q, kc, vc = A.make_inputs(kind, values, M, heads, kvh, hd, max_seq, pos, seed, shared=True)
    kb, vb = Q.quantize(kc), Q.quantize(vc)
    if values == "indicator":
        assert np.array_equal(Q.decode(vb), vc)                 # exact in e4m3
    ref, _ = A.attend(q, Q.decode(kb), Q.decode(vb), pos, heads)
    top = int(pos.max())
    kb[:, :, top + 1:] = Q.NAN_BYTE
    vb[:, :, top + 1:] = Q.NAN_BYTE
    return q, kb, vb, ref


def codes_v(hd, sign):
    """uint8 [1][4][CODES_SEQ][hd]: code (32 i + d mod 32) mod 127 (| 0x80 with sign) at every key."""
    i = np.arange(CODES_KVH)[:, None, None]
    d = np.arange(hd)[None, None, :]
    code = ((32 * i + d % 32) % 127).astype(np.uint8) | np.uint8(0x80 if sign else 0)
    return np.ascontiguousarray(np.broadcast_to(code, (CODES_KVH, CODES_SEQ, hd)))[None]


def codes_inputs(hd, sign):
    """-> q, kb, vb (0x7F past the chunk), the expected output [M][4][hd] f64 = each element's code value."""
    q, kc, _ = A.make_inputs("flat", "indicator", CODES_M, CODES_KVH, CODES_KVH, hd, CODES_SEQ, CODES_POS, 5, shared=True)
    kb, vb = Q.quantize(kc), codes_v(hd, sign)
    want = np.broadcast_to(Q.decode(vb[0, :, 0]).astype(f64), (CODES_M, CODES_KVH, hd)).copy()
    kb[:, :, CODES_M:] = Q.NAN_BYTE
    vb[:, :, CODES_M:] = Q.NAN_BYTE
    return q, kb, vb, want
