"""ti_attn_prefill_f8 (prefill_attn.hip, the KV8 instances) in every kernel it can choose, against the
float64 reference of tests/attn_ref.py over the very e4m3 bytes uploaded.

Inputs: kv8_prefill_cases.quantised -- attn_ref.make_inputs(..., shared=True), K and V quantised by
kv8_ref.quantize (`indicator` values are exact in e4m3), the reference attn_ref.attend over
kv8_ref.decode(bytes); every cache row past the chunk's largest position holds 0x7F (e4m3 NaN).
Bounds, both the project's: attn_ref.indicator_bound for `indicator` values, ATOL = RTOL = 4e-3 for `random`.

Kernel instances (the dispatch is ti_attn_prefill's own, pf_launch in prefill_attn.hip; `instance()` mirrors
it for the labels and assumes the MI355X's 256 CUs = 1024 SIMDs), under each mode of
ti_attn_prefill_set_kernel, which governs both entry points (head_dim 64 under modes 0 and 1 only):
  per-wave, ring 4   attn_prefill_kernel<hd, 4, 1, KV8>: grid <= 1024 waves
  per-wave, ring 3   attn_prefill_kernel<hd, 3, 2, KV8>: the shallow-ring shape, hd 64 modes 0 and 1, hd 128 mode 1
  shared-K/V, 4 waves, LDS ring 6   attn_prefill_wg_kernel<1, 6, KV8>: mode 2, hd 128
  shared-K/V, 8 waves, LDS ring 8, key-split halves   attn_prefill_wg_kernel<2, 8, KV8>: mode 3, hd 128, and
                     mode 0 by itself at the shallow-ring shape
Cases (each the smallest that reaches what it names):
  chunk from position 0   M0 = max(288, 2 * 16 * 8 + 32) = 288 rows, pos = 0 .. 287, max_seq 320, kv_heads 2,
                     G in {1, 2, 4, 8, 16}, flat / indicator: two full rounds of the deepest ring (8 blocks)
                     plus a block tail, every row its own length; for one G per kernel family (per-wave
                     G 4, shared G 2) also steep and ramp indicator and flat random
  40 rows behind a long prefix   pos 2008 .. 2047 of 2048, G in {1, 4}
  ragged positions   333 positions of [0, 900) in no order, max_seq 1024, G in {1, 4}: blocks of mixed
                     length, waves that only copy, upper key-split halves with no keys
  the shallow-ring shape   M = 264, heads 64, kv_heads 4 (1056 waves)
  codes              kv_heads 4, G 1, M 40: V = the e4m3 value of code (32 i + d mod 32) mod 127 at every
                     key, once as is and once with the sign bit set, so every output element must equal its
                     code's value within indicator_bound: all 254 finite bytes widen exactly on the V path
                     of both kernel families (test_kv8_prefill_ref.py shows on the CPU that a flushed
                     subnormal, a dropped sign or the fnuz bias leaves the bound).  K has no such isolated
                     case: its exactness rests on the ONE helper both paths share (common.hpp
                     e4m3x4_to_f16x4) and on the `random` cases, whose K bytes hold every subnormal code
                     (checked on the CPU in test_kv8_prefill_ref.py).
After EVERY launch: K and V bytes identical to the upload, 0x7F in every cache row past the chunk's largest
position, the 0xA5 pattern behind `out` intact, the output finite.

Measured on an MI355X over every case of this module (printed at module teardown, `pytest -s`), worst
err / bound of the `indicator` cases over every G and kind | worst |got - ref| / (4e-3 + 4e-3 |ref|) of the
`random` cases | worst err / bound of the codes cases:
  per-wave ring 4   hd 64 0.495 | 0.061 | 0.000, hd 128 0.501 | 0.079 | 0.000
  per-wave ring 3   hd 64 0.493, hd 128 0.495
  shared-K/V 4 waves 0.495 | 0.080 | 0.000;  shared-K/V 8 waves 0.495 | 0.080 | 0.000
As in the fp16 kernels the fp16 store alone is 0.5 of the bound and nothing shows beside it (0.501: the ramp
kind at hd 128, G 4; the fp16 module's worst is 0.497): the widening adds no term, and the codes cases
come out bit-exact (every element the fp16 value of its byte).
"""
from __future__ import annotations

import numpy as np
import pytest

import attn_ref as A
import kv8_prefill_cases as K8
import kv8_ref as Q
from test_gpu_attn_oracle import GUARD, PAT, dev, fetch, guarded
from test_gpu_prefill_attn_oracle import MODE_HD, MODES

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64
SIMDS = 1024            # 4 x 256 CUs (labels only)

WORST: dict = {}
_CASES: dict = {}


def note(label, value):
    WORST[label] = max(WORST.get(label, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    _CASES.clear()
    print("\nattn oracle (e4m3 prefill), worst per instance:")
    for k in sorted(WORST):
        print(f"  {k:52s} {WORST[k]:.3e}")


@pytest.fixture(params=MODE_HD, ids=["%s-hd%d" % (MODES[m], hd) for m, hd in MODE_HD])
def mode_hd(request, ti):
    """ti_attn_prefill_set_kernel for the test, mode 0 restored afterwards."""
    mode, hd = request.param
    L = ti.lib()
    assert L.ti_attn_prefill_set_kernel(mode) == 0
    yield mode, hd
    assert L.ti_attn_prefill_set_kernel(0) == mode


def instance(mode, M, heads, kvh, hd):
    """The kernel a call takes (pf_launch in prefill_attn.hip), for labels."""
    G = heads // kvh
    gx = -(-M // (16 // G))
    if hd == 128 and (mode >= 2 or (mode == 0 and -(-gx // 4) * kvh * 4 >= SIMDS)):
        return "f8 shared4 ring6" if mode == 2 else "f8 shared8 ring8"
    return "f8 per-wave " + ("ring4" if gx * kvh <= SIMDS else "ring3") + f" hd{hd}"


class PCase:
    def __init__(self, ti, M, heads, kvh, hd, max_seq, pos, values, kind, built):
        self.ti, self.kind, self.values = ti, kind, values
        self.M, self.heads, self.kvh, self.hd, self.max_seq = M, heads, kvh, hd, max_seq
        self.pos = np.asarray(pos, np.int32)
        assert self.pos.shape == (M,) and self.pos.min() >= 0 and self.pos.max() < max_seq
        q, kb, vb, self.row = built
        assert kb.dtype == np.uint8 and kb.shape == vb.shape == (1, kvh, max_seq, hd)
        self.top = int(self.pos.max())
        assert np.all(kb[:, :, self.top + 1:] == Q.NAN_BYTE) and np.all(vb[:, :, self.top + 1:] == Q.NAN_BYTE)
        self.kd, self.vd, self.qd, self.pd = dev(ti, kb), dev(ti, vb), dev(ti, q), dev(ti, self.pos)
        self.k_bytes, self.v_bytes = kb.reshape(-1).copy(), vb.reshape(-1).copy()


def pcase(ti, kind, values, M, heads, kvh, hd, max_seq, pos, seed=0):
    key = (kind, values, M, heads, kvh, hd, max_seq, np.asarray(pos, np.int32).tobytes(), seed)
    if key not in _CASES:
        _CASES[key] = PCase(ti, M, heads, kvh, hd, max_seq, pos, values, kind,
                            K8.quantised(kind, values, M, heads, kvh, hd, max_seq, pos, seed))
    return _CASES[key]


def codes_case(ti, hd, sign):
    key = ("codes", hd, sign)
    if key not in _CASES:
        _CASES[key] = PCase(ti, K8.CODES_M, K8.CODES_KVH, K8.CODES_KVH, hd, K8.CODES_SEQ, K8.CODES_POS, "codes",
                            "flat-" if sign else "flat+", K8.codes_inputs(hd, sign))
    return _CASES[key]


def run_prefill(ti, c, mode):
    L = ti.lib()
    M, heads, hd = c.M, c.heads, c.hd
    nbytes = M * heads * hd * 2
    out = guarded(ti, nbytes)
    ti.check(L.ti_attn_prefill_f8(c.qd.ptr, c.kd.ptr, c.vd.ptr, c.max_seq, c.pd.ptr, M, heads, c.kvh, hd, out.ptr, None))
    ti.sync()
    raw = fetch(ti, out, 0, nbytes + GUARD)
    assert np.all(raw[nbytes:] == PAT), "written behind out"
    for name, buf, want in (("K", c.kd, c.k_bytes), ("V", c.vd, c.v_bytes)):
        now = fetch(ti, buf, 0, want.nbytes)
        assert np.array_equal(now, want), f"{name} changed by the launch"
        assert np.all(now.reshape(c.kvh, c.max_seq, hd)[:, c.top + 1:] == Q.NAN_BYTE), f"{name}: no 0x7F past row {c.top}"
    got = raw[:nbytes].view(f16).astype(f64).reshape(M, heads, hd)
    label = f"{instance(mode, M, heads, c.kvh, hd)} G{heads // c.kvh}"
    assert np.all(np.isfinite(got)), f"{label}: non-finite output at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    err = np.abs(got - c.row)
    if c.values in ("indicator", "codes"):
        over = err / A.indicator_bound(c.row)
        note(f"{label} {c.kind}" + (" codes" if c.values == "codes" else ""), over.max())
        i = np.unravel_index(int(over.argmax()), over.shape)
        print(f"{label} {c.kind} {c.values}: err / bound {over.max():.3f}")
        assert over.max() <= 1.0, (f"{label} {c.kind} {c.values}: err / bound {over.max():.3g} at (row, head, d) {i}, "
                                   f"pos {int(c.pos[i[0]])}: got {got[i]!r}, ref {c.row[i]!r}")
    else:
        over = err / (A.ATOL + A.RTOL * np.abs(c.row))
        note(f"{label} random/4e-3", over.max())
        print(f"{label} random: {over.max():.3f} x (4e-3 + 4e-3 |ref|)")
        assert over.max() <= 1.0, f"{label}: random values off by {over.max():.3g} x (4e-3 + 4e-3 |ref|)"
    return label


@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
def test_chunk_from_position_zero(ti, mode_hd, G):
    """pos = 0 .. M0 - 1: every row is its own length, every row checked."""
    mode, hd = mode_hd
    run_prefill(ti, pcase(ti, "flat", "indicator", K8.M0, K8.KVH * G, K8.KVH, hd, K8.SEQ0, K8.POS0), mode)


@pytest.mark.parametrize("kind,values", [("steep", "indicator"), ("ramp", "indicator"), ("flat", "random")])
def test_chunk_kinds(ti, mode_hd, kind, values):
    """The same chunk with a moving maximum, with a sawtooth of rising scores and with cancelling values, at
    one G per kernel family (per-wave: 4, shared-K/V: 2; mode 0 takes the per-wave kernel at this size)."""
    mode, hd = mode_hd
    G = 2 if mode >= 2 else 4
    run_prefill(ti, pcase(ti, kind, values, K8.M0, K8.KVH * G, K8.KVH, hd, K8.SEQ0, K8.POS0, seed=K8.RANDOM_SEED), mode)


@pytest.mark.parametrize("G", [1, 4])
def test_long_prefix(ti, mode_hd, G):
    """40 rows behind a long prefix; at 2048 keys an output element sums 16 (hd 128) or 32 keys."""
    mode, hd = mode_hd
    pos = (2008 + np.arange(40)).astype(np.int32)
    run_prefill(ti, pcase(ti, "flat", "indicator", 40, K8.KVH * G, K8.KVH, hd, 2048, pos, seed=2), mode)


@pytest.mark.parametrize("G", [1, 4])
def test_ragged_positions(ti, mode_hd, G):
    """333 positions of [0, 900) in no order: blocks of mixed length, each row's own causal limit."""
    mode, hd = mode_hd
    pos = np.random.RandomState(hd + G).permutation(900)[:333].astype(np.int32)
    run_prefill(ti, pcase(ti, "flat", "indicator", 333, K8.KVH * G, K8.KVH, hd, 1024, pos, seed=3), mode)


def test_shallow_ring_shape(ti, mode_hd):
    """M = 264, heads 64, kv_heads 4: 1056 waves, more than one per SIMD.  The per-wave kernel then takes the
    3-deep ring; at hd 128 mode 0 chooses the 8-wave shared-K/V kernel by itself."""
    mode, hd = mode_hd
    M, heads, kvh = 264, 64, 4
    want = {(0, 64): "f8 per-wave ring3 hd64", (1, 64): "f8 per-wave ring3 hd64", (0, 128): "f8 shared8 ring8",
            (1, 128): "f8 per-wave ring3 hd128", (2, 128): "f8 shared4 ring6", (3, 128): "f8 shared8 ring8"}[(mode, hd)]
    assert instance(mode, M, heads, kvh, hd) == want
    run_prefill(ti, pcase(ti, "flat", "indicator", M, heads, kvh, hd, 272, np.arange(M, dtype=np.int32), seed=4), mode)


@pytest.mark.parametrize("sign", [0, 1], ids=["positive", "negative"])
def test_codes(ti, mode_hd, sign):
    """Every finite e4m3 byte as a V value: the output element is that byte's value."""
    mode, hd = mode_hd
    run_prefill(ti, codes_case(ti, hd, sign), mode)
