"""ti_attn_prefill (prefill_attn.hip) in every kernel it can choose, against the float64 reference of
tests/attn_ref.py.

The rows of a chunk attend causally to ONE cache; row m's limit is pos[m].  With `indicator` values every
output element is a sum of a few keys' softmax weights, so a 16-key block masked one key early or late, a
dropped tail of a key-split half or a skipped ring slot fails attn_ref.indicator_bound at any length; the
rows past the chunk's largest position hold NaN.  Inputs and the bound: attn_ref.py.

Kernel instances (dispatch prefill_attn.hip:577-640; `instance()` below mirrors it for the labels and
assumes the MI355X's 256 CUs = 1024 SIMDs) and the cases that reach them, under each mode of
ti_attn_prefill_set_kernel (head_dim 64 under modes 0 and 1 only: the shared kernels are hd 128):
  per-wave, ring 4   attn_prefill_kernel<hd, 4> (:624-626, :631-633): grid <= 1024 waves
                     modes 0 and 1 of every case below except the shallow-ring shape
  per-wave, ring 3   attn_prefill_kernel<hd, 3, 2> (:627-629, :634-636): more than 1024 waves
                     M = 264, heads 64, kv_heads 4 (G 16: 1056 waves): hd 64 modes 0 and 1, hd 128 mode 1
  shared-K/V, 4 waves, LDS ring 6   attn_prefill_wg_kernel<1, 6> (:620-622): mode 2, hd 128, every case
  shared-K/V, 8 waves, LDS ring 8, key-split halves   attn_prefill_wg_kernel<2, 8> (:617-619): mode 3,
                     hd 128, every case; and mode 0 by itself at the shallow-ring shape (66 x 4 workgroups
                     x 4 >= 1024, :616)
  G in {1, 2, 4, 8, 16}: the chunk from position 0 (one case per G) and its other input kinds.
Cases: a chunk from position 0 (M = 288, pos = 0 .. 287: every row its own length -- lengths 1 .. 288, block
tails, two rounds of each ring, rows whose upper key-split half has no keys); long prefixes (pos 1000 .. 1039
of 1100, 2008 .. 2047 of 2048); 333 ragged positions of [0, 900); the shallow-ring shape.
After EVERY launch: K and V bit-identical, the 0xA5 pattern behind `out` intact.

Measured on an MI355X over every case of this module (printed at module teardown, `pytest -s`), worst
err / bound of the `indicator` cases over every G and kind | worst |got - ref| / (4e-3 + 4e-3 |ref|) of the
`random` cases:
  per-wave ring 4   hd 64 0.497 | 0.079, hd 128 0.496 | 0.079
  per-wave ring 3   hd 64 0.497, hd 128 0.495
  shared-K/V 4 waves 0.496 | 0.079;  shared-K/V 8 waves 0.496 | 0.079
The fp16 store alone is 0.5 of the bound; the hi + lo products add nothing that shows beside it (the three
hd 128 kernels give the same worst element).
"""
from __future__ import annotations

import numpy as np
import pytest

import attn_ref as A
from test_gpu_attn_oracle import GUARD, PAT, dev, fetch, guarded

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64
SIMDS = 1024            # 4 x 256 CUs (labels only)
MODES = {0: "auto", 1: "per_wave", 2: "shared4", 3: "shared8"}
MODE_HD = [(0, 64), (1, 64), (0, 128), (1, 128), (2, 128), (3, 128)]

WORST: dict = {}
_CASES: dict = {}


def note(label, value):
    WORST[label] = max(WORST.get(label, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    _CASES.clear()
    print("\nattn oracle (prefill), worst per instance:")
    for k in sorted(WORST):
        print(f"  {k:44s} {WORST[k]:.3e}")


@pytest.fixture(params=MODE_HD, ids=["%s-hd%d" % (MODES[m], hd) for m, hd in MODE_HD])
def mode_hd(request, ti):
    """ti_attn_prefill_set_kernel for the test, mode 0 restored afterwards."""
    mode, hd = request.param
    L = ti.lib()
    assert L.ti_attn_prefill_set_kernel(mode) == 0
    yield mode, hd
    assert L.ti_attn_prefill_set_kernel(0) == mode


def instance(mode, M, heads, kvh, hd):
    """The kernel a call takes (prefill_attn.hip:588-637), for labels."""
    G = heads // kvh
    gx = -(-M // (16 // G))
    if hd == 128 and (mode >= 2 or (mode == 0 and -(-gx // 4) * kvh * 4 >= SIMDS)):
        return "shared4 ring6" if mode == 2 else "shared8 ring8"
    return "per-wave " + ("ring4" if gx * kvh <= SIMDS else "ring3") + f" hd{hd}"


class PCase:
    def __init__(self, ti, kind, values, M, heads, kvh, hd, max_seq, pos, seed):
        self.ti, self.kind, self.values = ti, kind, values
        self.M, self.heads, self.kvh, self.hd, self.max_seq = M, heads, kvh, hd, max_seq
        self.pos = np.asarray(pos, np.int32)
        assert self.pos.shape == (M,) and self.pos.min() >= 0 and self.pos.max() < max_seq
        q, kc, vc = A.make_inputs(kind, values, M, heads, kvh, hd, max_seq, self.pos, seed, shared=True)
        self.row, _ = A.attend(q, kc, vc, self.pos, heads)
        kp, vp = A.poison(kc, vc, self.pos, shared=True)
        self.kd, self.vd, self.qd, self.pd = dev(ti, kp), dev(ti, vp), dev(ti, q), dev(ti, self.pos)
        self.k_bits, self.v_bits = kp.view(np.uint16).reshape(-1), vp.view(np.uint16).reshape(-1)


def pcase(ti, kind, values, M, heads, kvh, hd, max_seq, pos, seed=0):
    key = (kind, values, M, heads, kvh, hd, max_seq, np.asarray(pos, np.int32).tobytes(), seed)
    if key not in _CASES:
        _CASES[key] = PCase(ti, kind, values, M, heads, kvh, hd, max_seq, pos, seed)
    return _CASES[key]


def run_prefill(ti, c, mode):
    L = ti.lib()
    M, heads, hd = c.M, c.heads, c.hd
    nbytes = M * heads * hd * 2
    out = guarded(ti, nbytes)
    ti.check(L.ti_attn_prefill(c.qd.ptr, c.kd.ptr, c.vd.ptr, c.max_seq, c.pd.ptr, M, heads, c.kvh, hd, out.ptr, None))
    ti.sync()
    raw = fetch(ti, out, 0, nbytes + GUARD)
    assert np.all(raw[nbytes:] == PAT), "written behind out"
    for name, buf, bits in (("K", c.kd, c.k_bits), ("V", c.vd, c.v_bits)):
        assert np.array_equal(fetch(ti, buf, 0, bits.nbytes).view(np.uint16), bits), f"{name} changed by the launch"
    got = raw[:nbytes].view(f16).astype(f64).reshape(M, heads, hd)
    label = f"{instance(mode, M, heads, c.kvh, hd)} G{heads // c.kvh}"
    assert np.all(np.isfinite(got)), f"{label}: non-finite output at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    err = np.abs(got - c.row)
    if c.values == "indicator":
        over = err / A.indicator_bound(c.row)
        note(f"{label} {c.kind}", over.max())
        i = np.unravel_index(int(over.argmax()), over.shape)
        assert over.max() <= 1.0, (f"{label} {c.kind}: err / bound {over.max():.3g} at (row, head, d) {i}, "
                                   f"pos {int(c.pos[i[0]])}: got {got[i]!r}, ref {c.row[i]!r}")
    else:
        over = err / (A.ATOL + A.RTOL * np.abs(c.row))
        note(f"{label} random/4e-3", over.max())
        assert over.max() <= 1.0, f"{label}: random values off by {over.max():.3g} x (4e-3 + 4e-3 |ref|)"
    return label


KVH = 2
M0, SEQ0 = 288, 320
POS0 = np.arange(M0, dtype=np.int32)


@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
def test_chunk_from_position_zero(ti, mode_hd, G):
    """pos = 0 .. 287: every row is its own length, every row checked."""
    mode, hd = mode_hd
    run_prefill(ti, pcase(ti, "flat", "indicator", M0, KVH * G, KVH, hd, SEQ0, POS0), mode)


@pytest.mark.parametrize("kind,values", [("steep", "indicator"), ("ramp", "indicator"), ("flat", "random")])
def test_chunk_kinds(ti, mode_hd, kind, values):
    """The same chunk with a moving maximum, with a sawtooth of rising scores (the running maximum moves
    past the kernel's slack of 8 again and again) and with cancelling values, per G."""
    mode, hd = mode_hd
    for G in (1, 2, 4, 8, 16):
        run_prefill(ti, pcase(ti, kind, values, M0, KVH * G, KVH, hd, SEQ0, POS0, seed=1), mode)


@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("start,max_seq", [(1000, 1100), (2008, 2048)])
def test_long_prefix(ti, mode_hd, start, max_seq, G):
    """40 rows behind a long prefix; at 2048 keys an output element sums 16 (hd 128) or 32 keys."""
    mode, hd = mode_hd
    pos = (start + np.arange(40)).astype(np.int32)
    run_prefill(ti, pcase(ti, "flat", "indicator", 40, KVH * G, KVH, hd, max_seq, pos, seed=2), mode)


@pytest.mark.parametrize("G", [1, 4])
def test_ragged_positions(ti, mode_hd, G):
    """333 positions of [0, 900) in no order: blocks of mixed length, each row's own causal limit."""
    mode, hd = mode_hd
    pos = np.random.RandomState(hd + G).permutation(900)[:333].astype(np.int32)
    run_prefill(ti, pcase(ti, "flat", "indicator", 333, KVH * G, KVH, hd, 1024, pos, seed=3), mode)


def test_shallow_ring_shape(ti, mode_hd):
    """M = 264, heads 64, kv_heads 4: 1056 waves, more than one per SIMD.  The per-wave kernel then takes the
    3-deep ring; at hd 128 mode 0 chooses the 8-wave shared-K/V kernel by itself."""
    mode, hd = mode_hd
    M, heads, kvh = 264, 64, 4
    want = {(0, 64): "per-wave ring3 hd64", (1, 64): "per-wave ring3 hd64", (0, 128): "shared8 ring8",
            (1, 128): "per-wave ring3 hd128", (2, 128): "shared4 ring6", (3, 128): "shared8 ring8"}[(mode, hd)]
    assert instance(mode, M, heads, kvh, hd) == want
    run_prefill(ti, pcase(ti, "flat", "indicator", M, heads, kvh, hd, 272, np.arange(M, dtype=np.int32), seed=4), mode)
