"""ti_attn_decode, ti_attn_decode_packed and ti_attn_decode_partials (attention.hip, attention_body.hpp)
against the float64 reference of tests/attn_ref.py.

The reference knows nothing of splits, slots, rings or lane layouts; the inputs (`flat`, `steep`, `ramp`
keys; `indicator` or `random` values; NaN behind every stream's limit) and the bound for `indicator`
outputs are described and derived in attn_ref.py.  With `indicator` values every output element is a sum
of a few keys' softmax weights, so one lost, doubled or wrongly admitted key fails the bound at any length
(test_attn_ref.py shows it on the reference side).

Kernel instances (attn_split_kernel<HD, G, R, HP>; dispatch attention.hip:46-81, body
attention_body.hpp:125; `instance()` below mirrors the dispatch for the labels only) and the cases that
reach them.  A pass is 8 waves x KPW keys (KPW 4 at hd 128, 8 at hd 64), head-parallel 8 keys:
  ring 2   <hd, 1, 2>  M > 1 MHA (attention.hip:69)         length sweep G1, kinds, stride, reuse
           <hd, 2, 2>  G = 2 (:69)                          length sweep G2, packed hd 64, partials M = 5
           <64, 4, 2>, <128, 8, 2>  (:52 false, :69)        length sweep, kinds, partials M = 5
  ring 3   <hd, 1, 3>  G = 1 and M = 1 (:67)                M = 1 sweep (decode and partials), 7B long context
           the same with kv_shift: partials, M = 1, heads > kv_heads, head by head (attention.hip:113-121)
                                                            M = 1 sweep `expand`, G in {2, 4, 8}
  ring 8   <128, 4, 8, HP>, <64, 8, 8, HP>  head-parallel lanes, max_seq / splits < 1024 (:52-53)
                                                            length sweep, kinds, packed hd 128, partials M = 5
  ring 4   <hd, 4 | 8, 4>  max_seq / splits >= 1024 (:48, :64-65), not head-parallel
                                                            long-range sweep (max_seq 1024, splits 1; the same
                                                            buffers with splits 3, 8, 64 leave the long range and
                                                            run ring 2 / ring 8), long contexts (max_seq 2048,
                                                            splits 1 and 2), partials at max_seq 2048 splits 2
  output   splits == 1 direct (attention_body.hpp:352); splits > 1 merged in the launch by the last
           arriver (:383-419), empty splits included (splits 64 over L < 64); the clamp at
           attn_max_splits (attention.hip:124: 45 / 22 at hd 64 G 4 / 8, 46 / 23 / 11 at hd 128 G 2 / 4 / 8) is
           crossed by splits = 64 in the length and long-range sweeps;
           partials (:356-360); packed order (:146-151) at M = 17, 45, 64.
Every launch writes into buffers of exactly the advertised size with a 0xA5 pattern behind them (out,
part_o, part_ml, the workspace), checked after every launch; K and V are compared bit for bit after
the launch on one case per entry point (test_memory_discipline).  ti_attn_decode_packed leaves rows
M .. 16 ceil(M / 16) of its output unwritten (the pattern is intact there; ti_hip.h would allow writing them,
so this is recorded by test_packed_output, not required).

Measured on an MI355X over every case of this module (printed at module teardown, `pytest -s`), worst
err / bound of the `indicator` cases (flat, steep and ramp together) | worst |got - ref| / (4e-3 + 4e-3 |ref|)
of the `random` cases:
  ring 2   hd 64:  G1 0.487 | 0.058, G2 0.490 | 0.054, G4 0.494 | 0.050; packed G2 0.490;
                   partials G1 0.476 | 0.047, G2 0.488 | 0.060, G4 0.479 | 0.055
           hd 128: G1 0.488 | 0.058, G2 0.490 | 0.056, G8 0.493 | 0.057;
                   partials G1 0.473 | 0.066, G2 0.452 | 0.073, G8 0.482 | 0.072
  ring 3   hd 64 0.488 | 0.013, partials (expanded GQA included) 0.489 | 0.014;
           hd 128 0.484 | 0.013, partials (expanded GQA included) 0.492 | 0.016
  ring 8   hd 128 G4 0.492 | 0.060, packed 0.492, partials 0.484 | 0.068;
           hd 64 G8 0.493 | 0.058, partials 0.482 | 0.065
  ring 4   hd 64 G4 0.493 | 0.042, G8 0.492 | 0.058, partials 0.472, 0.447;
           hd 128 G4 0.484 | 0.057, G8 0.492 | 0.060, partials 0.452, 0.446
The fp16 store alone is 0.5 of the bound (2^-11 |ref| of 2^-10 |ref|): the kernels' own fp32 arithmetic adds
nothing that shows beside it, so no instance needed a further term.
Logsumexp of the partials (host merge) against float64 over all partials cases of the module: worst
6.70e-6 (1.2e-7 over the flat cases with L <= 64); LSE_TOL = 4 x the worst = 2.7e-5.  That is below
0.5 / (L + 1) for every L <= 64 (7.7e-3 at L = 64) and indeed for every L <= 2048 (2.4e-4), so the logsumexp
check alone sees one lost key of a flat softmax at every length of this module.
A library whose four attention kernels ignore key 1000 (a change of values only) fails every case of this
module and of test_gpu_prefill_attn_oracle.py that holds key 1000 and accounts for keys (42 cases: all
but the `ramp` ones), and passes the rest.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import attn_ref as A

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64
GUARD = 4096            # pattern bytes behind every buffer a launch writes
PAT = 0xA5
LSE_TOL = 2.7e-5        # 4 x the measured worst, 6.70e-6 (module docstring)

WORST: dict = {}
_CASES: dict = {}


def note(label, value):
    WORST[label] = max(WORST.get(label, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    _CASES.clear()
    print("\nattn oracle (decode), worst per instance:")
    for k in sorted(WORST):
        print(f"  {k:44s} {WORST[k]:.3e}")


# ------------------------------------------------------------------ device plumbing
def dev(ti, a):
    return ti.DeviceBuffer.from_array(np.ascontiguousarray(a))


def fill(ti, buf, off, nbytes, byte):
    ti.check(ti.lib().ti_memset(buf.ptr + off, byte, nbytes, None))


def fetch(ti, buf, off, nbytes):
    out = np.empty(nbytes, np.uint8)
    ti.check(ti.lib().ti_memcpy_d2h(C.c_void_p(out.ctypes.data), buf.ptr + off, nbytes, None))
    return out


def guarded(ti, nbytes):
    """A buffer of nbytes + GUARD, all 0xA5."""
    b = ti.DeviceBuffer(nbytes + GUARD)
    fill(ti, b, 0, nbytes + GUARD, PAT)
    return b


def guard_intact(ti, buf, nbytes, what):
    assert np.all(fetch(ti, buf, nbytes, GUARD) == PAT), f"written behind {what}"


def instance(M, G, hd, max_seq, splits, partials=False):
    """The kernel instance a call takes: the dispatch of attention.hip:46-81 and :113-124, for labels."""
    expand = partials and M == 1 and G > 1
    g = 1 if expand else G
    if not partials:
        splits = min(splits, max(1, (48 * 1024) // (g * (hd + 4) * 4)))
    long_range = g >= 4 and max_seq // splits >= 1024
    if g >= 4 and hd // (64 // g) == 8 and not long_range:
        ring = "ring8hp"
    elif long_range:
        ring = "ring4long"
    elif g == 1 and M == 1:
        ring = "ring3"
    else:
        ring = "ring2"
    return f"{ring} hd{hd} G{g}" + (f" expand{G}" if expand else "")


class Case:
    """Seeded inputs on the device (NaN behind every limit) and their float64 reference."""

    def __init__(self, ti, kind, values, M, heads, kvh, hd, max_seq, pos, seed=0, shared=False, pad=0, keep=False,
                 poisoned=True):
        self.ti, self.kind, self.values = ti, kind, values
        self.M, self.heads, self.kvh, self.hd, self.max_seq = M, heads, kvh, hd, max_seq
        self.G = heads // kvh
        self.pos = np.asarray(pos, np.int32)
        assert self.pos.shape == (M,) and self.pos.min() >= 0 and self.pos.max() < max_seq
        q, kc, vc = A.make_inputs(kind, values, M, heads, kvh, hd, max_seq, self.pos, seed, shared=shared)
        self.row, self.lse = A.attend(q, kc, vc, self.pos, heads)
        kp, vp = A.poison(kc, vc, self.pos, shared=shared) if poisoned else (kc, vc)   # (Walk poisons on the device)
        del kc, vc
        n = kvh * max_seq * hd
        if pad:     # a stream stride larger than one stream's cache; the gap holds NaN
            assert not shared and pad % 8 == 0
            wide_k, wide_v = np.full((M, n + pad), np.nan, f16), np.full((M, n + pad), np.nan, f16)
            wide_k[:, :n], wide_v[:, :n] = kp.reshape(M, n), vp.reshape(M, n)
            kp, vp = wide_k, wide_v
        self.stride = 0 if shared else n + pad
        self.kd, self.vd, self.qd, self.pd = dev(ti, kp), dev(ti, vp), dev(ti, q), dev(ti, self.pos)
        self.k_bits, self.v_bits = (kp.view(np.uint16).copy(), vp.view(np.uint16).copy()) if keep else (None, None)

    def kv_unchanged(self):
        assert self.k_bits is not None
        for name, buf, bits in (("K", self.kd, self.k_bits), ("V", self.vd, self.v_bits)):
            got = fetch(self.ti, buf, 0, bits.nbytes).view(np.uint16)
            assert np.array_equal(got, bits.reshape(-1)), f"{name} changed by the launch"


def case(ti, *args, **kw):
    """One Case per set of arguments for the module (inputs uploaded and the reference computed once)."""
    key = tuple(a.tobytes() if isinstance(a, np.ndarray) else a for a in args) + tuple(sorted(kw.items()))
    if key not in _CASES:
        _CASES[key] = Case(ti, *args, **kw)
    return _CASES[key]


def check_rows(label, c, got, ref):
    """got, ref [rows][heads][hd]: the indicator bound, or rtol = atol = 4e-3 for random values."""
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got)), f"{label}: non-finite output at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    err = np.abs(got - ref)
    if c.values == "indicator":
        over = err / A.indicator_bound(ref)
        note(f"{label} {c.kind}", over.max())
        i = np.unravel_index(int(over.argmax()), over.shape)
        assert over.max() <= 1.0, (f"{label} {c.kind}: err / bound {over.max():.3g} at (row, head, d) {i}: "
                                   f"got {got[i]!r}, ref {ref[i]!r}")
    else:
        over = err / (A.ATOL + A.RTOL * np.abs(ref))
        note(f"{label} random/4e-3", over.max())
        assert over.max() <= 1.0, f"{label}: random values off by {over.max():.3g} x (4e-3 + 4e-3 |ref|)"


def run_decode(ti, c, splits, M=None, packed=False, ws=None, row0=0):
    """One ti_attn_decode / ti_attn_decode_packed launch over rows [row0, row0 + M) of the case, checked
    against the reference; -> the raw output bytes (packed runs: for the padding rows)."""
    L = ti.lib()
    M = c.M - row0 if M is None else M
    heads, hd, qd = c.heads, c.hd, c.heads * c.hd
    Mp = (M + 15) // 16 * 16 if packed else M
    out = guarded(ti, Mp * qd * 2)
    own_ws = ws is None
    if own_ws:
        ws_bytes = L.ti_attn_workspace_bytes(M, heads, hd, splits)
        ws = guarded(ti, ws_bytes)
        fill(ti, ws, 0, ws_bytes, 0)       # arrival tickets start at zero
    fn = L.ti_attn_decode_packed if packed else L.ti_attn_decode
    ti.check(fn(c.qd.ptr + row0 * qd * 4, c.kd.ptr + row0 * c.stride * 2, c.vd.ptr + row0 * c.stride * 2, c.stride,
                c.max_seq, c.pd.ptr + row0 * 4, M, heads, c.kvh, hd, splits, ws.ptr, out.ptr, None))
    ti.sync()
    raw = fetch(ti, out, 0, Mp * qd * 2 + GUARD)
    assert np.all(raw[Mp * qd * 2:] == PAT), "written behind out"
    if own_ws:
        guard_intact(ti, ws, ws.nbytes - GUARD, "the workspace")
    flat = raw[:Mp * qd * 2].view(f16)
    got = ti.unpack_rows(flat, M, qd) if packed else flat.reshape(M, qd)
    label = instance(M, c.G, hd, c.max_seq, splits) + (" packed" if packed else "")
    check_rows(label, c, got.astype(f64).reshape(M, heads, hd), c.row[row0:row0 + M])
    return raw[:Mp * qd * 2]


def run_partials(ti, c, splits, M=None, row0=0):
    """One ti_attn_decode_partials launch: well-formed splits, then the host merge against the row and
    the logsumexp of the reference."""
    L = ti.lib()
    M = c.M - row0 if M is None else M
    heads, hd, qd = c.heads, c.hd, c.heads * c.hd
    po_bytes, pml_bytes = M * heads * splits * hd * 2, M * heads * splits * 2 * 4
    po, pml = guarded(ti, po_bytes), guarded(ti, pml_bytes)
    ti.check(L.ti_attn_decode_partials(c.qd.ptr + row0 * qd * 4, c.kd.ptr + row0 * c.stride * 2,
                                       c.vd.ptr + row0 * c.stride * 2, c.stride, c.max_seq, c.pd.ptr + row0 * 4, M,
                                       heads, c.kvh, hd, splits, po.ptr, pml.ptr, None))
    ti.sync()
    guard_intact(ti, po, po_bytes, "part_o")
    guard_intact(ti, pml, pml_bytes, "part_ml")
    part_o = fetch(ti, po, 0, po_bytes).view(f16).reshape(M * heads, splits, hd)
    part_ml = fetch(ti, pml, 0, pml_bytes).view(f32).reshape(M * heads, splits, 2)
    A.check_partials(part_o, part_ml)
    row, lse = A.merge_partials(part_o, part_ml)
    label = instance(M, c.G, hd, c.max_seq, splits, partials=True) + " partials"
    check_rows(label, c, row.reshape(M, heads, hd), c.row[row0:row0 + M])
    d = np.abs(lse.reshape(M, heads) - c.lse[row0:row0 + M])
    note("logsumexp (all partials cases)", d.max())
    if c.kind == "flat":
        short = c.pos[row0:row0 + M] < 64
        if short.any():
            note("logsumexp (flat, L <= 64)", d[short].max())
    assert d.max() <= LSE_TOL, f"{label}: logsumexp off by {d.max():.3g} at (row, head) {np.argwhere(d > LSE_TOL)[:4].tolist()}"


# ------------------------------------------------------------------ the variants with M > 1
GROUPS = [(G, hd) for hd in (64, 128) for G in (1, 2, 4, 8)]
KVH = 2                 # kv-heads of the sweeps: 288 streams x 2 x 320 x 128 fp16 = 47 MB per cache
M_SWEEP, SEQ_SWEEP = 288, 320
M_KINDS = 96
POS_KINDS = (3 * np.arange(M_KINDS) + np.arange(M_KINDS) % 3).astype(np.int32)     # lengths 1 .. 288, every residue


def gid(p):
    return "G%d-hd%d" % p


@pytest.mark.parametrize("splits", [1, 3, 8, 64])
@pytest.mark.parametrize("G,hd", GROUPS, ids=[gid(p) for p in GROUPS])
def test_length_sweep(ti, G, hd, splits):
    """288 streams with pos = 0 .. 287 in one launch: every length through two rounds of the deepest ring
    (8 waves x 8 keys x ring 2; head-parallel 8 x ring 8 = 64 keys a round), the tail slot, the tail pass
    and L < KPW.  splits = 64 runs the first 96 streams (workspace size): L < 64 leaves splits empty, and
    G >= 4 crosses the clamp at attn_max_splits."""
    c = case(ti, "flat", "indicator", M_SWEEP, KVH * G, KVH, hd, SEQ_SWEEP, np.arange(M_SWEEP, dtype=np.int32))
    run_decode(ti, c, splits, M=96 if splits == 64 else None)


@pytest.mark.parametrize("kind,values", [("steep", "indicator"), ("ramp", "indicator"), ("flat", "random")])
@pytest.mark.parametrize("G,hd", GROUPS, ids=[gid(p) for p in GROUPS])
def test_kinds(ti, G, hd, kind, values):
    """A moving maximum (`steep`), a rescale at every key (`ramp`) and cancelling values (`random`):
    96 streams of lengths 1 .. 288, merged splits."""
    c = case(ti, kind, values, M_KINDS, KVH * G, KVH, hd, SEQ_SWEEP, POS_KINDS, seed=1)
    run_decode(ti, c, 3)


# lengths around the slots, passes (32 / 64 keys) and ring rounds (128 / 256 keys) of the ring-4 instances,
# through two rounds, and the last rows of the cache
LONG_L = sorted(set(list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161,
                                          191, 192, 193, 255, 256, 257, 287, 288, 289, 383, 384, 385, 511, 512, 513,
                                          575, 576, 577, 767, 768, 769, 1023, 1024]))
LONG_GROUPS = [(G, hd) for hd in (64, 128) for G in (4, 8)]


@pytest.mark.parametrize("G,hd", LONG_GROUPS, ids=[gid(p) for p in LONG_GROUPS])
def test_long_range_sweep(ti, G, hd):
    """max_seq = 1024, splits = 1: the ring-4 instance at any length (the dispatch looks at max_seq, not at
    L).  50 streams (27 MB per cache at hd 128).  The same buffers with splits 3, 8 and 64 run the ring-2 /
    head-parallel instances at max_seq 1024."""
    pos = np.array(LONG_L, np.int32) - 1
    c = case(ti, "flat", "indicator", len(pos), KVH * G, KVH, hd, 1024, pos, seed=2)
    assert instance(c.M, G, hd, 1024, 1).startswith("ring4long")
    for splits in (1, 3, 8, 64):
        run_decode(ti, c, splits)


@pytest.mark.parametrize("kind,values", [("steep", "indicator"), ("ramp", "indicator"), ("flat", "random")])
@pytest.mark.parametrize("G,hd", LONG_GROUPS, ids=[gid(p) for p in LONG_GROUPS])
def test_long_range_kinds(ti, G, hd, kind, values):
    pos = np.array([0, 5, 31, 64, 100, 127, 128, 200, 255, 256, 300, 511, 700, 1023], np.int32)
    c = case(ti, kind, values, len(pos), KVH * G, KVH, hd, 1024, pos, seed=3)
    run_decode(ti, c, 1)


@pytest.mark.parametrize("G,hd", LONG_GROUPS, ids=[gid(p) for p in LONG_GROUPS])
def test_long_contexts_long_range(ti, G, hd):
    """L = 1500 and 2048 at max_seq 2048: written directly (splits 1) and merged (splits 2, still 1024 keys
    per split), and as partials; sixteen (hd 128) or thirty-two keys per output element."""
    c = case(ti, "flat", "indicator", 2, KVH * G, KVH, hd, 2048, np.array([1499, 2047], np.int32), seed=4)
    for splits in (1, 2):
        assert instance(2, G, hd, 2048, splits).startswith("ring4long")
        run_decode(ti, c, splits)
    run_partials(ti, c, 2)


@pytest.mark.parametrize("L", [1500, 2048])
def test_long_context_7b(ti, L):
    """The 7B decode step: heads = kv_heads = 32, hd 128, one stream, partials with 8 splits."""
    c = case(ti, "flat", "indicator", 1, 32, 32, 128, 2048, np.array([L - 1], np.int32), seed=5)
    run_partials(ti, c, 8)
    run_decode(ti, c, 8)


# ------------------------------------------------------------------ the variants with M = 1
class Walk:
    """One stream's cache, uploaded once; launches at decreasing lengths, with NaN (0xFFFF) written
    behind each limit before its launch.  Row i of q / pos / the reference belongs to length ls[i]."""

    def __init__(self, ti, kind, values, heads, kvh, hd, max_seq, seed):
        self.ls = sorted(A.SWEEP_L, reverse=True)
        n, pos = len(self.ls), np.array(self.ls, np.int32) - 1
        c = Case(ti, kind, values, n, heads, kvh, hd, max_seq, pos, seed, shared=True, poisoned=False)
        self.c, self.limit = c, max_seq

    def lower(self, L):
        """NaN in rows [L, previous limit) of every kv-head."""
        c = self.c
        if L < self.limit:
            for i in range(c.kvh):
                for buf in (c.kd, c.vd):
                    fill(c.ti, buf, (i * c.max_seq + L) * c.hd * 2, (self.limit - L) * c.hd * 2, 0xFF)
            self.limit = L


@pytest.mark.parametrize("kind", ["flat", "steep", "ramp"])
@pytest.mark.parametrize("hd", [64, 128])
def test_m1_sweep_mha(ti, hd, kind):
    """One stream, MHA: the ring-3 instance, as a merged launch (splits 1, 4, 64) and as partials."""
    w = Walk(ti, kind, "indicator", 4, 4, hd, SEQ_SWEEP, seed=6)
    assert instance(1, 1, hd, SEQ_SWEEP, 4) == f"ring3 hd{hd} G1"
    for i, L in enumerate(w.ls):
        w.lower(L)
        for splits in (1, 4, 64) if kind == "flat" else (4,):
            run_decode(ti, w.c, splits, M=1, row0=i)
        for splits in (2, 8) if kind == "flat" else (3,):
            run_partials(ti, w.c, splits, M=1, row0=i)


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("hd", [64, 128])
def test_m1_sweep_expanded_partials(ti, hd, G):
    """One stream, GQA, partials: run head by head (kv_shift) on the ring-3 instance."""
    w = Walk(ti, "flat", "indicator", 2 * G, 2, hd, SEQ_SWEEP, seed=7)
    assert instance(1, G, hd, SEQ_SWEEP, 4, partials=True) == f"ring3 hd{hd} G1 expand{G}"
    for i, L in enumerate(w.ls):
        w.lower(L)
        for splits in (2, 5, 8):
            run_partials(ti, w.c, splits, M=1, row0=i)


def test_m1_random_values(ti):
    for heads, kvh, hd in ((4, 4, 128), (4, 4, 64), (8, 2, 64), (16, 2, 128)):
        c = case(ti, "flat", "random", 1, heads, kvh, hd, SEQ_SWEEP, np.array([299], np.int32), seed=8)
        run_decode(ti, c, 4)
        run_partials(ti, c, 4)


# ------------------------------------------------------------------ partials with M > 1, packed output
@pytest.mark.parametrize("kind,values", [("flat", "indicator"), ("steep", "indicator"), ("ramp", "indicator"),
                                         ("flat", "random")])
@pytest.mark.parametrize("G,hd", GROUPS, ids=[gid(p) for p in GROUPS])
def test_partials_m5(ti, G, hd, kind, values):
    """Five streams: part_o / part_ml written by the grouped kernels (head-parallel included)."""
    c = case(ti, kind, values, 5, KVH * G, KVH, hd, SEQ_SWEEP, np.array([0, 6, 63, 200, 319], np.int32), seed=9)
    for splits in (2, 3, 8) if kind == "flat" else (3,):
        run_partials(ti, c, splits)


@pytest.mark.parametrize("heads,kvh,hd", [(8, 2, 128), (4, 2, 64)], ids=["hp-hd128", "ring2-hd64"])
@pytest.mark.parametrize("M", [17, 45, 64])
def test_packed_output(ti, M, heads, kvh, hd):
    """TI_X_F16_PACKED order at M = 17, 45, 64, unpacked with ti.unpack_rows; the padding rows
    M .. 16 ceil(M / 16) are reported (module docstring), not required either way."""
    pos = np.random.default_rng(M).integers(0, SEQ_SWEEP, M).astype(np.int32)
    c = case(ti, "flat", "indicator", M, heads, kvh, hd, SEQ_SWEEP, pos, seed=10)
    for splits in (1, 4):
        raw = run_decode(ti, c, splits, packed=True)
        Mp, K = (M + 15) // 16 * 16, heads * hd
        if Mp > M:
            mm, kk = np.meshgrid(np.arange(M, Mp), np.arange(K), indexing="ij")
            pad_rows = raw.view(np.uint16)[ti.packed_index(mm, kk, K)]
            note("packed: padding rows written (1 = yes)", float(np.any(pad_rows != PAT * 0x0101)))


# ------------------------------------------------------------------ strides, memory, workspace reuse
@pytest.mark.parametrize("hd", [64, 128])
def test_padded_stream_stride(ti, hd):
    """kv_stream_stride larger than one stream's cache; the gap between streams holds NaN."""
    pos = np.array([0, 3, 40, 64, 129, 255, 319], np.int32)
    c = case(ti, "flat", "indicator", 7, 4, 2, hd, SEQ_SWEEP, pos, seed=11, pad=520)
    assert c.stride == 2 * SEQ_SWEEP * hd + 520
    for splits in (1, 4):
        run_decode(ti, c, splits)
    run_partials(ti, c, 4)


def test_stride_zero_unordered_positions(ti):
    """Stride 0: the rows are tokens of one stream, each with its own limit, in any order."""
    pos = np.array([200, 3, 77, 0, 310, 64, 63, 150, 9], np.int32)
    for heads, kvh, hd in ((4, 4, 128), (8, 2, 64)):
        c = case(ti, "flat", "indicator", 9, heads, kvh, hd, SEQ_SWEEP, pos, seed=12, shared=True)
        for splits in (1, 4):
            run_decode(ti, c, splits)
        run_partials(ti, c, 4)


@pytest.mark.parametrize("entry", ["decode", "packed", "partials"])
def test_memory_discipline(ti, entry):
    """K and V bit-identical after the launch (the pattern behind out, part_o, part_ml and the workspace
    is checked after every launch of this module)."""
    pos = np.array([0, 17, 100, 255, 319], np.int32)
    c = case(ti, "flat", "indicator", 5, 8, 2, 128, SEQ_SWEEP, pos, seed=13, keep=True)
    if entry == "partials":
        run_partials(ti, c, 4)
    else:
        run_decode(ti, c, 4, packed=entry == "packed")
    c.kv_unchanged()


def test_workspace_reuse(ti):
    """One workspace sized for the largest call and zeroed once; calls of different M, splits and heads
    follow each other on it (the ticket region is re-armed by every call, the partials are not cleared)."""
    L = ti.lib()
    calls = [(3, 4, 8, 2, 128), (1, 16, 4, 4, 128), (5, 2, 16, 2, 64), (3, 4, 8, 2, 128)]     # (M, splits, heads, kvh, hd)
    ws_bytes = max(L.ti_attn_workspace_bytes(M, heads, hd, splits) for M, splits, heads, kvh, hd in calls)
    ws = guarded(ti, ws_bytes)
    fill(ti, ws, 0, ws_bytes, 0)
    for n, (M, splits, heads, kvh, hd) in enumerate(calls):
        pos = np.array([319, 64, 7, 200, 31][:M], np.int32)
        c = case(ti, "flat", "indicator", M, heads, kvh, hd, SEQ_SWEEP, pos, seed=14 + n)
        run_decode(ti, c, splits, ws=ws)
        guard_intact(ti, ws, ws_bytes, "the workspace")
