"""ti_attn_decode_f8, ti_attn_decode_packed_f8 and ti_attn_decode_partials_f8 (the KV8 instances of
attn_split_kernel: attention.hip, attention_body.hpp) against the float64 reference of tests/attn_ref.py
over the very e4m3 bytes that are uploaded.

Inputs are attn_ref.make_inputs with K and V quantised by kv8_ref.quantize (`indicator` values are exact in
e4m3); the reference is attn_ref.attend over kv8_ref.decode(bytes).  The kernels widen every byte exactly
(v_cvt_pk_f32_fp8) and then run the fp16 kernels' own softmax and merges, so the error sources of
attn_ref.indicator_bound are unchanged and the bounds are those of test_gpu_attn_oracle.py: the derived
indicator bound, rtol = atol = 4e-3 for `random` values, LSE_TOL = 2.7e-5 for the partials' logsumexp.
test_kv8_ref.py shows on the reference side that bytes read with the wrong exponent bias leave the bound
by more than 10 times.

Instances (the dispatch is the fp16 one, attention.hip launch_attn; `instance()` of test_gpu_attn_oracle.py
gives the labels) and the cases that reach them:
  ring 2   <hd, 1 | 2, 2>, <64, 4, 2>, <128, 8, 2>      M = 5 groups (splits 1, 3, 8, 64; partials), packed hd 64,
                                                        stride 0
  ring 3   <hd, 1, 3>  M = 1 MHA, and with kv_shift     M = 1 sweeps over attn_ref.SWEEP_L (decode, partials,
                                                        partials with GQA expansion)
  ring 8   <128, 4, 8, HP>, <64, 8, 8, HP>              M = 5 groups, packed hd 128, stride 0 (G 4 at hd 64 is ring 2)
  ring 4   <hd, 4 | 8, 4>  max_seq / splits >= 1024     max_seq 1024 with splits 1, max_seq 2048 with splits 2
           <128, 4, 4> holds 16 dims per lane (16-byte loads) by default; the 8-dim instance behind
           TI_ATTN_KV8_LOAD16=0 runs the same cases in a child process (test_long_range_8_byte_loads)
  outputs  direct (splits 1), merged by the last arriver (empty splits and the attn_max_splits clamp at
           splits 64), partials, packed order at M = 17 and 45.
Guards: rows behind every limit hold 0x7F (e4m3 NaN); 0xA5 behind out, part_o, part_ml and the workspace,
checked after every launch; K / V bytes compared after a launch per entry point.

Measured on an MI355X over every case of this module (printed at module teardown, `pytest -s`), worst
err / bound of the `indicator` cases | worst |got - ref| / (4e-3 + 4e-3 |ref|) of the `random` cases:
  ring 2 0.495 | 0.038, ring 3 (expansion included) 0.494 | 0.013, ring 8 head-parallel 0.494 | 0.032,
  ring 4 long-range 0.491 | 0.056 (16 and 8 dims per lane alike); logsumexp of the partials: worst 8.8e-6.
As for the fp16 kernels the fp16 store of the output is 0.5 of the bound; no instance needed a further term.
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import attn_ref as A
import kv8_ref as Q
import test_gpu_attn_oracle as O          # device plumbing and the dispatch mirror (imported, not edited)

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64
GUARD, PAT = O.GUARD, O.PAT
LSE_TOL = 2.7e-5        # test_gpu_attn_oracle.py's (4 x its measured worst); the merge code is shared
NAN8 = Q.NAN_BYTE
SEQ = 320

WORST: dict = {}
_CASES: dict = {}


def note(label, value):
    WORST[label] = max(WORST.get(label, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    _CASES.clear()
    print("\nkv8 attention, worst per instance:")
    for k in sorted(WORST):
        print(f"  {k:52s} {WORST[k]:.3e}")


class Case:
    """Seeded inputs quantised to e4m3 on the device (0x7F behind every limit), the float64 reference over
    the decoded bytes."""

    def __init__(self, ti, kind, values, M, heads, kvh, hd, max_seq, pos, seed=0, shared=False, keep=False,
                 poisoned=True):
        self.ti, self.kind, self.values = ti, kind, values
        self.M, self.heads, self.kvh, self.hd, self.max_seq = M, heads, kvh, hd, max_seq
        self.G = heads // kvh
        self.pos = np.asarray(pos, np.int32)
        assert self.pos.shape == (M,) and self.pos.min() >= 0 and self.pos.max() < max_seq
        q, kc, vc = A.make_inputs(kind, values, M, heads, kvh, hd, max_seq, self.pos, seed, shared=shared)
        kb, vb = Q.quantize(kc), Q.quantize(vc)
        del kc, vc
        self.row, self.lse = A.attend(q, Q.decode(kb), Q.decode(vb), self.pos, heads)
        if poisoned:
            if shared:
                kb[:, :, int(self.pos.max()) + 1:] = NAN8
                vb[:, :, int(self.pos.max()) + 1:] = NAN8
            else:
                for m in range(M):
                    kb[m, :, int(self.pos[m]) + 1:] = NAN8
                    vb[m, :, int(self.pos[m]) + 1:] = NAN8
        self.stride = 0 if shared else kvh * max_seq * hd
        self.kd, self.vd, self.qd, self.pd = O.dev(ti, kb), O.dev(ti, vb), O.dev(ti, q), O.dev(ti, self.pos)
        self.k_bits, self.v_bits = (kb.copy(), vb.copy()) if keep else (None, None)

    def kv_unchanged(self):
        for name, buf, bits in (("K", self.kd, self.k_bits), ("V", self.vd, self.v_bits)):
            assert np.array_equal(O.fetch(self.ti, buf, 0, bits.nbytes), bits.reshape(-1)), f"{name} changed by the launch"


def case(ti, *args, **kw):
    key = tuple(a.tobytes() if isinstance(a, np.ndarray) else a for a in args) + tuple(sorted(kw.items()))
    if key not in _CASES:
        _CASES[key] = Case(ti, *args, **kw)
    return _CASES[key]


def check_rows(label, c, got, ref):
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


def run_decode(ti, c, splits, M=None, packed=False, row0=0):
    """One ti_attn_decode_f8 / _packed_f8 launch over rows [row0, row0 + M) of the case (one byte per cache
    element: the stream offset is row0 * stride bytes)."""
    L = ti.lib()
    M = c.M - row0 if M is None else M
    heads, hd, qd = c.heads, c.hd, c.heads * c.hd
    Mp = (M + 15) // 16 * 16 if packed else M
    out = O.guarded(ti, Mp * qd * 2)
    ws_bytes = L.ti_attn_workspace_bytes(M, heads, hd, splits)
    ws = O.guarded(ti, ws_bytes)
    O.fill(ti, ws, 0, ws_bytes, 0)
    fn = L.ti_attn_decode_packed_f8 if packed else L.ti_attn_decode_f8
    ti.check(fn(c.qd.ptr + row0 * qd * 4, c.kd.ptr + row0 * c.stride, c.vd.ptr + row0 * c.stride, c.stride,
                c.max_seq, c.pd.ptr + row0 * 4, M, heads, c.kvh, hd, splits, ws.ptr, out.ptr, None))
    ti.sync()
    raw = O.fetch(ti, out, 0, Mp * qd * 2 + GUARD)
    assert np.all(raw[Mp * qd * 2:] == PAT), "written behind out"
    O.guard_intact(ti, ws, ws_bytes, "the workspace")
    flat = raw[:Mp * qd * 2].view(f16)
    got = ti.unpack_rows(flat, M, qd) if packed else flat.reshape(M, qd)
    label = O.instance(M, c.G, hd, c.max_seq, splits) + (" packed" if packed else "")
    check_rows(label, c, got.astype(f64).reshape(M, heads, hd), c.row[row0:row0 + M])
    out.free()
    ws.free()
    return label


def run_partials(ti, c, splits, M=None, row0=0):
    L = ti.lib()
    M = c.M - row0 if M is None else M
    heads, hd, qd = c.heads, c.hd, c.heads * c.hd
    po_bytes, pml_bytes = M * heads * splits * hd * 2, M * heads * splits * 2 * 4
    po, pml = O.guarded(ti, po_bytes), O.guarded(ti, pml_bytes)
    ti.check(L.ti_attn_decode_partials_f8(c.qd.ptr + row0 * qd * 4, c.kd.ptr + row0 * c.stride,
                                          c.vd.ptr + row0 * c.stride, c.stride, c.max_seq, c.pd.ptr + row0 * 4, M,
                                          heads, c.kvh, hd, splits, po.ptr, pml.ptr, None))
    ti.sync()
    O.guard_intact(ti, po, po_bytes, "part_o")
    O.guard_intact(ti, pml, pml_bytes, "part_ml")
    part_o = O.fetch(ti, po, 0, po_bytes).view(f16).reshape(M * heads, splits, hd)
    part_ml = O.fetch(ti, pml, 0, pml_bytes).view(f32).reshape(M * heads, splits, 2)
    A.check_partials(part_o, part_ml)
    row, lse = A.merge_partials(part_o, part_ml)
    label = O.instance(M, c.G, hd, c.max_seq, splits, partials=True) + " partials"
    check_rows(label, c, row.reshape(M, heads, hd), c.row[row0:row0 + M])
    d = np.abs(lse.reshape(M, heads) - c.lse[row0:row0 + M])
    note("logsumexp (all partials cases)", d.max())
    assert d.max() <= LSE_TOL, f"{label}: logsumexp off by {d.max():.3g}"
    po.free()
    pml.free()
    return label


# ------------------------------------------------------------------ M = 5: every group, every output path
GROUPS = [(G, hd) for hd in (64, 128) for G in (1, 2, 4, 8)]
KVH = 2
POS5 = np.array([0, 62, 63, 64, 256], np.int32)           # L = 1, 63, 64, 65, 257


def gid(p):
    return "G%d-hd%d" % p


@pytest.mark.parametrize("splits", [1, 3, 8, 64])
@pytest.mark.parametrize("G,hd", GROUPS, ids=[gid(p) for p in GROUPS])
def test_m5_groups(ti, G, hd, splits):
    """Five streams of L = 1, 63, 64, 65, 257: direct output, merged splits, empty splits (64 over L < 64)
    and the attn_max_splits clamp (G >= 4 at 64)."""
    c = case(ti, "flat", "indicator", 5, KVH * G, KVH, hd, SEQ, POS5)
    label = run_decode(ti, c, splits)
    hp = G >= 4 and hd // (64 // G) == 8
    assert label.startswith("ring8hp" if hp else "ring2")


@pytest.mark.parametrize("kind,values", [("flat", "indicator"), ("steep", "indicator"), ("ramp", "indicator"),
                                         ("flat", "random")])
@pytest.mark.parametrize("G,hd", GROUPS, ids=[gid(p) for p in GROUPS])
def test_m5_kinds_and_partials(ti, G, hd, kind, values):
    """A moving maximum, a rescale at every key and cancelling values; merged (3 splits) and as partials."""
    c = case(ti, kind, values, 5, KVH * G, KVH, hd, SEQ, POS5, seed=1 if kind != "flat" or values == "random" else 0)
    if not (kind == "flat" and values == "indicator"):
        run_decode(ti, c, 3)
    for splits in (2, 3, 8) if kind == "flat" else (3,):
        run_partials(ti, c, splits)


# ------------------------------------------------------------------ M = 1 over SWEEP_L
class Walk:
    """One stream's cache, uploaded once; launches at decreasing lengths, 0x7F written behind each limit
    before its launch.  Row i of q / pos / the reference belongs to length ls[i]."""

    def __init__(self, ti, kind, values, heads, kvh, hd, max_seq, seed):
        self.ls = sorted(A.SWEEP_L, reverse=True)
        pos = np.array(self.ls, np.int32) - 1
        self.c = Case(ti, kind, values, len(self.ls), heads, kvh, hd, max_seq, pos, seed, shared=True, poisoned=False)
        self.limit = max_seq

    def lower(self, L):
        c = self.c
        if L < self.limit:
            for i in range(c.kvh):
                for buf in (c.kd, c.vd):
                    O.fill(c.ti, buf, (i * c.max_seq + L) * c.hd, (self.limit - L) * c.hd, NAN8)
            self.limit = L


@pytest.mark.parametrize("hd", [64, 128])
def test_m1_sweep_mha(ti, hd):
    """One stream, MHA: the ring-3 instance, merged (splits 1, 4, 64) and as partials (2, 8)."""
    w = Walk(ti, "flat", "indicator", 4, 4, hd, SEQ, seed=6)
    for i, L in enumerate(w.ls):
        w.lower(L)
        for splits in (1, 4, 64):
            assert run_decode(ti, w.c, splits, M=1, row0=i) == f"ring3 hd{hd} G1"
        for splits in (2, 8):
            run_partials(ti, w.c, splits, M=1, row0=i)


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("hd", [64, 128])
def test_m1_sweep_expanded_partials(ti, hd, G):
    """One stream, GQA, partials: run head by head (kv_shift) on the ring-3 instance."""
    w = Walk(ti, "flat", "indicator", 2 * G, 2, hd, SEQ, seed=7)
    for i, L in enumerate(w.ls):
        w.lower(L)
        for splits in (2, 5, 8):
            assert run_partials(ti, w.c, splits, M=1, row0=i) == f"ring3 hd{hd} G1 expand{G} partials"


def test_m1_random_values(ti):
    for heads, kvh, hd in ((4, 4, 128), (4, 4, 64), (8, 2, 64), (16, 2, 128)):
        c = case(ti, "flat", "random", 1, heads, kvh, hd, SEQ, np.array([299], np.int32), seed=8)
        run_decode(ti, c, 4)
        run_partials(ti, c, 4)


# ------------------------------------------------------------------ long range (ring 4)
LONG_GROUPS = [(G, hd) for hd in (64, 128) for G in (4, 8)]


@pytest.mark.parametrize("G,hd", LONG_GROUPS, ids=[gid(p) for p in LONG_GROUPS])
def test_long_range(ti, G, hd):
    """max_seq 1024 with splits 1 (lengths around the slots, passes and ring rounds, and the last row), and
    max_seq 2048 with splits 2 (merged and as partials): the ring-4 instances."""
    pos = np.array([1, 4, 9, 31, 32, 33, 64, 127, 128, 129, 257, 384, 513, 769, 1023, 1024], np.int32) - 1
    c = case(ti, "flat", "indicator", len(pos), KVH * G, KVH, hd, 1024, pos, seed=2)
    assert run_decode(ti, c, 1).startswith("ring4long")
    cr = case(ti, "flat", "random", 3, KVH * G, KVH, hd, 1024, np.array([5, 300, 1023], np.int32), seed=3)
    assert run_decode(ti, cr, 1).startswith("ring4long")
    c2 = case(ti, "flat", "indicator", 2, KVH * G, KVH, hd, 2048, np.array([1499, 2047], np.int32), seed=4)
    assert run_decode(ti, c2, 2).startswith("ring4long")
    assert run_partials(ti, c2, 2).startswith("ring4long")


def test_long_range_8_byte_loads():
    """The knob itself: TI_ATTN_KV8_LOAD16 is read once per process, so the 8-dims-per-lane ring-4 instance
    at hd 128 G 4 runs test_long_range in a child process with the knob off."""
    env = dict(os.environ, TI_ATTN_KV8_LOAD16="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        os.path.abspath(__file__) + "::test_long_range"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "4 passed" in r.stdout


# ------------------------------------------------------------------ packed output, stride 0
@pytest.mark.parametrize("heads,kvh,hd", [(8, 2, 128), (4, 2, 64)], ids=["hp-hd128", "ring2-hd64"])
@pytest.mark.parametrize("M", [17, 45])
def test_packed_output(ti, M, heads, kvh, hd):
    pos = np.random.default_rng(M).integers(0, SEQ, M).astype(np.int32)
    c = case(ti, "flat", "indicator", M, heads, kvh, hd, SEQ, pos, seed=10)
    for splits in (1, 4):
        run_decode(ti, c, splits, packed=True)


@pytest.mark.parametrize("heads,kvh,hd", [(4, 4, 128), (8, 2, 64), (8, 2, 128)])
def test_stride_zero_shared_cache(ti, heads, kvh, hd):
    """Stride 0: 17 rows are consecutive tokens (positions 40 .. 56) of one stream, each with its own limit
    in the shared cache -- a prompt chunk of a KV8 engine (row-major and packed)."""
    pos = np.arange(40, 57, dtype=np.int32)
    c = case(ti, "flat", "indicator", 17, heads, kvh, hd, SEQ, pos, seed=12, shared=True)
    assert c.stride == 0
    for splits in (1, 4):
        run_decode(ti, c, splits)
        run_decode(ti, c, splits, packed=True)
    run_partials(ti, c, 4)


@pytest.mark.parametrize("entry", ["decode", "packed", "partials"])
def test_memory_discipline(ti, entry):
    """K and V bytes identical after the launch."""
    pos = np.array([0, 17, 100, 255, 319], np.int32)
    c = case(ti, "flat", "indicator", 5, 8, 2, 128, SEQ, pos, seed=13, keep=True)
    if entry == "partials":
        run_partials(ti, c, 4)
    else:
        run_decode(ti, c, 4, packed=entry == "packed")
    c.kv_unchanged()
