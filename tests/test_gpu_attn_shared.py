"""ti_attn_decode_shared (shared_attn.hip) against the float64 reference of tests/attn_ref.py: stream m attends keys
[0, P) of stream 0's cache and keys [P, pos[m]] of its own, in two dependent launches (prefix partials on MFMA per
16 (stream, q-head) columns and split; own keys and the merge per (stream, kv-head)).

Inputs are attn_ref.make_inputs' (a cache per stream) with rows [0, P) of every stream replaced by stream 0's; the
reference is attn_ref.attend on those.  In the uploaded caches rows [0, P) of streams >= 1 hold NaN (never read)
and so do the rows past pos[m].  Every case runs, at kv_heads 2 and max_seq 512,
  hd in {64, 128} x G in {1, 4, 8} x M in {1, 2, 5, 16, 17, 64} (packed too at M 17 and 64) x splits in {1, 3, 32}
  x kinds flat / steep / ramp `indicator` and flat `random` x P in {1, 15, 16, 17, 33, 300},
with own lengths pos[m] - P + 1 cycling over {0, 1, 2, 15, 16, 17, 63, 64, 65, 150} across the streams: stream 0
(and every tenth) is prefix-only -- half of those pass a position below P - 1, which counts as P - 1 -- and the
columns of one 16-column block end in different key blocks.  One long case: P = 2040 of max_seq 2064, M = 5.
Bars (the project's own): `indicator` err / attn_ref.indicator_bound <= 1; `random` within ATOL + RTOL |ref|; every
output finite; the 0xA5 pattern behind `out` and behind the workspace intact (the workspace is handed over
holding that pattern, never zeroed); K and V bit-identical after the launch; a second launch gives the same bits;
and the result lies within the same bars of ti_attn_decode's on the same inputs with finite prefix copies.

Measured on an MI355X over every case of this module (printed at module teardown, `pytest -s`), worst
err / bound of the `indicator` cases over the three kinds | worst |got - ref| / (4e-3 + 4e-3 |ref|) of `random`:
  hd 64   G 1 0.494 | 0.076   G 4 0.494 | 0.076   G 8 0.495 | 0.076   (G 2, steep only: 0.444)
  hd 128  G 1 0.493 | 0.075   G 4 0.493 | 0.076   G 8 0.497 | 0.081   (G 2, steep only: 0.469)
The fp16 store alone is 0.5 of the bound (ti_attn_prefill_split sits at 0.490-0.497, test_gpu_attn_prefill_split.py):
the fp32 partials, the own keys' fp32 FMA and the merge add nothing that shows beside it.
"""
from __future__ import annotations

import numpy as np
import pytest

import attn_ref as A
from test_gpu_attn_oracle import GUARD, PAT, dev, fetch, fill, guarded

pytestmark = pytest.mark.gpu

f16, f64 = np.float16, np.float64
KVH = 2
MAX_SEQ = 512
SPLITS = (1, 3, 32)
KINDS = (("flat", "indicator"), ("steep", "indicator"), ("ramp", "indicator"), ("flat", "random"))
PREFIXES = (1, 15, 16, 17, 33, 300)
OWN = (0, 1, 2, 15, 16, 17, 63, 64, 65, 150)

WORST: dict = {}


def note(label, value):
    WORST[label] = max(WORST.get(label, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    print("\nattn oracle (decode, shared prefix), worst per instance:")
    for k in sorted(WORST):
        print(f"  {k:44s} {WORST[k]:.3e}")


class SCase:
    """Seeded inputs with a common prefix of P rows, on the device twice -- NaN wherever ti_attn_decode_shared must
    not read, and with finite prefix copies for ti_attn_decode -- and their float64 reference."""

    def __init__(self, ti, kind, values, M, heads, hd, max_seq, P, seed):
        self.ti, self.kind, self.values = ti, kind, values
        self.M, self.heads, self.kvh, self.hd, self.max_seq, self.P = M, heads, KVH, hd, max_seq, P
        own = np.array([OWN[m % len(OWN)] for m in range(M)])
        self.eff = (P - 1 + own).astype(np.int32)              # the last key each stream attends
        assert self.eff.max() < max_seq
        # what the launch is given: a prefix-only row may sit anywhere at or below P - 1
        given = self.eff.copy()
        for m in range(M):
            if own[m] == 0 and (m // len(OWN)) % 2 == 1:
                given[m] = max(0, P - 5)
        q, kc, vc = A.make_inputs(kind, values, M, heads, KVH, hd, max_seq, self.eff, seed)
        kc, vc = np.array(kc, f16), np.array(vc, f16)
        kc[1:, :, :P] = kc[0, :, :P]
        vc[1:, :, :P] = vc[0, :, :P]
        self.row, _ = A.attend(q, kc, vc, self.eff, heads)
        kp, vp = A.poison(kc, vc, self.eff)                    # finite prefix copies: ti_attn_decode's inputs
        self.stride = KVH * max_seq * hd
        self.qd = dev(ti, q)
        self.kd_plain, self.vd_plain, self.pd_plain = dev(ti, kp), dev(ti, vp), dev(ti, self.eff)
        kp[1:, :, :P] = np.nan
        vp[1:, :, :P] = np.nan
        self.kd, self.vd, self.pd = dev(ti, kp), dev(ti, vp), dev(ti, given)
        self.k_bits, self.v_bits = kp.view(np.uint16).reshape(-1).copy(), vp.view(np.uint16).reshape(-1).copy()


def within_bars(c, got, ref, what):
    err = np.abs(got - ref)
    if c.values == "indicator":
        over = err / A.indicator_bound(c.row)
    else:
        over = err / (A.ATOL + A.RTOL * np.abs(c.row))
    i = np.unravel_index(int(over.argmax()), over.shape)
    assert over.max() <= 1.0, (f"hd{c.hd} G{c.heads // KVH} M{c.M} P{c.P} {c.kind} {c.values} {what}: err / bound "
                               f"{over.max():.3g} at (row, head, d) {i}, last key {int(c.eff[i[0]])}: got {got[i]!r}, "
                               f"ref {ref[i]!r}")
    return float(over.max())


def launch(ti, c, splits, packed, ws, out):
    ti.check(ti.lib().ti_attn_decode_shared(c.qd.ptr, c.kd.ptr, c.vd.ptr, c.stride, c.max_seq, c.pd.ptr, c.M, c.heads,
                                            c.kvh, c.hd, c.P, splits, int(packed), ws.ptr, out.ptr, None))
    ti.sync()


def run_shared(ti, c, splits, packed=False):
    M, heads, hd, K = c.M, c.heads, c.hd, c.heads * c.hd
    Mp = (M + 15) // 16 * 16 if packed else M
    nbytes = Mp * K * 2
    ws_bytes = ti.lib().ti_attn_shared_workspace_bytes(M, heads, hd, splits)
    assert ws_bytes > 0
    out, ws = guarded(ti, nbytes), guarded(ti, ws_bytes)       # (the workspace starts as 0xA5 bytes, not zeros)
    launch(ti, c, splits, packed, ws, out)
    raw = fetch(ti, out, 0, nbytes + GUARD)
    assert np.all(raw[nbytes:] == PAT), "written behind out"
    assert np.all(fetch(ti, ws, ws_bytes, GUARD) == PAT), "written behind the workspace"
    for name, buf, bits in (("K", c.kd, c.k_bits), ("V", c.vd, c.v_bits)):
        assert np.array_equal(fetch(ti, buf, 0, bits.nbytes).view(np.uint16), bits), f"{name} changed by the launch"
    flat = raw[:nbytes].view(f16)
    got = (ti.unpack_rows(flat, M, K) if packed else flat.reshape(M, K)).astype(f64).reshape(M, heads, hd)
    what = f"splits {splits}" + (" packed" if packed else "")
    assert np.all(np.isfinite(got)), f"{what}: non-finite output at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    worst = within_bars(c, got, c.row, what + " vs float64")
    note(f"shared hd{hd} G{heads // KVH} {c.kind} {c.values}" + ("" if c.values == "indicator" else "/4e-3"), worst)
    # a second launch, the workspace as the first left it: the same bits
    out2 = guarded(ti, nbytes)
    launch(ti, c, splits, packed, ws, out2)
    assert np.array_equal(fetch(ti, out2, 0, nbytes), raw[:nbytes]), f"{what}: second launch differs"
    return got


def run_plain(ti, c):
    """ti_attn_decode over the caches with finite prefix copies."""
    L = ti.lib()
    nbytes = c.M * c.heads * c.hd * 2
    ws_bytes = L.ti_attn_workspace_bytes(c.M, c.heads, c.hd, 4)
    out, ws = guarded(ti, nbytes), ti.DeviceBuffer(ws_bytes)
    fill(ti, ws, 0, ws_bytes, 0)
    ti.check(L.ti_attn_decode(c.qd.ptr, c.kd_plain.ptr, c.vd_plain.ptr, c.stride, c.max_seq, c.pd_plain.ptr, c.M, c.heads,
                              c.kvh, c.hd, 4, ws.ptr, out.ptr, None))
    ti.sync()
    return fetch(ti, out, 0, nbytes).view(f16).astype(f64).reshape(c.M, c.heads, c.hd)


def run_case(ti, c):
    plain = run_plain(ti, c)
    for splits in SPLITS:
        got = run_shared(ti, c, splits)
        within_bars(c, got, plain, f"splits {splits} vs ti_attn_decode")
        if c.M in (17, 64) and splits != 3:
            got = run_shared(ti, c, splits, packed=True)
            within_bars(c, got, plain, f"splits {splits} packed vs ti_attn_decode")


@pytest.mark.parametrize("kind,values", KINDS, ids=[f"{k}-{v}" for k, v in KINDS])
@pytest.mark.parametrize("M", [1, 2, 5, 16, 17, 64])
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("hd", [64, 128])
def test_shared_matches_float64_and_decode(ti, hd, G, M, kind, values):
    for P in PREFIXES:
        run_case(ti, SCase(ti, kind, values, M, KVH * G, hd, MAX_SEQ, P, seed=P))


@pytest.mark.parametrize("hd,G", [(64, 1), (128, 4), (128, 8)])
def test_long_prefix(ti, hd, G):
    """P = 2040 of max_seq 2064: 128 prefix blocks dealt over the splits, several rounds of the ring per split."""
    for kind, values in (("flat", "indicator"), ("flat", "random")):
        run_case(ti, SCase(ti, kind, values, 5, KVH * G, hd, 2064, 2040, seed=3))


def test_two_kv_head_groups_of_two(ti):
    """G = 2, the group size the grid above leaves out."""
    for hd in (64, 128):
        run_case(ti, SCase(ti, "steep", "indicator", 17, KVH * 2, hd, MAX_SEQ, 33, seed=5))
