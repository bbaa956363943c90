"""ti_guide_step + ti_guide_reset (kernels/guide.hip) against the NumPy restatement (tests/guide_ref.py), bit for bit.

Every launch works on buffers of exactly the advertised size with a 0xA5 pattern behind them (the helpers of
tests/test_gpu_attn_oracle.py): the logits [M][ldl], the state row, and the guide's four buffers, which must come
back unchanged.  With ldl = V + 5 the rows start at every alignment modulo 16 bytes, so the scalar head, the 16-byte
groups (whose four mask bits then straddle two words) and the scalar tail all run; the pad columns hold a pattern
that must survive.  Rows hold -inf, both zeros, NaN and the largest finite values."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import guide_ref as R
from test_gpu_attn_oracle import dev, fetch, guard_intact, guarded

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
FMAX = np.finfo(f32).max
PLANTED = np.array([-np.inf, np.inf, 0.0, -0.0, FMAX, -FMAX, 1e-40, np.nan], f32)
PAD_BITS = 0x7FC12345                    # a NaN payload no arithmetic produces


def states_guide(V) -> R.Guide:
    """One automaton whose states are the mask shapes under test: only {0}, only {V - 1}, every 32nd id, all ids,
    all but one, the odd ids.  Every state moves to state (v mod n) on v."""
    rows = [[0], [V - 1], list(range(0, V, 32)), list(range(V))]
    if V > 1:
        rows += [[v for v in range(V) if v != V // 2], list(range(1, V, 2))]
    n = len(rows)
    return R.Guide([[(v, v % n) for v in r] for r in rows])


class DevGuide:
    def __init__(self, ti, g: R.Guide, V):
        self.host = dict(row_ptr=g.row_ptr, tokens=g.tokens, next=g.next, mask=g.bitmask(V))
        self.buf = {}
        for k, a in self.host.items():
            self.buf[k] = guarded(ti, a.nbytes)
            self.buf[k].upload(np.ascontiguousarray(a))
        self.ti = ti
        self.c = ti.GuideDev(g.n_states, (V + 31) // 32, self.buf["row_ptr"].ptr, self.buf["tokens"].ptr,
                             self.buf["next"].ptr, self.buf["mask"].ptr)

    def unchanged(self):
        for k, a in self.host.items():
            got = fetch(self.ti, self.buf[k], 0, a.nbytes)
            assert np.array_equal(got, np.ascontiguousarray(a).view(np.uint8).reshape(-1)), f"the guide's {k} changed"
            guard_intact(self.ti, self.buf[k], a.nbytes, f"the guide's {k}")


def rows_for(M, V, ldl, seed):
    r = np.random.RandomState(seed)
    lg = (r.standard_normal((M, ldl)) * 2.0).astype(f32)
    for m in range(M):
        at = r.choice(V, min(V, 2 * PLANTED.size), replace=False)
        lg[m, at] = np.resize(PLANTED, at.size)
    lg.view(np.uint32)[:, V:] = PAD_BITS
    return lg


def launch(ti, dg, lg, V, state, draw_stride=1, advance=1, step_ctr=None, n_in=None, out_tokens=None, out_stride=0,
           carry=None):
    """-> (the rows after the launch, the state row after it)."""
    M, ldl = lg.shape
    buf = guarded(ti, lg.nbytes)
    buf.upload(lg)
    st = guarded(ti, M * 4)
    st.upload(np.ascontiguousarray(state, i32))
    a = ti.GuideArgs(buf.ptr, ldl, M, V, dg.c, st.ptr, draw_stride, advance, step_ctr.ptr if step_ctr else None,
                     n_in.ptr if n_in else None, out_tokens.ptr if out_tokens else None, out_stride,
                     carry.ptr if carry else None)
    ti.check(ti.lib().ti_guide_step(C.byref(a), None))
    ti.sync()
    guard_intact(ti, buf, lg.nbytes, "the logits")
    guard_intact(ti, st, M * 4, "the state row")
    dg.unchanged()
    return fetch(ti, buf, 0, lg.nbytes).view(f32).reshape(M, ldl), fetch(ti, st, 0, M * 4).view(i32)


@pytest.mark.parametrize("M", [1, 3, 64])
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("V", [1, 31, 32, 33, 1000, 32003])
def test_mask_matches_the_restatement(ti, V, pad, M):
    g = states_guide(V)
    assert R.check(g, V) is None
    dg = DevGuide(ti, g, V)
    ldl = V + pad
    # the mask shapes cycled over the streams, one free slot (-1) among them when there is room
    state = np.array([(m + M) % g.n_states for m in range(M)], i32)
    if M > 1:
        state[M // 2] = -1
    lg = rows_for(M, V, ldl, seed=V + M)
    got, st = launch(ti, dg, lg, V, state)            # step_ctr null: t = 0; no carry: the states do not move
    assert np.array_equal(st, state)
    for m in range(M):
        want = R.mask(g, int(state[m]), lg[m, :V])
        assert np.array_equal(R.bits(got[m, :V]), R.bits(want)), (m, state[m], np.flatnonzero(R.bits(got[m, :V]) != R.bits(want))[:8])
        assert np.all(R.bits(got[m, V:]) == PAD_BITS), f"stream {m}: a pad column changed"
    again, st2 = launch(ti, dg, lg, V, state)
    assert np.array_equal(R.bits(again), R.bits(got)) and np.array_equal(st2, state)


CARRY = {"null": None, "minus1": [-1, -1, -1], "allowed": [5, 11, 2], "refused": [0, 11, 7]}


@pytest.mark.parametrize("advance", [1, 0])
@pytest.mark.parametrize("carry", list(CARRY))
def test_stepping_consumes_exactly_what_each_step_fed(ti, carry, advance):
    """M = 3, n_in = (1, 3, 5), draw_stride = 4, the step counter swept 0 .. 8 with fresh rows each step: stream m's
    draw index is t = (ctr - advance) - (n_in[m] - 1); outside [0, 4) the row and the state keep their bits; at
    t >= 1 the state first consumes out_tokens[m][t - 1], at t == 0 its carry (non-null and >= 0).  The guide is
    the cycle over ids mod 3 in V = 1000 (ldl 1003); stream 2's feed leaves it at t = 2, into the dead state."""
    M, V, ldl, stride, out_stride = 3, 1000, 1003, 4, 6
    g = R.cycle(V, 3)
    dg = DevGuide(ti, g, V)
    n_in = np.array([1, 3, 5], i32)
    start = [2, 2, 1]                                   # "allowed" carries 5, 11, 2 (= 2, 2, 2 mod 3): stream 2's is refused
    out = np.array([[0, 1, 2, 7, 7, 7], [3, 4, 5, 8, 8, 8], [1, 5, 999, 9, 9, 9]], i32)
    cv = CARRY[carry]
    d_nin, d_out, d_ctr = dev(ti, n_in), dev(ti, out), ti.DeviceBuffer(4)
    d_carry = dev(ti, np.array(cv, i32)) if cv is not None else None
    state = np.array(start, i32)
    active = dead = 0
    for ctr in range(9):
        d_ctr.upload(np.array([ctr], i32))
        lg = rows_for(M, V, ldl, seed=4000 + ctr)
        got, new_state = launch(ti, dg, lg, V, state, draw_stride=stride, advance=advance, step_ctr=d_ctr, n_in=d_nin,
                                out_tokens=d_out, out_stride=out_stride, carry=d_carry)
        for m in range(M):
            t = (ctr - advance) - (int(n_in[m]) - 1)
            s = int(state[m])
            if 0 <= t < stride:
                active += 1
                tok = int(out[m, t - 1]) if t >= 1 else (cv[m] if cv is not None else -1)
                s = R.advance(g, s, tok)
                dead += s < 0
                want = R.mask(g, s, lg[m, :V])
            else:
                want = lg[m, :V]
            assert int(new_state[m]) == s, (ctr, m, t)
            assert np.array_equal(R.bits(got[m, :V]), R.bits(want)), (ctr, m, t)
            assert np.all(R.bits(got[m, V:]) == PAD_BITS)
        state = new_state.copy()
    assert active >= 9 and dead >= 1


def test_stale_state_is_treated_as_free(ti):
    V = 100
    g = R.cycle(V, 3)
    dg = DevGuide(ti, g, V)
    lg = rows_for(2, V, V, seed=1)
    got, st = launch(ti, dg, lg, V, [3, 2 ** 31 - 1])   # no state of this guide
    assert np.array_equal(R.bits(got), R.bits(lg))


def test_reset_sets_only_its_slots(ti):
    st = guarded(ti, 8 * 4)
    st.upload(np.arange(100, 108, dtype=i32))
    ti.check(ti.lib().ti_guide_reset(st.ptr, 2, 3, 7, None))
    ti.check(ti.lib().ti_guide_reset(st.ptr, 7, 1, -1, None))
    ti.sync()
    guard_intact(ti, st, 32, "the state row")
    assert fetch(ti, st, 0, 32).view(i32).tolist() == [100, 101, 7, 7, 7, 105, 106, -1]
