"""ti_penalty_step_rows (kernels/penalty.hip): ti_penalty_step with each row's repetition / presence / frequency taken
from a device table of ti_row_params, against the product's host restatement ti_penalize_logits, bit for bit.

V = 1000, 5 rows whose contexts (with repeats) are loaded by ti_penalty_reset, the rows' values
(1.3, 0, 0), (1, 0.5, 0.25), (0.8, -0.5, 0.1), (1, 0, 0), (nan, 0, 0): the first three are penalised exactly as the
host function penalises them; the last two -- a request that does not penalise, an entry ti_penalty_step would have
refused -- keep every logit bit and their counts / seen / n_seen rows, even when the step feeds them a token.  The
struct's own three values are NaN throughout: nothing may read them.  The stepping test sweeps the counter with
n_in = (1, 3, 2, 1, 2): per row, outside the draw window nothing moves, inside it the token the step fed
(out_tokens at t >= 1, the carry at t == 0) is noted first -- ti_penalty_step's rules.  Buffers are exactly as large
as advertised with the 0xA5 pattern behind them (the helpers of tests/test_gpu_penalty_kernels.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import penalty_ref as R
from test_gpu_attn_oracle import dev, fetch, guard_intact, guarded
from test_gpu_penalty_kernels import State

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
V, LDL, M = 1000, 1000, 5
NAN = float("nan")
VALUES = [(1.3, 0.0, 0.0), (1.0, 0.5, 0.25), (0.8, -0.5, 0.1), (1.0, 0.0, 0.0), (NAN, 0.0, 0.0)]
ACTIVE = (0, 1, 2)
KINDS = ("seven300", "rand2047", "same40", "seven300", "rand2047")


def table(values):
    t = np.zeros(len(values), np.dtype([("t", f32), ("k", i32), ("p", f32), ("pen", f32, 3), ("res", i32, 2)]))
    assert t.itemsize == 32
    for m, v in enumerate(values):
        t[m] = (1.0, 1, 1.0, v, (0, 0))
    return t


def contexts():
    return [R.context(KINDS[m], V, seed=m) for m in range(M)]


def loaded_state(ti, ctxs):
    st = State(ti, M, V)
    for m, ctx in enumerate(ctxs):
        st.reset(m, ctx)
    return st


def step_rows(ti, st, lg, values, draw_stride=1, advance=1, step_ctr=None, n_in=None, out_tokens=None, out_stride=0,
              carry=None):
    """One launch on a guarded copy of lg -> the rewritten logits (guards of logits and state checked)."""
    buf = guarded(ti, lg.nbytes)
    buf.upload(lg)
    td = dev(ti, table(values))
    a = ti.PenaltyArgs(buf.ptr, LDL, M, V, st.c, NAN, NAN, NAN, draw_stride, advance,
                       step_ctr.ptr if step_ctr else None, n_in.ptr if n_in else None,
                       out_tokens.ptr if out_tokens else None, out_stride, carry.ptr if carry else None)
    ti.check(ti.lib().ti_penalty_step_rows(C.byref(a), td.ptr, None))
    ti.sync()
    guard_intact(ti, buf, lg.nbytes, "the logits")
    st.guards_intact()
    return fetch(ti, buf, 0, lg.nbytes).view(f32).reshape(M, LDL)


def host(ti, lg_row, counts, values):
    return ti.penalize_logits(lg_row, np.repeat(np.arange(V), counts), *values)


def logits_for(ctxs, seed):
    return np.stack([R.logits_for(ctx, V, seed + m) for m, ctx in enumerate(ctxs)])


def test_rows_take_their_own_values(ti):
    ctxs = contexts()
    st = loaded_state(ti, ctxs)
    before = [a.copy() for a in st.read()]
    lg = logits_for(ctxs, 1)
    got = step_rows(ti, st, lg, VALUES)                 # step_ctr null: t = 0; no carry: the state does not move
    for m in range(M):
        want = host(ti, lg[m], R.counts_of(ctxs[m], V), VALUES[m]) if m in ACTIVE else lg[m]
        assert np.array_equal(R.bits(got[m]), R.bits(want)), (m, np.flatnonzero(R.bits(got[m]) != R.bits(want))[:8])
        if m in ACTIVE:
            assert not np.array_equal(R.bits(got[m]), R.bits(lg[m])), m
    for b, a in zip(before, st.read()):
        assert np.array_equal(b, a)
    # the values are the row's, not the slot's: the table rotated by one
    rot = VALUES[1:] + VALUES[:1]
    got = step_rows(ti, st, lg, rot)
    for m in range(M):
        want = lg[m] if rot[m] in (VALUES[3], VALUES[4]) else host(ti, lg[m], R.counts_of(ctxs[m], V), rot[m])
        assert np.array_equal(R.bits(got[m]), R.bits(want)), m


def test_a_row_that_does_not_penalise_notes_nothing(ti):
    """Every row is fed a token through the carry (t = 0): the penalising rows count it before they walk, the other
    two leave logits, counts, seen and n_seen as they were."""
    ctxs = contexts()
    st = loaded_state(ti, ctxs)
    before = [a.copy() for a in st.read()]
    fed = np.array([int(ctxs[0][0]), 901, 902, 903, int(ctxs[4][0])], i32)      # a counted token, new ones
    lg = logits_for(ctxs, 2)
    got = step_rows(ti, st, lg, VALUES, carry=dev(ti, fed))
    counts, seen, n_seen = st.read()
    for m in range(M):
        c = R.counts_of(ctxs[m], V)
        if m in ACTIVE:
            c[fed[m]] += 1
            st.check(m, c)
            assert np.array_equal(R.bits(got[m]), R.bits(host(ti, lg[m], c, VALUES[m]))), m
        else:
            assert np.array_equal(R.bits(got[m]), R.bits(lg[m])), m
            assert np.array_equal(counts[m], before[0][m]) and np.array_equal(seen[m], before[1][m]), m
            assert n_seen[m] == before[2][m], m


@pytest.mark.parametrize("advance", [1, 0])
def test_stepping_rules_hold_per_row(ti, advance):
    stride, out_stride = 3, 5
    n_in = np.array([1, 3, 2, 1, 2], i32)
    ctxs = contexts()
    st = loaded_state(ti, ctxs)
    counts = [R.counts_of(ctx, V) for ctx in ctxs]
    frozen = [a.copy() for a in st.read()]
    rng = np.random.RandomState(6)
    out = rng.randint(0, V, (M, out_stride)).astype(i32)
    out[:, 1] = out[:, 0]                               # the same new token twice
    carry = np.array([950, -1, 951, 952, 953], i32)     # row 1 has none
    d_nin, d_out, d_ctr, d_carry = dev(ti, n_in), dev(ti, out), ti.DeviceBuffer(4), dev(ti, carry)
    active = 0
    for ctr in range(7):
        d_ctr.upload(np.array([ctr], i32))
        lg = (np.random.RandomState(4000 + ctr).standard_normal((M, LDL)) * 2.0).astype(f32)
        got = step_rows(ti, st, lg, VALUES, draw_stride=stride, advance=advance, step_ctr=d_ctr, n_in=d_nin,
                        out_tokens=d_out, out_stride=out_stride, carry=d_carry)
        now = st.read()
        for m in range(M):
            t = (ctr - advance) - (int(n_in[m]) - 1)
            if m in ACTIVE and 0 <= t < stride:
                active += 1
                tok = int(out[m, t - 1]) if t >= 1 else int(carry[m])
                if tok >= 0:
                    counts[m][tok] += 1
                want = host(ti, lg[m], counts[m], VALUES[m])
            else:
                want = lg[m]
            assert np.array_equal(R.bits(got[m]), R.bits(want)), (ctr, m, t)
            if m in ACTIVE:
                st.check(m, counts[m])
            else:
                assert all(np.array_equal(f[m], a[m]) for f, a in zip(frozen, now)), (ctr, m)
    assert active >= 8
