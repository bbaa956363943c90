"""ti_penalty_reset + ti_penalty_step (kernels/penalty.hip) against the NumPy float32 restatement
(tests/penalty_ref.py), bit for bit.

Every launch works on buffers of exactly the advertised size with a 0xA5 pattern behind them (the helpers of
tests/test_gpu_attn_oracle.py): the logits [M][ldl] and the three state buffers.  Checked: the histogram and the
distinct-token list a reset leaves, the rewritten logits of every stream (pad columns and uncounted tokens keep
their bits), a second identical run, slots other than the one reset, and the decode loop's stepping -- rows
outside their draw window keep logits and state, the others accumulate the tokens the step fed (out_tokens,
carry) exactly."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import penalty_ref as R
from test_gpu_attn_oracle import dev, fetch, fill, guard_intact, guarded

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
SHAPES = [(1000, 1000), (4100, 4104)]      # (V, ldl)


class State:
    """counts / seen [M][V] and n_seen [M] on the device, each with the guard pattern behind it."""

    def __init__(self, ti, M, V, byte=0):
        self.ti, self.M, self.V = ti, M, V
        self.sizes = dict(counts=M * V * 4, seen=M * V * 4, n_seen=M * 4)
        self.buf = {k: guarded(ti, n) for k, n in self.sizes.items()}
        for k, n in self.sizes.items():
            fill(ti, self.buf[k], 0, n, byte)
        self.c = ti.PenaltyState(self.buf["counts"].ptr, self.buf["seen"].ptr, self.buf["n_seen"].ptr)

    def reset(self, m, ctx):
        ctx = np.ascontiguousarray(ctx, i32)
        d = dev(self.ti, ctx) if ctx.size else None
        self.ti.check(self.ti.lib().ti_penalty_reset(C.byref(self.c), self.V, m, d.ptr if d else None, ctx.size, None))
        self.ti.sync()

    def read(self):
        g = {k: fetch(self.ti, self.buf[k], 0, n).view(i32) for k, n in self.sizes.items()}
        return g["counts"].reshape(self.M, self.V), g["seen"].reshape(self.M, self.V), g["n_seen"]

    def guards_intact(self):
        for k, n in self.sizes.items():
            guard_intact(self.ti, self.buf[k], n, k)

    def check(self, m, counts):
        """Slot m holds exactly the histogram `counts` [V]."""
        c, s, n = self.read()
        ids = np.flatnonzero(counts)
        assert np.array_equal(c[m], counts), f"slot {m}: counts"
        assert n[m] == ids.size, f"slot {m}: n_seen {n[m]} for {ids.size} distinct ids"
        assert sorted(s[m, : n[m]].tolist()) == ids.tolist(), f"slot {m}: seen"


def step(ti, st, logits_buf, ldl, M, V, params, draw_stride=1, advance=1, step_ctr=None, n_in=None, out_tokens=None,
         out_stride=0, carry=None):
    a = ti.PenaltyArgs(logits_buf.ptr, ldl, M, V, st.c, params[0], params[1], params[2], draw_stride, advance,
                       step_ctr.ptr if step_ctr else None, n_in.ptr if n_in else None,
                       out_tokens.ptr if out_tokens else None, out_stride, carry.ptr if carry else None)
    ti.check(ti.lib().ti_penalty_step(C.byref(a), None))
    ti.sync()


def padded_logits(contexts, V, ldl, seed):
    """[M][ldl] float32: each row's first V columns are penalty_ref.logits_for its context, the pad is random."""
    M = len(contexts)
    lg = (np.random.RandomState(3000 + seed).standard_normal((M, ldl)) * 2.0).astype(f32)
    for m, ctx in enumerate(contexts):
        lg[m, :V] = R.logits_for(ctx, V, seed + m)
    return lg


def run(ti, st, lg, V, params, **kw):
    M, ldl = lg.shape
    buf = guarded(ti, lg.nbytes)
    buf.upload(lg)
    step(ti, st, buf, ldl, M, V, params, **kw)
    guard_intact(ti, buf, lg.nbytes, "the logits")
    st.guards_intact()
    return fetch(ti, buf, 0, lg.nbytes).view(f32).reshape(M, ldl)


@pytest.mark.parametrize("params", R.PARAMS, ids=lambda p: "r%g_p%g_f%g" % p)
@pytest.mark.parametrize("M", [1, 3, 64])
@pytest.mark.parametrize("V,ldl", SHAPES)
def test_reset_and_step_match_the_restatement(ti, V, ldl, M, params):
    # the context kinds cycled over the streams ("perm": n_seen = V, more than the workgroup has threads)
    contexts = [R.context(R.CONTEXT_KINDS[(m + M) % len(R.CONTEXT_KINDS)], V, seed=m) for m in range(M)]
    st = State(ti, M, V)
    for m, ctx in enumerate(contexts):
        st.reset(m, ctx)
    st.guards_intact()
    for m, ctx in enumerate(contexts):
        st.check(m, R.counts_of(ctx, V))
    lg = padded_logits(contexts, V, ldl, seed=M)
    got = run(ti, st, lg, V, params)                 # step_ctr null: t = 0; no carry: the state does not move
    for m, ctx in enumerate(contexts):
        ref = R.penalize(lg[m, :V], ctx, *params)
        assert np.array_equal(R.bits(got[m, :V]), R.bits(ref)), (m, np.flatnonzero(R.bits(got[m, :V]) != R.bits(ref))[:8])
        assert np.array_equal(R.bits(got[m, V:]), R.bits(lg[m, V:])), f"stream {m}: a pad column changed"
        st.check(m, R.counts_of(ctx, V))
    again = run(ti, st, lg, V, params)
    assert np.array_equal(R.bits(again), R.bits(got))


def test_reset_leaves_the_other_slots(ti):
    M, V = 3, 1000
    st = State(ti, M, V, byte=0x5A)
    before = [a.copy() for a in st.read()]
    ctx = R.context("seven300", V)
    st.reset(1, ctx)
    st.guards_intact()
    st.check(1, R.counts_of(ctx, V))
    after = st.read()
    for b, a in zip(before, after):
        assert np.array_equal(b[0], a[0]) and np.array_equal(b[2], a[2])
    st.reset(1, [])                                   # n = 0 empties the slot
    st.check(1, np.zeros(V, np.int64))
    st.reset(1, [5, -1, V, 5])                        # ids outside [0, V) are skipped
    st.check(1, R.counts_of([5, 5], V))


def test_stale_state_cannot_index_out_of_bounds(ti):
    """A slot nobody reset: n_seen beyond V is clamped to V, ids outside [0, V) are skipped."""
    M, V, ldl = 2, 1000, 1000
    st = State(ti, M, V)
    counts = np.zeros((M, V), i32)
    seen = np.zeros((M, V), i32)
    counts[0, [3, 7]] = [2, 1]
    seen[0, :6] = [3, -5, V, V + 3, 2 ** 31 - 1, 7]
    seen[0, 6:] = -1
    seen[1, :] = V + 9
    st.buf["counts"].upload(counts)
    st.buf["seen"].upload(seen)
    st.buf["n_seen"].upload(np.array([V + 100, 2 ** 31 - 1], i32))
    lg = padded_logits([[3, 3, 7], []], V, ldl, seed=9)
    got = run(ti, st, lg, V, (1.1, 0.4, 0.2))
    assert np.array_equal(R.bits(got[0]), R.bits(R.penalize(lg[0], [3, 3, 7], 1.1, 0.4, 0.2)))
    assert np.array_equal(R.bits(got[1]), R.bits(lg[1]))


CARRY = {"null": None, "minus1": [-1, -1, -1], "new": [900, 901, 902], "seen": [11, 12, 13]}


@pytest.mark.parametrize("advance", [1, 0])
@pytest.mark.parametrize("carry", list(CARRY))
def test_stepping_accumulates_exactly_what_each_step_fed(ti, carry, advance):
    """M = 3, n_in = (1, 3, 5), draw_stride = 4, the step counter swept 0 .. 8 with fresh logits each step: stream
    m's draw index is t = (ctr - advance) - (n_in[m] - 1); outside [0, 4) logits and state keep their bits; at
    t >= 1 the row first notes out_tokens[m][t - 1], at t == 0 its carry (non-null and >= 0)."""
    M, V, ldl, stride, out_stride, params = 3, 1000, 1000, 4, 6, (1.1, 0.4, 0.2)
    n_in = np.array([1, 3, 5], i32)
    contexts = [np.array(c, i32) for c in ([11, 40, 11], [12, 41], [13, 13, 13, 42, 43])]
    # the feed record: a token of the context, a new one, the same new one again
    out = np.array([[11, 500, 500, 7, 7, 7], [600, 41, 600, 8, 8, 8], [13, 13, 700, 9, 9, 9]], i32)
    st = State(ti, M, V)
    for m, ctx in enumerate(contexts):
        st.reset(m, ctx)
    counts = [R.counts_of(ctx, V) for ctx in contexts]
    cv = CARRY[carry]
    d_nin, d_out, d_ctr = dev(ti, n_in), dev(ti, out), ti.DeviceBuffer(4)
    d_carry = dev(ti, np.array(cv, i32)) if cv is not None else None
    active = 0
    for ctr in range(9):
        d_ctr.upload(np.array([ctr], i32))
        lg = (np.random.RandomState(4000 + ctr).standard_normal((M, ldl)) * 2.0).astype(f32)
        got = run(ti, st, lg, V, params, draw_stride=stride, advance=advance, step_ctr=d_ctr, n_in=d_nin,
                  out_tokens=d_out, out_stride=out_stride, carry=d_carry)
        for m in range(M):
            t = (ctr - advance) - (int(n_in[m]) - 1)
            if 0 <= t < stride:
                active += 1
                tok = int(out[m, t - 1]) if t >= 1 else (cv[m] if cv is not None else -1)
                if tok >= 0:
                    counts[m][tok] += 1
                ref = R.penalize(lg[m], np.repeat(np.arange(V), counts[m]), *params)
            else:
                ref = lg[m]
            assert np.array_equal(R.bits(got[m]), R.bits(ref)), (ctr, m, t)
            st.check(m, counts[m])
    assert active >= 9
