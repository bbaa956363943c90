"""ti_guide_step_rows (kernels/guide.hip): ti_guide_step with each row's guide picked by the handle in its ti_row_params
entry (reserved[0]) out of a device table of ti_guide_dev descriptors.  References: the scalar ti_guide_step launched
with the row's descriptor on that row alone, and the NumPy restatement tests/guide_ref.py -- both bit for bit.

One launch of 9 rows (ROWS below): three different guides (the mask shapes of tests/test_gpu_guide_kernels.py, a ban,
a cycle), a second row on the first guide, and five rows that must do nothing at all -- handle 0, handle -1, handle
guide_cap + 1, the handle of a zeroed entry, and an entry whose mask_words is wrong.  Every row is fed a token through
the carry, so valid rows move their state before they mask and the others show that they consumed nothing.  The
struct's own descriptor (a->guide) is all-zero throughout: nothing may read it.  Logits rows hold the planted values
of the scalar test (+-inf, +-0, +-FMAX, a denormal, NaN), the row padding a NaN payload, and 0xA5 guard words stand
behind the logits, the state row, the carry, both tables and the guides' buffers."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import guide_ref as R
from test_gpu_attn_oracle import dev, fetch, guard_intact, guarded
from test_gpu_guide_kernels import CARRY, PAD_BITS, DevGuide, rows_for, states_guide

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
ROW_T = np.dtype([("t", f32), ("k", i32), ("p", f32), ("pen", f32, 3), ("res", i32, 2)])
CAP = 5                      # handles 1 .. 3: the guides; 4: a zeroed entry; 5: mask_words off by one
H_ZERO, H_BAD_WORDS = 4, 5
# (handle, state before the launch) per row; the guides of handles 1 .. 3 are GUIDES(V)
ROWS = [(1, 2), (2, 0), (3, 1), (0, 0), (-1, 0), (CAP + 1, 0), (H_ZERO, 0), (H_BAD_WORDS, 1), (1, 3)]
VALID = [m for m, (h, _) in enumerate(ROWS) if 1 <= h <= 3]


def guides_for(V):
    """Handles 1, 2, 3."""
    banned = {0, V // 2, V - 1} if V > 3 else set()
    return [states_guide(V), R.ban(V, banned), R.cycle(V, min(3, V))]


class Table:
    """The device table [CAP] of descriptors, guarded, over the guides' own guarded buffers."""

    def __init__(self, ti, guides, V):
        self.ti = ti
        self.dg = [DevGuide(ti, g, V) for g in guides]
        arr = (ti.GuideDev * CAP)()
        for i, d in enumerate(self.dg):
            arr[i] = d.c
        c = self.dg[2].c
        arr[H_BAD_WORDS - 1] = ti.GuideDev(c.n_states, c.mask_words + 1, c.row_ptr, c.tokens, c.next, c.mask)
        self.host = np.frombuffer(bytes(arr), np.uint8).copy()
        assert self.host.size == CAP * 40 and not self.host[(H_ZERO - 1) * 40: H_ZERO * 40].any()
        self.buf = guarded(ti, self.host.size)
        self.buf.upload(self.host)

    def unchanged(self):
        assert np.array_equal(fetch(self.ti, self.buf, 0, self.host.size), self.host), "the descriptor table changed"
        guard_intact(self.ti, self.buf, self.host.size, "the descriptor table")
        for d in self.dg:
            d.unchanged()


def row_table(handles):
    t = np.zeros(len(handles), ROW_T)
    assert t.itemsize == 32
    for m, h in enumerate(handles):
        t[m] = (1.0, 1, 1.0, (1.0, 0.0, 0.0), (h, 0))
    return t


def launch_rows(ti, tab, lg, V, handles, state, draw_stride=1, advance=1, step_ctr=None, n_in=None, out_tokens=None,
                out_stride=0, carry=None, bad=None):
    """One ti_guide_step_rows launch on guarded copies -> (rows after, state row after); every guard checked.
    bad: arguments overridden (GuideArgs fields, guides_ptr / rows_ptr False for null, cap); the call must then
    fail with TI_ERR_ARG."""
    M, ldl = lg.shape
    buf = guarded(ti, lg.nbytes)
    buf.upload(lg)
    st = guarded(ti, M * 4)
    st.upload(np.ascontiguousarray(state, i32))
    rt_host = row_table(handles)
    rt = guarded(ti, rt_host.nbytes)
    rt.upload(rt_host)
    cr = None
    if carry is not None:
        cr = guarded(ti, M * 4)
        cr.upload(np.ascontiguousarray(carry, i32))
    f = dict(logits=buf.ptr, ldl=ldl, M=M, V=V, state=st.ptr, draw_stride=draw_stride, out_stride=out_stride,
             out_tokens=out_tokens.ptr if out_tokens else None)
    f.update(guides_ptr=True, rows_ptr=True, cap=CAP)
    f.update(bad or {})
    a = ti.GuideArgs(f["logits"], f["ldl"], f["M"], f["V"], ti.GuideDev(), f["state"], f["draw_stride"], advance,
                     step_ctr.ptr if step_ctr else None, n_in.ptr if n_in else None, f["out_tokens"], f["out_stride"],
                     cr.ptr if cr else None)
    rc = ti.lib().ti_guide_step_rows(C.byref(a), tab.buf.ptr if f["guides_ptr"] else None, f["cap"],
                                     rt.ptr if f["rows_ptr"] else None, None)
    if bad is not None:
        assert rc == 1 and b"ti_guide_step_rows" in ti.lib().ti_last_error(), (rc, bad)
    else:
        ti.check(rc)
    ti.sync()
    guard_intact(ti, buf, lg.nbytes, "the logits")
    guard_intact(ti, st, M * 4, "the state row")
    guard_intact(ti, rt, rt_host.nbytes, "the row table")
    assert np.array_equal(fetch(ti, rt, 0, rt_host.nbytes), rt_host.view(np.uint8).reshape(-1)), "the row table changed"
    if cr:
        guard_intact(ti, cr, M * 4, "the carry")
    tab.unchanged()
    return fetch(ti, buf, 0, lg.nbytes).view(f32).reshape(M, ldl), fetch(ti, st, 0, M * 4).view(i32)


def launch_scalar_row(ti, dg, lg, V, state, m, carry):
    """ti_guide_step with dg's descriptor on row m alone (M = 1, the row at its place in the [M][ldl] buffer, so at
    the same address alignment) -> (all rows after, the whole state row after)."""
    M, ldl = lg.shape
    buf = guarded(ti, lg.nbytes)
    buf.upload(lg)
    st = guarded(ti, M * 4)
    st.upload(np.ascontiguousarray(state, i32))
    cr = dev(ti, np.ascontiguousarray(carry, i32))
    a = ti.GuideArgs(buf.ptr + m * ldl * 4, ldl, 1, V, dg.c, st.ptr + m * 4, 1, 1, None, None, None, 0, cr.ptr + m * 4)
    ti.check(ti.lib().ti_guide_step(C.byref(a), None))
    ti.sync()
    guard_intact(ti, buf, lg.nbytes, "the logits")
    guard_intact(ti, st, M * 4, "the state row")
    return fetch(ti, buf, 0, lg.nbytes).view(f32).reshape(M, ldl), fetch(ti, st, 0, M * 4).view(i32)


def carry_for(guides, V, state):
    """A token per row: rows 0 and 2 one their state allows (they move), row 1 a banned one when there is one (it
    dies), row 8 one its state allows; the rows that must do nothing get a token too."""
    c = np.zeros(len(ROWS), i32)
    for m in VALID:
        c[m] = int(guides[ROWS[m][0] - 1].allowed(int(state[m]))[-1])
    if V > 3:
        c[1] = V // 2
    return c


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("V", [1, 33, 1000, 32003])
def test_rows_take_their_own_guides(ti, V, pad):
    guides = guides_for(V)
    tab = Table(ti, guides, V)
    M, ldl = len(ROWS), V + pad
    handles = [h for h, _ in ROWS]
    state = np.array([min(s, guides[h - 1].n_states - 1) if 1 <= h <= 3 else s for h, s in ROWS], i32)
    carry = carry_for(guides, V, state)
    lg = rows_for(M, V, ldl, seed=77 + V)
    got, st = launch_rows(ti, tab, lg, V, handles, state, carry=carry)
    moved = 0
    for m in range(M):
        h = handles[m]
        if m in VALID:
            g = guides[h - 1]
            s = R.advance(g, int(state[m]), int(carry[m]))
            want = R.mask(g, s, lg[m, :V])
            assert int(st[m]) == s, (m, st[m], s)
            assert np.array_equal(R.bits(got[m, :V]), R.bits(want)), (m, np.flatnonzero(R.bits(got[m, :V]) != R.bits(want))[:8])
            ref_lg, ref_st = launch_scalar_row(ti, tab.dg[h - 1], lg, V, state, m, carry)
            assert np.array_equal(R.bits(ref_lg[m]), R.bits(got[m])) and ref_st[m] == st[m], m
            others = [x for x in range(M) if x != m]
            assert np.array_equal(R.bits(ref_lg[others]), R.bits(lg[others])) and np.array_equal(ref_st[others], state[others])
            moved += s != state[m]
        else:
            assert st[m] == state[m], (m, h)
            assert np.array_equal(R.bits(got[m]), R.bits(lg[m])), (m, h)
        assert np.all(R.bits(got[m, V:]) == PAD_BITS), f"row {m}: a pad column changed"
    assert moved >= 1 or V == 1
    if V > 3:
        assert st[1] == -1 and np.array_equal(R.bits(got[1]), R.bits(lg[1]))     # the banned token killed row 1
    # the same rows in another order give the same rows in that order
    perm = np.random.RandomState(V).permutation(M)
    got_p, st_p = launch_rows(ti, tab, lg[perm], V, [handles[i] for i in perm], state[perm], carry=carry[perm])
    assert np.array_equal(R.bits(got_p), R.bits(got[perm])) and np.array_equal(st_p, st[perm])


@pytest.mark.parametrize("advance", [1, 0])
@pytest.mark.parametrize("carry", list(CARRY))
def test_stepping_consumes_exactly_what_each_step_fed(ti, carry, advance):
    """The sweep of tests/test_gpu_guide_kernels.py, three rows on three guides: M = 3, n_in = (1, 3, 5), draw_stride
    4, the step counter swept 0 .. 8 with fresh rows each step.  Row m's draw index is t = (ctr - advance) -
    (n_in[m] - 1); outside [0, 4) the row and its state keep their bits; at t >= 1 the state first consumes
    out_tokens[m][t - 1], at t == 0 its carry (non-null and >= 0) -- each in the row's own automaton."""
    M, V, ldl, stride, out_stride = 3, 1000, 1003, 4, 6
    guides = guides_for(V)
    tab = Table(ti, guides, V)
    handles = [3, 1, 2]                                 # the cycle, the mask shapes (6 states, v -> v mod 6), the ban
    n_in = np.array([1, 3, 5], i32)
    start = [2, 3, 0]                                   # (state 3 of the mask shapes allows every id)
    out = np.array([[0, 1, 2, 7, 7, 7], [3, 4, 5, 8, 8, 8], [1, 5, 999, 9, 9, 9]], i32)   # 999 is banned: row 2 dies
    cv = CARRY[carry]
    d_nin, d_out, d_ctr = dev(ti, n_in), dev(ti, out), ti.DeviceBuffer(4)
    state = np.array(start, i32)
    active = dead = alive = 0
    for ctr in range(9):
        d_ctr.upload(np.array([ctr], i32))
        lg = rows_for(M, V, ldl, seed=4000 + ctr)
        got, new_state = launch_rows(ti, tab, lg, V, handles, state, draw_stride=stride, advance=advance, step_ctr=d_ctr,
                                     n_in=d_nin, out_tokens=d_out, out_stride=out_stride, carry=cv)
        for m in range(M):
            g = guides[handles[m] - 1]
            t = (ctr - advance) - (int(n_in[m]) - 1)
            s = int(state[m])
            if 0 <= t < stride:
                active += 1
                tok = int(out[m, t - 1]) if t >= 1 else (cv[m] if cv is not None else -1)
                s = R.advance(g, s, tok)
                dead += s < 0
                alive += s >= 0
                want = R.mask(g, s, lg[m, :V])
            else:
                want = lg[m, :V]
            assert int(new_state[m]) == s, (ctr, m, t)
            assert np.array_equal(R.bits(got[m, :V]), R.bits(want)), (ctr, m, t)
            assert np.all(R.bits(got[m, V:]) == PAD_BITS)
        state = new_state.copy()
    assert active >= 9 and dead >= 1 and alive >= 3


def test_a_state_of_another_rows_larger_guide_is_free(ti):
    """State 5 is a state of the 6-state guide of row 0 and none of the 3-state cycle of row 1: row 1 is treated as
    free (-1) -- nothing masked, nothing consumed -- exactly as the scalar launch of the cycle treats it."""
    V = 1000
    guides = guides_for(V)
    tab = Table(ti, guides, V)
    lg = rows_for(2, V, V + 5, seed=3)
    state, carry = np.array([5, 5], i32), np.array([7, 7], i32)       # (state 5 of row 0's guide allows the odd ids)
    got, st = launch_rows(ti, tab, lg, V, [1, 3], state, carry=carry)
    s0 = R.advance(guides[0], 5, 7)
    assert s0 >= 0 and st[0] == s0
    assert np.array_equal(R.bits(got[0, :V]), R.bits(R.mask(guides[0], s0, lg[0, :V])))
    assert not np.array_equal(R.bits(got[0]), R.bits(lg[0]))
    ref_lg, ref_st = launch_scalar_row(ti, tab.dg[2], lg, V, state, 1, carry)
    assert np.array_equal(R.bits(got[1]), R.bits(lg[1])) and np.array_equal(R.bits(ref_lg[1]), R.bits(lg[1]))
    assert st[1] == ref_st[1] == 5


BAD = [dict(logits=None), dict(state=None), dict(guides_ptr=False), dict(rows_ptr=False), dict(cap=0), dict(cap=-3),
       dict(M=0), dict(V=0), dict(ldl=999), dict(draw_stride=0), dict(out_stride=-1)]


def test_argument_errors_launch_nothing(ti):
    V = 1000
    guides = guides_for(V)
    tab = Table(ti, guides, V)
    lg = rows_for(3, V, V, seed=5)
    state, carry = np.array([2, 0, 1], i32), np.array([5, 1, 4], i32)
    for bad in BAD:
        got, st = launch_rows(ti, tab, lg, V, [1, 2, 3], state, carry=carry, bad=bad)
        assert np.array_equal(R.bits(got), R.bits(lg)) and np.array_equal(st, state), bad
    # a step counter without the feed record, and null args
    ctr = dev(ti, np.zeros(1, i32))
    got, st = launch_rows(ti, tab, lg, V, [1, 2, 3], state, carry=carry, step_ctr=ctr, bad={})
    assert np.array_equal(R.bits(got), R.bits(lg)) and np.array_equal(st, state)
    assert ti.lib().ti_guide_step_rows(None, tab.buf.ptr, CAP, tab.buf.ptr, None) == 1
    # and the same buffers do step with good arguments
    got, st = launch_rows(ti, tab, lg, V, [1, 2, 3], state, carry=carry)
    assert not np.array_equal(R.bits(got), R.bits(lg))


def test_the_module_wrapper_launches(ti):
    V = 100
    guides = guides_for(V)
    tab = Table(ti, guides, V)
    lg = rows_for(2, V, V, seed=9)
    buf, st = dev(ti, lg), dev(ti, np.array([0, 1], i32))
    rt = dev(ti, row_table([2, 0]))
    a = ti.GuideArgs(buf.ptr, V, 2, V, ti.GuideDev(), st.ptr, 1, 1, None, None, None, 0, None)
    ti.guide_step_rows(a, tab.buf, CAP, rt)
    ti.sync()
    got = buf.download(f32, (2, V))
    assert np.array_equal(R.bits(got[0]), R.bits(R.mask(guides[1], 0, lg[0])))
    assert np.array_equal(R.bits(got[1]), R.bits(lg[1]))
