"""The host guide helpers (ti_guide_check, ti_guide_apply; csrc/host/sampling.cpp) against the NumPy restatement
(tests/guide_ref.py), without a GPU: the mask bit for bit over rows that hold -inf, both zeros, NaN and the largest
finite values; the advance, into the dead state and out of it never; and every violation of the contract
ti_guide_check has to name."""
from __future__ import annotations

import os

import numpy as np
import pytest

import guide_ref as R
import turboinfer_amd as T

f32, i32 = np.float32, np.int32
FMAX = np.finfo(f32).max
PLANTED = np.array([-np.inf, np.inf, 0.0, -0.0, FMAX, -FMAX, 1e-40, np.nan], f32)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(T.LIB_PATH):
        T.build()
    return T.lib()


def row(V, seed):
    r = np.random.RandomState(seed)
    lg = (r.standard_normal(V) * 2.0).astype(f32)
    at = r.choice(V, min(V, 2 * PLANTED.size), replace=False)
    lg[at] = np.resize(PLANTED, at.size)
    return lg


def guides(V):
    every32 = list(range(0, V, 32))
    g = {
        "only0": R.Guide([[(0, 0)]]),
        "last": R.Guide([[(V - 1, 0)]]),
        "every32": R.Guide([[(v, 0) for v in every32]]),
        "all": R.Guide([[(v, 0) for v in range(V)]]),
        "cycle3": R.cycle(V, min(3, V)),
    }
    if V > 1:
        g["all_but_one"] = R.ban(V, [V // 2])
    return g


@pytest.mark.parametrize("V", [1, 31, 32, 33, 1000, 32003])
def test_apply_masks_bit_for_bit(L, V):
    for name, g in guides(V).items():
        assert R.check(g, V) is None, name
        T.guide_check(*g.args, V)
        for s in range(g.n_states):
            lg = row(V, 7 * V + s)
            ns, got = T.guide_apply(g.csr, s, -1, lg)
            assert ns == s, name
            want = R.mask(g, s, lg)
            assert np.array_equal(R.bits(got), R.bits(want)), (name, s, np.flatnonzero(R.bits(got) != R.bits(want))[:8])
            allowed = g.allowed(s)
            assert np.array_equal(R.bits(got[allowed]), R.bits(lg[allowed])), name
            assert np.count_nonzero(R.bits(got) == R.NEG_INF_BITS) >= V - allowed.size
        ns, got = T.guide_apply(g.csr, -1, 0, lg)                  # a free slot: nothing moves
        assert ns == -1 and np.array_equal(R.bits(got), R.bits(lg)), name


def test_apply_advances_then_masks(L):
    V = 1000
    g = R.cycle(V, 3)
    lg = row(V, 1)
    s = g.start
    for tok in [0, 1, 2, 3, 700, 998]:                              # 0 -> 1 -> 2 -> 0 -> 1 -> 2 -> 0
        ns, got = T.guide_apply(g.csr, s, tok, lg)
        assert ns == R.advance(g, s, tok) == (s + 1) % 3
        assert np.array_equal(R.bits(got), R.bits(R.mask(g, ns, lg)))
        s = ns
    states, ok = R.run(g, [0, 1, 2, 3, 700, 998])
    assert ok and states[-1] == s


def test_the_dead_state(L):
    V = 64
    g = R.forced(V, [5, 9])
    lg = row(V, 2)
    ns, got = T.guide_apply(g.csr, 0, 9, lg)                        # state 0 allows only 5
    assert ns == -1 == R.advance(g, 0, 9)
    assert np.array_equal(R.bits(got), R.bits(lg)), "a dead slot's row is left alone"
    ns, got = T.guide_apply(g.csr, -1, 5, lg)                       # and stays dead
    assert ns == -1 and np.array_equal(R.bits(got), R.bits(lg))
    assert T.guide_apply(g.csr, 0, V + 3, lg)[0] == -1              # an id no state can hold
    states, ok = R.run(g, [5, 9, 40, 41])
    assert ok and states == [0, 1, 2, 2, 2]
    states, ok = R.run(g, [5, 8, 40])
    assert not ok and states == [0, 1, -1, -1]


def broken(kind, V):
    g = R.Guide([[(1, 1), (5, 0), (9, 1)], [(2, 0), (7, 1)]])
    if kind == "unsorted":
        g.tokens = np.array([1, 9, 5, 2, 7], i32)
    elif kind == "duplicate":
        g.tokens = np.array([1, 5, 5, 2, 7], i32)
    elif kind == "token_negative":
        g.tokens = np.array([-1, 5, 9, 2, 7], i32)
    elif kind == "token_is_V":
        g.tokens = np.array([1, 5, 9, 2, V], i32)
    elif kind == "next_negative":
        g.next = np.array([1, 0, -1, 0, 1], i32)
    elif kind == "next_is_n":
        g.next = np.array([1, 0, 1, 0, 2], i32)
    elif kind == "empty_state":
        g.row_ptr = np.array([0, 5, 5], np.int64)
    elif kind == "start_negative":
        g.start = -1
    elif kind == "start_is_n":
        g.start = 2
    elif kind == "row_ptr_decreases":
        g.row_ptr = np.array([0, 6, 5], np.int64)
    elif kind == "row_ptr0":
        g.row_ptr = np.array([1, 3, 5], np.int64)
    return g


KINDS = ["unsorted", "duplicate", "token_negative", "token_is_V", "next_negative", "next_is_n", "empty_state",
         "start_negative", "start_is_n", "row_ptr_decreases", "row_ptr0"]


def test_check_accepts_the_intact_guide(L):
    g = broken("none", 10)
    assert R.check(g, 10) is None
    T.guide_check(*g.args, 10)
    assert L.ti_guide_check(None, 10) == 1 and b"ti_guide_check" in L.ti_last_error()
    with pytest.raises(T.TiError, match="ti error 1: ti_guide_check"):
        T.guide_check(*g.args, 0)
    with pytest.raises(T.TiError, match="ti error 1: ti_guide_check"):
        T.guide_check(*g.args, 9)                                   # 9 is no id of a 9-token vocabulary


@pytest.mark.parametrize("kind", KINDS)
def test_check_rejects(L, kind):
    g = broken(kind, 10)
    assert R.check(g, 10) is not None
    keep = (np.ascontiguousarray(g.row_ptr, np.int64), np.ascontiguousarray(g.tokens, i32), np.ascontiguousarray(g.next, i32))
    c = T.Guide(g.n_states, g.start, *(a.ctypes.data for a in keep))
    import ctypes as C
    assert L.ti_guide_check(C.byref(c), 10) == 1
    assert b"ti_guide_check" in L.ti_last_error()


def test_apply_argument_errors(L):
    g = R.cycle(10, 3)
    lg = np.zeros(10, f32)
    for state, tok in ((3, -1), (-2, -1), (0, -2)):
        with pytest.raises(T.TiError, match="ti error 1: ti_guide_apply"):
            T.guide_apply(g.csr, state, tok, lg)
