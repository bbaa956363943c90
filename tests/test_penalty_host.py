"""ti_penalize_logits, the host form of the device loops' penalties, against the NumPy float32 restatement
(tests/penalty_ref.py), bit for bit: every parameter set over every context kind at both vocabulary sizes, the
planted zeros / huge values / subnormal on counted tokens, uncounted tokens and the neutral values untouched,
and the argument errors.  No GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import penalty_ref as R


@pytest.fixture(scope="module")
def L(ti_host):
    return ti_host.lib()


@pytest.mark.parametrize("V", R.VOCABS)
@pytest.mark.parametrize("kind", R.CONTEXT_KINDS)
@pytest.mark.parametrize("params", R.PARAMS, ids=lambda p: "r%g_p%g_f%g" % p)
def test_matches_the_numpy_restatement_bit_for_bit(ti_host, V, kind, params):
    ctx = R.context(kind, V)
    lg = R.logits_for(ctx, V)
    ids = np.unique(ctx)
    # the planted values sit on counted tokens (as many as the context has distinct ids)
    assert np.array_equal(R.bits(lg[ids[: R.PLANTED.size]]), R.bits(R.PLANTED[: ids.size]))
    got = ti_host.penalize_logits(lg, ctx, *params)
    ref = R.penalize(lg, ctx, *params)
    assert got.dtype == np.float32 and got.shape == (V,)
    assert np.array_equal(R.bits(got), R.bits(ref)), np.flatnonzero(R.bits(got) != R.bits(ref))[:8]
    off = np.ones(V, bool)
    off[ids] = False
    assert np.array_equal(R.bits(got[off]), R.bits(lg[off])), "a token with count 0 changed"
    if ids.size > R.PLANTED.size:   # (every parameter set moves a counted N(0, 4) logit: not the identity)
        assert not np.array_equal(R.bits(ref[ids]), R.bits(lg[ids]))


@pytest.mark.parametrize("V", R.VOCABS)
@pytest.mark.parametrize("kind", R.CONTEXT_KINDS)
def test_neutral_values_leave_every_bit(ti_host, V, kind):
    ctx = R.context(kind, V)
    lg = R.logits_for(ctx, V)
    lg[: 3] = [np.nan, np.inf, -np.inf]   # "off", not "apply the identity": even these keep their bits
    got = ti_host.penalize_logits(lg, ctx, 1.0, 0.0, 0.0)
    assert np.array_equal(R.bits(got), R.bits(lg))


def test_ids_outside_the_vocabulary_are_ignored(ti_host):
    V = 1000
    ctx = np.array([5, -1, V, 5, 2 ** 31 - 1, 7], np.int32)
    lg = R.logits_for(ctx[(ctx >= 0) & (ctx < V)], V)
    got = ti_host.penalize_logits(lg, ctx, 1.1, 0.4, 0.2)
    assert np.array_equal(R.bits(got), R.bits(R.penalize(lg, [5, 5, 7], 1.1, 0.4, 0.2)))


def call(L, logits=True, V=8, ctx=True, n=2, rep=1.1, pres=0.0, freq=0.0):
    lg = (C.c_float * 8)()
    cx = (C.c_int32 * 4)(1, 2, 3, 4)
    return L.ti_penalize_logits(lg if logits else None, V, cx if ctx else None, n, rep, pres, freq)


@pytest.mark.parametrize("kw", [dict(logits=False), dict(V=0), dict(n=-1), dict(ctx=False, n=1), dict(rep=0.0),
                                dict(rep=-1.0), dict(rep=float("inf")), dict(rep=float("nan")),
                                dict(pres=float("inf")), dict(pres=float("nan")), dict(freq=-float("inf")),
                                dict(freq=float("nan"))])
def test_argument_errors(L, kw):
    assert call(L, **kw) == 1
    assert b"ti_penalize_logits" in L.ti_last_error()


def test_empty_context_with_a_null_pointer_is_fine(L):
    assert call(L, ctx=False, n=0) == 0
