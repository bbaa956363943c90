"""CPU-side checks of the penalty entry points (ti_penalty_reset, ti_penalty_step, ti_penalize_logits,
ti_engine_set_penalties, ti_engine_get_penalties): declared and exported, bound by the Python package with
argtypes, and their host-side argument checks fail with status 1 and a message naming the function without
touching a GPU.  (What lies behind the null engine needs a device: tests/test_gpu_penalty_engine.py.)"""
from __future__ import annotations

import ctypes as C
import os

import pytest

import turboinfer_amd as T
from conftest import ROOT
from test_abi import header_functions

HIP = ("ti_penalty_reset", "ti_penalty_step")
ENGINE = ("ti_engine_set_penalties", "ti_engine_get_penalties", "ti_penalize_logits")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(T.LIB_PATH):
        T.build()
    return T.lib()


def test_symbols_declared_exported_and_bound(L):
    hip = header_functions(os.path.join(ROOT, "include", "ti_hip.h"))
    eng = header_functions(os.path.join(ROOT, "include", "ti_engine.h"))
    for f in HIP:
        assert f in hip, f
    for f in ENGINE:
        assert f in eng, f
    for f in HIP + ENGINE:
        assert f in T.EXPORTED and hasattr(L, f), f
        assert getattr(L, f).argtypes is not None, f
    assert hasattr(T.Engine, "set_penalties") and hasattr(T.Engine, "penalties") and hasattr(T, "penalize_logits")
    assert {n for n, _ in T.PenaltyArgs._fields_} >= {"logits", "state", "repetition", "presence", "frequency", "carry"}


def test_args_struct_matches_the_header_layout():
    # float* + 3 int32 (+ pad) | 3 pointers | 3 floats + 2 int32 (+ pad) | 3 pointers | int32 (+ pad) | pointer
    assert C.sizeof(T.PenaltyState) == 24
    assert T.PenaltyArgs.state.offset == 24 and T.PenaltyArgs.repetition.offset == 48
    assert T.PenaltyArgs.step_ctr.offset == 72 and T.PenaltyArgs.carry.offset == 104
    assert C.sizeof(T.PenaltyArgs) == 112


def test_engine_entry_points_null_engine(L):
    assert L.ti_engine_set_penalties(None, 1.1, 0.0, 0.0) == 1
    assert b"ti_engine_set_penalties" in L.ti_last_error()
    r = C.c_float()
    assert L.ti_engine_get_penalties(None, C.byref(r), None, None) == 1
    assert b"ti_engine_get_penalties" in L.ti_last_error()


def step(L, args=True, logits=16, counts=16, seen=16, n_seen=16, out_tokens=16, step_ctr=16, M=2, V=1000, ldl=1000,
         draw_stride=4, out_stride=8, rep=1.1, pres=0.0, freq=0.0):
    # (non-null fake pointers: every check fails before anything is launched)
    a = T.PenaltyArgs(logits, ldl, M, V, T.PenaltyState(counts, seen, n_seen), rep, pres, freq, draw_stride, 1, step_ctr,
                      16, out_tokens, out_stride, None)
    return L.ti_penalty_step(C.byref(a) if args else None, None)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("kw", [dict(args=False), dict(logits=None), dict(counts=None), dict(seen=None),
                                dict(n_seen=None), dict(out_tokens=None), dict(M=0), dict(V=0), dict(ldl=999),
                                dict(draw_stride=0), dict(rep=0.0), dict(rep=-2.0), dict(rep=INF), dict(rep=NAN),
                                dict(pres=INF), dict(pres=NAN), dict(freq=-INF), dict(freq=NAN)])
def test_penalty_step_argument_errors_without_launch(L, kw):
    assert step(L, **kw) == 1
    assert b"ti_penalty_step" in L.ti_last_error()


@pytest.mark.parametrize("kw", [dict(st=False), dict(counts=None), dict(seen=None), dict(n_seen=None), dict(V=0),
                                dict(m=-1), dict(n=-1), dict(tokens=None, n=3)])
def test_penalty_reset_argument_errors_without_launch(L, kw):
    d = dict(st=True, counts=16, seen=16, n_seen=16, V=1000, m=0, tokens=16, n=3)
    d.update(kw)
    st = T.PenaltyState(d["counts"], d["seen"], d["n_seen"])
    assert L.ti_penalty_reset(C.byref(st) if d["st"] else None, d["V"], d["m"], d["tokens"], d["n"], None) == 1
    assert b"ti_penalty_reset" in L.ti_last_error()
