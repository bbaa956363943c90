"""CPU-side checks of the per-request entry points (ti_sample_step_rows, ti_sample_device_rows,
ti_penalty_step_rows, ti_engine_serve_requests): declared and exported, bound by the Python package with 32-byte
mirrors of their two structs, and their host-side argument checks fail with TI_ERR_ARG and a message naming the
function without touching a GPU.  (The checks behind the null engine need an engine, which needs a device:
tests/test_gpu_serve_requests.py.)"""
from __future__ import annotations

import ctypes as C
import os

import pytest

import turboinfer_amd as T
from conftest import ROOT
from test_abi import header_functions

KERNEL = ("ti_sample_step_rows", "ti_sample_device_rows", "ti_penalty_step_rows")
ENGINE = ("ti_engine_serve_requests",)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(T.LIB_PATH):
        T.build()
    return T.lib()


def test_symbols_declared_exported_and_bound(L):
    hip = header_functions(os.path.join(ROOT, "include", "ti_hip.h"))
    eng = header_functions(os.path.join(ROOT, "include", "ti_engine.h"))
    for f in KERNEL:
        assert f in hip, f
    for f in ENGINE:
        assert f in eng, f
    for f in KERNEL + ENGINE:
        assert f in T.EXPORTED and hasattr(L, f), f
        assert getattr(L, f).argtypes is not None, f
    assert hasattr(T.Engine, "serve_requests")


def test_struct_mirrors_are_32_bytes():
    assert C.sizeof(T.RowParams) == C.sizeof(T.RequestParams) == 32
    q = T.RequestParams(max_new=5, top_k=40, temperature=0.5)
    assert (q.max_new, q.stop_token, q.top_k, q.top_p, q.repetition, q.presence, q.frequency) == (5, -1, 40, 1.0, 1.0, 0.0, 0.0)
    r = T.RowParams(0.5, 40, 0.9, 1.0, 0.0, 0.0)
    assert (r.top_k, r.reserved[0], r.reserved[1]) == (40, 0, 0)


def test_serve_requests_null_engine(L):
    out = (C.c_int32 * 4)()
    dr = (C.c_float * 4)()
    offs = (C.c_int32 * 2)(0, 1)
    q = (T.RequestParams * 1)(T.RequestParams(max_new=4))
    assert L.ti_engine_serve_requests(None, 1, out, offs, q, 4, dr, 4, out, out, None) == 1
    assert b"ti_engine_serve_requests" in L.ti_last_error()


def step_rows(L, logits=16, ldl=1024, M=4, V=1024, rows=16, max_k=40, draws=16, stride=8, ctr=16, n_in=16, argmax=16,
              lps=16, ws=None):
    # (non-null fake pointers: every check fails before anything is launched)
    return L.ti_sample_step_rows(logits, ldl, M, V, rows, max_k, draws, stride, ctr, 1, n_in, argmax, lps, ws, None)


def device_rows(L, logits=16, ldl=1024, M=4, V=1024, rows=16, max_k=40, draws=16, tokens=16, lps=16, ws=None):
    return L.ti_sample_device_rows(logits, ldl, M, V, rows, max_k, draws, tokens, lps, ws, None)


COMMON = [dict(logits=None), dict(draws=None), dict(rows=None), dict(M=0), dict(V=0), dict(ldl=1023), dict(max_k=0),
          dict(max_k=1025), dict(V=8192, ldl=8192, max_k=4097)]       # above TI_SAMPLE_MAX_K without a workspace


@pytest.mark.parametrize("kw", COMMON + [dict(stride=0), dict(ctr=None), dict(argmax=None)])
def test_sample_step_rows_argument_errors_without_launch(L, kw):
    assert step_rows(L, **kw) == 1
    assert b"ti_sample_step_rows" in L.ti_last_error()


@pytest.mark.parametrize("kw", COMMON + [dict(tokens=None)])
def test_sample_device_rows_argument_errors_without_launch(L, kw):
    assert device_rows(L, **kw) == 1
    assert b"ti_sample_device_rows" in L.ti_last_error()


def penalty_rows(L, rows=16, null_args=False, **kw):
    f = dict(logits=16, ldl=1024, M=3, V=1024, counts=16, seen=16, n_seen=16, draw_stride=4, ctr=None, out_tokens=None,
             out_stride=0)
    f.update(kw)
    a = T.PenaltyArgs(f["logits"], f["ldl"], f["M"], f["V"], T.PenaltyState(f["counts"], f["seen"], f["n_seen"]),
                      float("nan"), float("nan"), float("nan"),      # (the struct's three values are ignored)
                      f["draw_stride"], 1, f["ctr"], None, f["out_tokens"], f["out_stride"], None)
    return L.ti_penalty_step_rows(None if null_args else C.byref(a), rows, None)


@pytest.mark.parametrize("kw", [dict(null_args=True), dict(rows=None), dict(logits=None), dict(counts=None),
                                dict(seen=None), dict(n_seen=None), dict(ctr=16), dict(M=0), dict(V=0), dict(ldl=1023),
                                dict(draw_stride=0), dict(out_stride=-1)])
def test_penalty_step_rows_argument_errors_without_launch(L, kw):
    assert penalty_rows(L, **kw) == 1
    assert b"ti_penalty_step_rows" in L.ti_last_error()
