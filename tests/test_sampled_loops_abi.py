"""CPU-side checks of the sampled device loops' entry points (ti_lookahead_sample,
ti_engine_generate_lookahead_sampled, ti_engine_serve_sampled): declared and exported, bound by the Python
package, and their host-side argument checks fail with their status and a message naming the function without
touching a GPU.  (The checks behind the null engine need an engine, which needs a device:
tests/test_gpu_lookahead_sampled_engine.py, tests/test_gpu_serve_sampled.py.)"""
from __future__ import annotations

import ctypes as C
import os

import pytest

import turboinfer_amd as T
from conftest import ROOT
from test_abi import header_functions

NEW_ENGINE = ("ti_engine_generate_lookahead_sampled", "ti_engine_serve_sampled")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(T.LIB_PATH):
        T.build()
    return T.lib()


def test_symbols_declared_exported_and_bound(L):
    assert "ti_lookahead_sample" in header_functions(os.path.join(ROOT, "include", "ti_hip.h"))
    eng = header_functions(os.path.join(ROOT, "include", "ti_engine.h"))
    for f in ("ti_lookahead_sample",) + NEW_ENGINE:
        assert f in T.EXPORTED and hasattr(L, f), f
        assert getattr(L, f).argtypes is not None, f
    for f in NEW_ENGINE:
        assert f in eng, f
    assert hasattr(T.Engine, "generate_lookahead_sampled") and hasattr(T.Engine, "serve_sampled")


def test_engine_entry_points_null_arguments(L):
    out = (C.c_int32 * 4)()
    dr = (C.c_float * 4)()
    assert L.ti_engine_generate_lookahead_sampled(None, 0, out, 1, 0, None, 0, 4, 3, 4, 1.0, 2, 1.0, dr, out, None,
                                                  None) == 1
    assert b"ti_engine_generate_lookahead_sampled" in L.ti_last_error()
    offs = (C.c_int32 * 2)(0, 1)
    assert L.ti_engine_serve_sampled(None, 1, out, offs, 4, 2, 4, 1.0, 2, 1.0, dr, out, out, None) == 1
    assert b"ti_engine_serve_sampled" in L.ti_last_error()


def la_sample(L, logits=16, ldl=1024, R=4, V=1024, T_=1.0, k=2, p=1.0, draws=16, cap=8, state=16, cfg=16, argmax=16,
              lps=16, ws=None):
    # (non-null fake pointers: every check fails before anything is launched)
    return L.ti_lookahead_sample(logits, ldl, R, V, T_, k, p, draws, cap, state, cfg, argmax, lps, ws, None)


@pytest.mark.parametrize("kw", [dict(logits=None), dict(draws=None), dict(state=None), dict(cfg=None), dict(argmax=None),
                                dict(R=0), dict(R=17), dict(V=0), dict(ldl=1023), dict(cap=0), dict(k=0), dict(k=1025),
                                dict(V=8192, ldl=8192, k=4097)])           # above TI_SAMPLE_MAX_K without a workspace
def test_lookahead_sample_argument_errors_without_launch(L, kw):
    assert la_sample(L, **kw) == 1
    assert b"ti_" in L.ti_last_error()
