"""CPU-side checks of the per-request guide entry points (ti_guide_step_rows, ti_engine_add_guide,
ti_engine_remove_guide, ti_engine_guide_count, ti_engine_serve_requests_guided): declared with the argument types of
the headers and exported, bound by the Python package, ti_row_params still 32 bytes with the guide handle in
reserved[0] at offset 24, TI_GUIDE_CAP the same in the binding and the header, and the host-side argument checks
failing with status 1 and a message naming the function without touching a GPU."""
from __future__ import annotations

import ctypes as C
import os
import re

import pytest

import turboinfer_amd as T
from conftest import ROOT
from test_abi import header_functions

HIP = ("ti_guide_step_rows",)
ENGINE = ("ti_engine_add_guide", "ti_engine_remove_guide", "ti_engine_guide_count", "ti_engine_serve_requests_guided")
vp, i32 = C.c_void_p, C.c_int
ARGTYPES = {
    "ti_guide_step_rows": [C.POINTER(T.GuideArgs), vp, i32, vp, vp],
    "ti_engine_add_guide": [vp, C.POINTER(T.Guide), C.POINTER(C.c_int)],
    "ti_engine_remove_guide": [vp, i32],
    "ti_engine_guide_count": [vp, C.POINTER(C.c_int)],
    "ti_engine_serve_requests_guided": [vp, i32, vp, vp, C.POINTER(T.RequestParams), vp, i32, vp, i32, vp, vp, vp],
}
# the parameter lists as the headers declare them (types only, one per argument)
DECLARED = {
    "ti_guide_step_rows": ["const ti_guide_args*", "const ti_guide_dev*", "int", "const ti_row_params*", "ti_stream_t"],
    "ti_engine_add_guide": ["ti_engine*", "const ti_guide*", "int*"],
    "ti_engine_remove_guide": ["ti_engine*", "int"],
    "ti_engine_guide_count": ["ti_engine*", "int*"],
    "ti_engine_serve_requests_guided": ["ti_engine*", "int", "const int32_t*", "const int32_t*", "const ti_request_params*",
                                        "const int32_t*", "int", "const float*", "int", "int32_t*", "int32_t*", "float*"],
}


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(T.LIB_PATH):
        T.build()
    return T.lib()


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_types(src, fn):
    m = re.search(r"\bint\s+" + fn + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{fn} is not declared"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())) for a in m.group(1).split(",")]


def test_symbols_declared_exported_and_bound(L):
    hip = header_functions(os.path.join(ROOT, "include", "ti_hip.h"))
    eng = header_functions(os.path.join(ROOT, "include", "ti_engine.h"))
    for f in HIP:
        assert f in hip, f
        assert declared_types(header("ti_hip.h"), f) == DECLARED[f], f
    for f in ENGINE:
        assert f in eng, f
        assert declared_types(header("ti_engine.h"), f) == DECLARED[f], f
    for f in HIP + ENGINE:
        assert f in T.EXPORTED and hasattr(L, f), f
        assert list(getattr(L, f).argtypes) == ARGTYPES[f], f
    for m in ("add_guide", "remove_guide", "guide_count"):
        assert hasattr(T.Engine, m), m
    assert hasattr(T, "guide_step_rows")
    assert "guides" in T.Engine.serve_requests.__code__.co_varnames


def test_row_params_keeps_its_layout():
    assert C.sizeof(T.RowParams) == 32 and T.RowParams.reserved.offset == 24
    assert C.sizeof(T.RequestParams) == 32
    r = T.RowParams(0.5, 40, 0.9, 1.0, 0.0, 0.0, (3, 0))
    assert (r.reserved[0], r.reserved[1]) == (3, 0)
    src = header("ti_hip.h")
    body = re.search(r"typedef struct ti_row_params \{(.*?)\} ti_row_params;", src, flags=re.S).group(1)
    assert [" ".join(x.split()) for x in body.split(";") if x.strip()] == [
        "float temperature", "int32_t top_k", "float top_p", "float repetition, presence, frequency", "int32_t reserved[2]"]


def test_guide_cap_matches_the_header():
    m = re.search(r"^#define\s+TI_GUIDE_CAP\s+(\d+)\s*$", header("ti_engine.h"), flags=re.M)
    assert m and int(m.group(1)) == T.GUIDE_CAP and T.GUIDE_CAP >= 1


def test_engine_entry_points_null_engine(L):
    h, n = C.c_int(7), C.c_int(7)
    g = T.Guide()
    assert L.ti_engine_add_guide(None, C.byref(g), C.byref(h)) == 1
    assert b"ti_engine_add_guide" in L.ti_last_error() and h.value == 7
    assert L.ti_engine_remove_guide(None, 0) == 1
    assert b"ti_engine_remove_guide" in L.ti_last_error()
    assert L.ti_engine_guide_count(None, C.byref(n)) == 1
    assert b"ti_engine_guide_count" in L.ti_last_error() and n.value == 7
    out = (C.c_int32 * 4)()
    dr = (C.c_float * 4)()
    offs = (C.c_int32 * 2)(0, 1)
    q = (T.RequestParams * 1)(T.RequestParams(max_new=4))
    gh = (C.c_int32 * 1)(0)
    assert L.ti_engine_serve_requests_guided(None, 1, out, offs, q, gh, 4, dr, 4, out, out, None) == 1
    assert b"ti_engine_serve_requests_guided" in L.ti_last_error()


def step_rows(L, args=True, logits=16, state=16, out_tokens=16, step_ctr=16, guides=16, cap=4, rows=16, M=2, V=1000,
              ldl=1000, draw_stride=4, out_stride=8):
    # (non-null fake pointers: every check fails before anything is launched; a->guide is all-zero and ignored)
    a = T.GuideArgs(logits, ldl, M, V, T.GuideDev(), state, draw_stride, 1, step_ctr, 16, out_tokens, out_stride, None)
    return L.ti_guide_step_rows(C.byref(a) if args else None, guides, cap, rows, None)


@pytest.mark.parametrize("kw", [dict(args=False), dict(logits=None), dict(state=None), dict(out_tokens=None),
                                dict(guides=None), dict(rows=None), dict(cap=0), dict(cap=-1), dict(M=0), dict(V=0),
                                dict(ldl=999), dict(draw_stride=0), dict(out_stride=-1)])
def test_guide_step_rows_argument_errors_without_launch(L, kw):
    assert step_rows(L, **kw) == 1
    assert b"ti_guide_step_rows" in L.ti_last_error()
