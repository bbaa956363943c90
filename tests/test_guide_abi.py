"""CPU-side checks of the guide entry points (ti_guide_reset, ti_guide_step, ti_guide_check, ti_guide_apply,
ti_engine_set_guide, ti_engine_guide_states): declared and exported, bound by the Python package with argtypes, the
ctypes structs laid out as the headers', and the host-side argument checks failing with status 1 and a message
naming the function without touching a GPU."""
from __future__ import annotations

import ctypes as C
import os

import pytest

import turboinfer_amd as T
from conftest import ROOT
from test_abi import header_functions

HIP = ("ti_guide_reset", "ti_guide_step")
ENGINE = ("ti_engine_set_guide", "ti_engine_guide_states", "ti_guide_check", "ti_guide_apply")


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
    assert hasattr(T.Engine, "set_guide") and hasattr(T.Engine, "guide_states")
    assert hasattr(T, "guide_apply") and hasattr(T, "guide_check")
    assert {n for n, _ in T.GuideArgs._fields_} >= {"logits", "guide", "state", "draw_stride", "out_tokens", "carry"}


def test_structs_match_the_header_layout():
    # ti_guide: 2 int32 | 3 pointers
    assert C.sizeof(T.Guide) == 32 and T.Guide.row_ptr.offset == 8
    # ti_guide_dev: 2 int32 | 4 pointers
    assert C.sizeof(T.GuideDev) == 40 and T.GuideDev.mask.offset == 32
    # ti_guide_args: float* + 3 int32 (+ pad) | ti_guide_dev | pointer | 2 int32 | 3 pointers | int32 (+ pad) | pointer
    assert T.GuideArgs.guide.offset == 24 and T.GuideArgs.state.offset == 64
    assert T.GuideArgs.draw_stride.offset == 72 and T.GuideArgs.step_ctr.offset == 80
    assert T.GuideArgs.out_stride.offset == 104 and T.GuideArgs.carry.offset == 112
    assert C.sizeof(T.GuideArgs) == 120


def test_engine_entry_points_null_engine(L):
    assert L.ti_engine_set_guide(None, None) == 1
    assert b"ti_engine_set_guide" in L.ti_last_error()
    assert L.ti_engine_guide_states(None, None) == 1
    assert b"ti_engine_guide_states" in L.ti_last_error()


def step(L, args=True, logits=16, row_ptr=16, tokens=16, nxt=16, mask=16, state=16, out_tokens=16, step_ctr=16, M=2,
         V=1000, ldl=1000, n_states=3, mask_words=32, draw_stride=4, out_stride=8):
    # (non-null fake pointers: every check fails before anything is launched)
    a = T.GuideArgs(logits, ldl, M, V, T.GuideDev(n_states, mask_words, row_ptr, tokens, nxt, mask), state, draw_stride,
                    1, step_ctr, 16, out_tokens, out_stride, None)
    return L.ti_guide_step(C.byref(a) if args else None, None)


@pytest.mark.parametrize("kw", [dict(args=False), dict(logits=None), dict(row_ptr=None), dict(tokens=None),
                                dict(nxt=None), dict(mask=None), dict(state=None), dict(out_tokens=None), dict(M=0),
                                dict(V=0), dict(ldl=999), dict(n_states=0), dict(mask_words=31), dict(mask_words=33),
                                dict(draw_stride=0), dict(out_stride=-1)])
def test_guide_step_argument_errors_without_launch(L, kw):
    assert step(L, **kw) == 1
    assert b"ti_guide_step" in L.ti_last_error()


@pytest.mark.parametrize("kw", [dict(state=None), dict(first=-1), dict(count=0), dict(value=-2)])
def test_guide_reset_argument_errors_without_launch(L, kw):
    d = dict(state=16, first=0, count=1, value=0)
    d.update(kw)
    assert L.ti_guide_reset(d["state"], d["first"], d["count"], d["value"], None) == 1
    assert b"ti_guide_reset" in L.ti_last_error()
