"""CPU-side checks of the lookahead entry points (ti_attn_prefill_split, ti_lookahead_begin / _accept,
ti_engine_generate_lookahead): declared and exported, and their host-side argument checks fail with their
status and a message naming the function without touching a GPU.  (The engine entry's checks behind the null
engine need an engine, which needs a device: tests/test_gpu_lookahead_engine.py.)"""
from __future__ import annotations

import ctypes as C
import os

import pytest

import turboinfer_amd as T
from conftest import ROOT
from test_abi import header_functions

NEW_HIP = ("ti_attn_prefill_split", "ti_attn_prefill_split_workspace_bytes", "ti_lookahead_begin", "ti_lookahead_accept")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(T.LIB_PATH):
        T.build()
    return T.lib()


def test_lookahead_symbols_declared_and_exported(L):
    hip = header_functions(os.path.join(ROOT, "include", "ti_hip.h"))
    for f in NEW_HIP:
        assert f in hip and f in T.EXPORTED and hasattr(L, f)
    assert "ti_engine_generate_lookahead" in header_functions(os.path.join(ROOT, "include", "ti_engine.h"))
    assert "ti_engine_generate_lookahead" in T.EXPORTED and hasattr(L, "ti_engine_generate_lookahead")
    assert hasattr(T.Engine, "generate_lookahead")


def test_generate_lookahead_null_arguments(L):
    out = (C.c_int32 * 4)()
    assert L.ti_engine_generate_lookahead(None, 0, out, 1, 0, None, 0, 4, 3, 4, out, None) == 1
    assert b"ti_engine_generate_lookahead" in L.ti_last_error()


def split(L, M=4, heads=8, kvh=2, hd=64, splits=4, q=16, k=16, v=16, pos=16, ws=16, out=16, max_seq=64):
    # (non-null fake pointers: every check fails before anything is launched)
    return L.ti_attn_prefill_split(q, k, v, max_seq, pos, M, heads, kvh, hd, splits, ws, out, None)


@pytest.mark.parametrize("kw", [dict(M=0), dict(M=17), dict(splits=0), dict(splits=33), dict(heads=7), dict(kvh=0),
                                dict(max_seq=0), dict(q=None), dict(k=None), dict(v=None), dict(pos=None),
                                dict(ws=None), dict(out=None)])
def test_prefill_split_argument_errors_without_launch(L, kw):
    assert split(L, **kw) == 1
    assert b"ti_attn_prefill_split" in L.ti_last_error()


def test_prefill_split_unsupported_shapes_as_ti_attn_prefill(L):
    for kw in (dict(hd=96), dict(heads=6, kvh=2), dict(heads=64, kvh=2)):     # head_dim, G = 3, G = 32
        assert split(L, **kw) == 3 and b"ti_attn_prefill_split" in L.ti_last_error()
        a = dict(M=4, heads=8, kvh=2, hd=64)
        a.update(kw)
        assert L.ti_attn_prefill(16, 16, 16, 64, 16, a["M"], a["heads"], a["kvh"], a["hd"], 16, None) == 3


def test_prefill_split_workspace_bytes(L):
    ws = L.ti_attn_prefill_split_workspace_bytes
    # tickets (heads rounded up to 64 words), then (query blocks x kv-heads) x splits x (16 hd + 32) floats:
    # 32 heads, 8 rows: MHA has 32 blocks, and no group size has more
    assert ws(8, 32, 128, 4) == 4 * (64 + 32 * 4 * (16 * 128 + 32))
    assert ws(16, 8, 64, 32) == 4 * (64 + 8 * 32 * (16 * 64 + 32))
    assert ws(1, 8, 64, 1) >= 4 * (64 + 8 * (16 * 64 + 32))       # G = 1: one block per kv-head
    for bad in ((0, 8, 64, 1), (17, 8, 64, 1), (4, 8, 64, 0), (4, 8, 64, 33), (4, 8, 96, 1), (4, 0, 64, 1)):
        assert ws(*bad) == 0


def la_args(**kw):
    a = T.LookaheadArgs(state=16, cfg=16, hist=16, k=4, hidden=64, vocab=32, max_pos=63, emb=16, h=16, row_tok=16,
                        pos=16, argmax=16, out_tokens=16)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("fn", ["ti_lookahead_begin", "ti_lookahead_accept"])
def test_lookahead_kernels_argument_errors_without_launch(L, fn):
    f = getattr(L, fn)
    assert f(None, None) == 1 and fn.encode() in L.ti_last_error()
    for kw in (dict(k=0), dict(k=16), dict(hidden=0), dict(vocab=0), dict(max_pos=-1), dict(state=None),
               dict(cfg=None), dict(hist=None), dict(emb=None), dict(h=None), dict(row_tok=None), dict(pos=None),
               dict(argmax=None), dict(out_tokens=None)):
        a = la_args(**kw)
        assert f(C.byref(a), None) == 1, kw
        assert fn.encode() in L.ti_last_error()
