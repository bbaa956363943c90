"""The C-ABI of the e4m3 prefill attention on the CPU: ti_attn_prefill_f8 and ti_engine_prefill_attn_name are
declared and exported, and ti_attn_prefill_f8's host-side argument checks answer as ti_attn_prefill's, before
any launch (the pointers are not device memory, so nothing may be launched)."""
from __future__ import annotations

import os

import pytest

import turboinfer_amd as T
from conftest import ROOT

NEW = ["ti_attn_prefill_f8", "ti_engine_prefill_attn_name"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(T.LIB_PATH):
        T.build()
    return T.lib()


def test_symbols_declared_and_exported(L):
    hip = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    eng = open(os.path.join(ROOT, "include", "ti_engine.h")).read()
    for name in NEW:
        assert name + "(" in (eng if name.startswith("ti_engine") else hip), name
        assert name in T.EXPORTED and hasattr(L, name), name
    assert hasattr(T.Engine, "prefill_attn_name")


def _args(**kw):
    a = dict(q=1, k=1, v=1, max_seq=16, pos=1, M=4, heads=4, kv_heads=4, hd=128, out=1)
    a.update(kw)
    return (a["q"], a["k"], a["v"], a["max_seq"], a["pos"], a["M"], a["heads"], a["kv_heads"], a["hd"], a["out"], None)


BAD = [dict(q=None), dict(k=None), dict(v=None), dict(pos=None), dict(out=None), dict(M=0), dict(max_seq=0),
       dict(heads=6, kv_heads=4), dict(hd=96), dict(heads=12, kv_heads=4), dict(heads=32, kv_heads=1)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_argument_errors_match_ti_attn_prefill(L, kw):
    """Each null pointer, M = 0, max_seq = 0, heads 6 over kv_heads 4, head_dim 96, G = 3, G = 32: the same
    non-zero status from both entry points."""
    want, got = L.ti_attn_prefill(*_args(**kw)), L.ti_attn_prefill_f8(*_args(**kw))
    assert want != 0 and got == want, (kw, got, want)
    assert b"ti_attn_prefill_f8" in L.ti_last_error()


def test_the_statuses_themselves(L):
    assert L.ti_attn_prefill_f8(*_args(k=None)) == 1                      # TI_ERR_ARG
    assert L.ti_attn_prefill_f8(*_args(M=0)) == 1
    assert L.ti_attn_prefill_f8(*_args(heads=6, kv_heads=4)) == 1
    assert L.ti_attn_prefill_f8(*_args(hd=96)) == 3                       # TI_ERR_UNSUPPORTED
    assert L.ti_attn_prefill_f8(*_args(heads=12, kv_heads=4)) == 3        # G = 3
    assert L.ti_attn_prefill_f8(*_args(heads=32, kv_heads=1)) == 3        # G = 32


def test_prefill_attn_name_null_engine(L):
    import ctypes as C
    buf = C.create_string_buffer(64)
    assert L.ti_engine_prefill_attn_name(None, 16, buf, 64) == 1
    assert b"ti_engine_prefill_attn_name" in L.ti_last_error()
