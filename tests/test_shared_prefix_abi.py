"""CPU-side checks of the shared-prefix entry points (ti_attn_decode_shared, ti_attn_shared_workspace_bytes,
ti_engine_share_prefix, ti_engine_shared_prefix): declared, exported and bound, and their host-side argument
checks fail with TI_ERR_ARG and a message naming the function without touching a GPU.  (The engine calls' checks
behind the null engine need an engine, which needs a device: tests/test_gpu_shared_prefix_engine.py.)"""
from __future__ import annotations

import ctypes as C
import os

import pytest

import turboinfer_amd as T
from conftest import ROOT
from test_abi import header_functions

MAX_M = 1024   # TI_ATTN_MAX_M


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(T.LIB_PATH):
        T.build()
    return T.lib()


def test_shared_prefix_symbols_declared_exported_and_bound(L):
    hip = header_functions(os.path.join(ROOT, "include", "ti_hip.h"))
    eng = header_functions(os.path.join(ROOT, "include", "ti_engine.h"))
    for f in ("ti_attn_decode_shared", "ti_attn_shared_workspace_bytes"):
        assert f in hip and f in T.EXPORTED and hasattr(L, f)
    for f in ("ti_engine_share_prefix", "ti_engine_shared_prefix"):
        assert f in eng and f in T.EXPORTED and hasattr(L, f)
    assert L.ti_attn_decode_shared.argtypes is not None and len(L.ti_attn_decode_shared.argtypes) == 16
    assert L.ti_attn_shared_workspace_bytes.restype is C.c_size_t
    assert hasattr(T.Engine, "share_prefix") and hasattr(T.Engine, "shared_prefix")
    with open(os.path.join(ROOT, "include", "ti_hip.h")) as fh:
        assert "#define TI_ATTN_MAX_M %d" % MAX_M in fh.read()


def shared(L, M=4, heads=8, kvh=2, hd=64, P=8, splits=4, packed=0, q=16, k=16, v=16, pos=16, ws=16, out=16, max_seq=64,
           stride=None):
    # (non-null fake pointers: every check fails before anything is launched)
    stride = kvh * max_seq * hd if stride is None else stride
    return L.ti_attn_decode_shared(q, k, v, stride, max_seq, pos, M, heads, kvh, hd, P, splits, packed, ws, out, None)


@pytest.mark.parametrize("kw", [
    dict(M=0), dict(M=MAX_M + 1),                                   # 1 <= M <= TI_ATTN_MAX_M
    dict(hd=96), dict(hd=32), dict(hd=256),                         # head_dim 64 or 128
    dict(heads=6, kvh=2), dict(heads=32, kvh=2), dict(heads=7, kvh=2), dict(kvh=0), dict(heads=0),   # G in {1, 2, 4, 8}
    dict(P=0), dict(P=-1), dict(P=64), dict(P=65), dict(max_seq=0),  # 1 <= prefix_len < max_seq
    dict(splits=0), dict(splits=33),                                # 1 <= splits <= 32
    dict(packed=1, heads=1, kvh=1, hd=64),                          # packed: heads * head_dim % 128 == 0
    dict(stride=0), dict(stride=-8),                                # kv_stream_stride > 0
    dict(q=None), dict(k=None), dict(v=None), dict(pos=None), dict(ws=None), dict(out=None)])
def test_decode_shared_argument_errors_without_launch(L, kw):
    assert shared(L, **kw) == 1, kw
    assert b"ti_attn_decode_shared" in L.ti_last_error()


def test_shared_workspace_bytes(L):
    ws = L.ti_attn_shared_workspace_bytes
    # (16-column blocks x kv-heads) x splits x (16 hd + 32) floats, the largest over the group sizes: 32 heads and
    # 8 streams are 16 blocks x 1 kv-head ... 1 block x 32 kv-heads (MHA), and no group size has more than 32
    assert ws(8, 32, 128, 4) == 4 * 32 * 4 * (16 * 128 + 32)
    assert ws(64, 32, 128, 1) == 4 * 128 * (16 * 128 + 32)
    assert ws(1, 8, 64, 1) >= 4 * 8 * (16 * 64 + 32)              # G = 1: one block per kv-head
    for bad in ((0, 8, 64, 1), (MAX_M + 1, 8, 64, 1), (4, 8, 64, 0), (4, 8, 64, 33), (4, 8, 96, 1), (4, 0, 64, 1)):
        assert ws(*bad) == 0
    for heads, hd in ((8, 64), (32, 128), (4, 128)):
        prev = 0
        for M in (1, 2, 5, 16, 17, 64, 65, MAX_M):
            n = ws(M, heads, hd, 3)
            assert n >= prev > -1 and n > 0
            prev = n
        prev = 0
        for splits in range(1, 33):
            n = ws(17, heads, hd, splits)
            assert n > prev
            prev = n


def test_engine_calls_null_engine(L):
    toks = (C.c_int32 * 4)(1, 2, 3, 4)
    assert L.ti_engine_share_prefix(None, toks, 4, 2) == 1
    assert b"ti_engine_share_prefix" in L.ti_last_error()
    a, b = C.c_int(7), C.c_int(7)
    assert L.ti_engine_shared_prefix(None, C.byref(a), C.byref(b)) == 1
    assert b"ti_engine_shared_prefix" in L.ti_last_error()
