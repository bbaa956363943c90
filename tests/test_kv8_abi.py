"""The C-ABI of the 8-bit (e4m3) KV cache on the CPU: its symbols are declared and exported, and the
host-side argument checks of the new entry points answer as those of their fp16 twins, before any launch."""
from __future__ import annotations

import ctypes as C
import os

import pytest

import turboinfer_amd as T
from conftest import ROOT

NEW = ["ti_attn_decode_f8", "ti_attn_decode_packed_f8", "ti_attn_decode_partials_f8", "ti_fill_kv_uniform_f8",
       "ti_engine_read_kv"]


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
    assert "#define TI_BITS_KV8 128" in hip and T.BITS_KV8 == 128
    assert "kv_fp8" in hip and "kv_fp8" in [f[0] for f in T.Epilogue._fields_]
    assert T.Epilogue._fields_[-1][0] == "kv_fp8"          # the trailing field
    assert L.ti_epilogue_bytes() == C.sizeof(T.Epilogue)


def _attn_args(**kw):
    a = dict(q=1, k=1, v=1, stride=1 << 20, max_seq=16, pos=1, M=1, heads=4, kv_heads=4, hd=128, splits=1, ws=1, out=1)
    a.update(kw)
    return (a["q"], a["k"], a["v"], a["stride"], a["max_seq"], a["pos"], a["M"], a["heads"], a["kv_heads"], a["hd"],
            a["splits"], a["ws"], a["out"], None)


BAD = [dict(q=None), dict(k=None), dict(v=None), dict(pos=None), dict(out=None), dict(ws=None), dict(hd=96),
       dict(stride=4 * 16 * 128 - 8), dict(M=0), dict(M=1025), dict(heads=6),
       dict(splits=0), dict(max_seq=0), dict(heads=12)]


@pytest.mark.parametrize("pair", [("ti_attn_decode", "ti_attn_decode_f8"),
                                  ("ti_attn_decode_packed", "ti_attn_decode_packed_f8"),
                                  ("ti_attn_decode_partials", "ti_attn_decode_partials_f8")])
def test_argument_errors_match_the_fp16_entry_points(L, pair):
    """Null pointers, bad head_dim, too-small stride, bad sizes, an unsupported group: the same status from
    both, and never TI_OK (nothing is launched: the pointers are not device memory)."""
    f16_fn, f8_fn = getattr(L, pair[0]), getattr(L, pair[1])
    partials = pair[0].endswith("partials")
    for kw in BAD:
        kw = dict(kw)
        if partials:
            kw.setdefault("splits", 2)
        a = _attn_args(**kw)
        want, got = f16_fn(*a), f8_fn(*a)
        assert want != 0, kw
        assert got == want, (pair, kw, got, want)
    # the statuses themselves
    assert f8_fn(*_attn_args(k=None, splits=2)) == 1
    assert f8_fn(*_attn_args(hd=96, splits=2)) == 3
    assert f8_fn(*_attn_args(stride=4 * 16 * 128 - 8, splits=2)) == 1 and b"kv_stream_stride" in L.ti_last_error()
    if partials:
        assert f8_fn(*_attn_args(splits=1)) == 1 and f8_fn(*_attn_args(splits=9)) == 1
    if pair[0].endswith("packed"):
        assert f8_fn(*_attn_args(heads=1, kv_heads=1, hd=64)) == 1      # heads * head_dim not a multiple of 128


def test_fill_and_read_kv_argument_errors(L):
    assert L.ti_fill_kv_uniform_f8(1, 0, 4, 2, 64, 16, None, None) == 1
    assert L.ti_fill_kv_uniform_f8(1, 0, 17, 2, 64, 16, 1, None) == 1          # n > max_seq
    assert L.ti_fill_kv_uniform(1, 0, 17, 2, 64, 16, 1, None) == 1
    assert L.ti_engine_read_kv(None, 0, 0, 0, 0, 1, 1) == 1 and b"ti_engine_read_kv" in L.ti_last_error()


def test_engine_config_rejects_kv8_on_compat(L):
    """TI_BITS_KV8 with compat = 1: TI_ERR_ARG from the configuration check (a compat engine has no KV cache)."""
    cfg = T.EngineConfig(1024, 256, 2, 4, 4, 64, 512, 1e4, 1e-5, 16 | T.BITS_KV8, 64, 1, 1, 0, 0)
    h = C.c_void_p()
    assert L.ti_engine_create(C.byref(cfg), C.byref(h)) == 1 and b"TI_BITS_KV8" in L.ti_last_error()
    # the flag alone is no weight format
    cfg = T.EngineConfig(1024, 256, 2, 4, 4, 64, 512, 1e4, 1e-5, T.BITS_KV8, 64, 1, 0, 0, 0)
    assert L.ti_engine_create(C.byref(cfg), C.byref(h)) == 1 and b"bits" in L.ti_last_error()
    # a QKV epilogue with a kv_fp8 other than 0 / 1
    ep = T.Epilogue()
    ep.kind, ep.ldo, ep.out, ep.q_dim, ep.kv_dim, ep.head_dim, ep.max_seq = T.EPI_QKV_ROPE_KV, 256, 1, 256, 128, 64, 16
    ep.pos, ep.rope_cs, ep.k_cache, ep.v_cache, ep.kv_fp8 = 1, 1, 1, 1, 2
    rc = L.ti_gemm_wq_a16(1, 1, 4, 1, T.X_F16, 512, None, 1e-5, 1, 512, 512, C.byref(ep), None)
    assert rc == 1 and b"kv_fp8" in L.ti_last_error()
