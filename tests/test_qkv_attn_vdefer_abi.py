"""CPU-side checks of ti_qkv_attn_v_deferred (the v tile deferred into the attention loop): the
symbol is declared and exported, it answers 1 only for the head_dim-128 instances, and its knob TI_QA_VDEFER is
read once per process -- a value set after the first call changes nothing, a fresh process sees it.  No GPU is
touched: the function only reports which instance a launch would take."""
from __future__ import annotations

import os
import subprocess
import sys

import pytest

import turboinfer_amd as T
from conftest import ROOT
from test_abi import header_functions

CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import turboinfer_amd as T
L = T.lib()
print(",".join(str(L.ti_qkv_attn_v_deferred(b, hd)) for b, hd in ((4, 128), (8, 128), (4, 64), (8, 64), (16, 128))))
"""


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(T.LIB_PATH):
        T.build()
    return T.lib()


def child(value):
    env = {k: v for k, v in os.environ.items() if k != "TI_QA_VDEFER"}
    if value is not None:
        env["TI_QA_VDEFER"] = value
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [int(x) for x in r.stdout.strip().split(",")]


def test_symbol_declared_and_exported(L):
    assert "ti_qkv_attn_v_deferred" in header_functions(os.path.join(ROOT, "include", "ti_hip.h"))
    assert "ti_qkv_attn_v_deferred" in T.EXPORTED and hasattr(L, "ti_qkv_attn_v_deferred")


def test_default_and_knob_in_fresh_processes():
    assert child(None) == [1, 1, 0, 0, 0]     # head_dim 128 at 4 and 8 bits only
    assert child("0") == [0, 0, 0, 0, 0]      # the old order everywhere
    assert child("1") == [1, 1, 0, 0, 0]


def test_knob_is_read_once(L, monkeypatch):
    first = [L.ti_qkv_attn_v_deferred(4, 128), L.ti_qkv_attn_v_deferred(8, 128)]
    assert first[0] == first[1] and first[0] in (0, 1)
    assert L.ti_qkv_attn_v_deferred(4, 64) == 0 and L.ti_qkv_attn_v_deferred(16, 128) == 0
    for v in ("0", "1"):   # (os.environ writes through to the C environment: getenv would see it)
        monkeypatch.setenv("TI_QA_VDEFER", v)
        assert [L.ti_qkv_attn_v_deferred(4, 128), L.ti_qkv_attn_v_deferred(8, 128)] == first
