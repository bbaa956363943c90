"""CPU-side checks of the scoring entry points (ti_logprob_rows, ti_engine_score): both are
exported and declared, and their host-side argument checks fail with TI_ERR_ARG and a message
naming the function without touching a GPU."""
from __future__ import annotations

import os

import pytest

import turboinfer_amd as T
from conftest import ROOT
from test_abi import header_functions


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(T.LIB_PATH):
        T.build()
    return T.lib()


def test_scoring_symbols_declared_and_exported(L):
    assert "ti_logprob_rows" in header_functions(os.path.join(ROOT, "include", "ti_hip.h"))
    assert "ti_engine_score" in header_functions(os.path.join(ROOT, "include", "ti_engine.h"))
    for f in ("ti_logprob_rows", "ti_engine_score"):
        assert f in T.EXPORTED and hasattr(L, f)


def test_engine_score_null_engine(L):
    rc = L.ti_engine_score(None, 0, None, 1, 0, None, None, None)
    assert rc == 1 and b"ti_engine_score" in L.ti_last_error()


def test_logprob_rows_argument_errors_without_launch(L):
    # (non-null fake pointers: every check below fails before anything is launched)
    assert L.ti_logprob_rows(16, 32, 0, 32, 16, 16, None, None) == 1     # rows = 0
    assert b"ti_logprob_rows" in L.ti_last_error()
    assert L.ti_logprob_rows(16, 31, 1, 32, 16, 16, None, None) == 1     # ld < vocab
    assert b"ti_logprob_rows" in L.ti_last_error()
    assert L.ti_logprob_rows(16, 32, 1, 0, 16, 16, None, None) == 1      # vocab = 0
    assert L.ti_logprob_rows(None, 32, 1, 32, 16, 16, None, None) == 1   # null logits
    assert L.ti_logprob_rows(16, 32, 1, 32, None, 16, None, None) == 1   # null targets
    assert L.ti_logprob_rows(16, 32, 1, 32, 16, None, None, None) == 1   # null out_logprob
