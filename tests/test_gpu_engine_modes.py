"""The engine's graph cache across changes of step mode and of what the graphs bake in.

One long-lived engine runs a sequence of calls that move between the greedy, sampled, shared-prefix and penalised
step graphs and the lookahead verify graphs, changing the sampler's parameters, the penalties and the prefix
registration on the way.  Every call must return, bit for bit, what the same call returns on a fresh engine that
has run nothing else: a graph cached under one mode or parameter set and replayed for another gives other tokens
(it does not crash), and this is the test that sees it.

The model is MID of test_gpu_shared_prefix_engine.py (int4 weights, fp16 KV cache), max_batch 4, created under
TI_SHARE_MIN=1 so the 40-token prefix takes the shared attention.  Prompts have 8..12 tokens, every call makes 8.

Most calls of the sequence follow a change that empties the cache (sampler parameters, penalties, registration), so
they pin the drops; steps 2 -> 3 and 6 -> 7 keep rows and mode and change what is baked in or the carry, and steps
12 -> 13 -> 14 change nothing but the mode (a library whose key ignores `sampled` fails at 13).
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_shared_prefix_engine import MODELS, make_engine

pytestmark = pytest.mark.gpu

NAME, N_NEW, B = "MID", 8, 4
PREFIX = MODELS[NAME][2]
A, PARAMS_B = (0.8, 40, 0.95), (1.1, 8, 0.9)   # temperature, top_k, top_p
PEN = (1.3, 0.2, 0.1)


def _inputs():
    rng = np.random.default_rng(20261)
    vocab = MODELS[NAME][0]["vocab"]
    prompts = [rng.integers(0, vocab, size=int(n)).tolist() for n in rng.integers(8, 13, size=6)]
    assert all(8 <= len(p) <= 12 for p in prompts)
    draws = rng.random((8, 6, N_NEW), dtype=np.float32)   # [call][request][token]
    return prompts, draws


def _bits(x):
    """A call's result as nested tuples of plain values and the bytes of its arrays (floats compare bit for bit)."""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, dict):
        return tuple(sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return tuple(_bits(v) for v in x)
    return x


def _sequence():
    """[(name, setup(e), call(e))]: `setup` is the state the call needs and a fresh engine lacks."""
    prompts, draws = _inputs()
    two, four, reqs = prompts[:2], prompts[:4], prompts[:6]
    P = len(PREFIX)
    none = lambda e: None
    pen_on = lambda e: e.set_penalties(*PEN)
    shared = lambda e: e.share_prefix(PREFIX, B)
    return [
        ("1 generate", none, lambda e: e.generate(two, N_NEW)),
        # (four streams: step 3 then asks for the same rows and mode with other sampler parameters)
        ("2 generate_sampled A", none, lambda e: e.generate_sampled(four, N_NEW, *A, draws[0, :4])),
        ("3 serve_sampled B", none, lambda e: e.serve_sampled(reqs, N_NEW, *PARAMS_B, draws[1], eos=-1, chunk=4)),
        ("4 generate_lookahead_sampled A", none,
         lambda e: e.generate_lookahead_sampled(prompts[0], N_NEW, *A, draws[2, 0], k=3)),
        ("5 generate_lookahead", none, lambda e: e.generate_lookahead(prompts[1], N_NEW, k=3)),
        # (four streams again: step 7's graph differs from this one by the carry alone)
        ("6 penalties, generate_sampled A", pen_on, lambda e: e.generate_sampled(four, N_NEW, *A, draws[3, :4])),
        ("7 penalties, serve_sampled A", pen_on,
         lambda e: e.serve_sampled(reqs, N_NEW, *A, draws[4], eos=-1, chunk=4)),
        ("8 penalties off", none, lambda e: e.set_penalties(1.0, 0.0, 0.0)),
        ("9 share_prefix, generate x4", shared, lambda e: e.generate(four, N_NEW, start_pos=[P] * B)),
        ("10 step x4 behind the prefix", shared, lambda e: e.step([p[0] for p in four], [P] * B)),
        ("11 share_prefix(0)", none, lambda e: e.share_prefix([], B)),
        ("12 generate again", none, lambda e: e.generate(two, N_NEW)),
        # nothing is dropped between 12, 13 and 14 (A is still set): two streams greedy, sampled, greedy differ by
        # the key's sampled field alone
        ("13 generate_sampled A behind a greedy graph", none,
         lambda e: e.generate_sampled(two, N_NEW, *A, draws[5, :2])),
        ("14 generate behind a sampled graph", none, lambda e: e.generate(two, N_NEW)),
    ]


def test_each_call_matches_a_fresh_engine(ti, monkeypatch):
    monkeypatch.setenv("TI_SHARE_MIN", "1")
    seq = _sequence()
    long_lived = make_engine(ti, NAME, max_batch=B)
    got = {}
    for name, setup, call in seq:
        setup(long_lived)                      # (a no-op where the sequence has already set that state)
        got[name] = _bits(call(long_lived))
    assert long_lived.shared_prefix() == (0, 0) and long_lived.penalties() == (1.0, 0.0, 0.0)
    long_lived.close()
    assert got["12 generate again"] == got["1 generate"] == got["14 generate behind a sampled graph"]
    for name, setup, call in seq:
        fresh = make_engine(ti, NAME, max_batch=B)
        setup(fresh)
        want = _bits(call(fresh))
        fresh.close()
        assert got[name] == want, f"{name}: the long-lived engine's result differs from a fresh engine's"
