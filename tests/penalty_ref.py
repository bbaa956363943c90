"""NumPy float32 restatement of the repetition / presence / frequency penalties (ti_hip.h ti_penalty_step,
ti_engine.h ti_penalize_logits; llama.cpp's llama_sampler_penalties_apply with penalty_last_n = -1), and the
shared inputs of the penalty tests.

For every token v with count[v] > 0 in the context, four operations, each rounded once to float32:
    a   = l <= 0 ? l * repetition : l / repetition
    b   = float(count) * frequency
    d   = b + presence
    out = a - d
Every other element keeps its bits.  NumPy's float32 array arithmetic rounds each operation once and never
fuses two, which is what the product's host and device code are held to, bit for bit."""
from __future__ import annotations

import numpy as np

f32 = np.float32

# (repetition, presence, frequency)
PARAMS = [(1.3, 0.0, 0.0), (1.0, 0.7, 0.0), (1.0, 0.0, 0.25), (0.8, -0.5, 0.1), (1.1, 0.4, 0.2)]
VOCABS = (1000, 4100)
CONTEXT_KINDS = ("empty", "one", "same40", "seven300", "perm", "rand2047")
# values planted on counted tokens: both zeros (the l <= 0 branch at its edge), both huge signs, a subnormal
PLANTED = np.array([0.0, -0.0, 1e30, -1e30, 1e-40], f32)


def counts_of(context, V) -> np.ndarray:
    ctx = np.asarray(context, np.int64).reshape(-1)
    return np.bincount(ctx, minlength=V)[:V].astype(np.int64)


def penalize(logits_f32, context, repetition, presence, frequency) -> np.ndarray:
    lg = np.array(logits_f32, f32).reshape(-1)
    cnt = counts_of(context, lg.size)
    on = cnt > 0
    l = lg[on]
    with np.errstate(all="ignore"):
        a = np.where(l <= f32(0.0), l * f32(repetition), l / f32(repetition)).astype(f32)
        b = cnt[on].astype(f32) * f32(frequency)
        d = b + f32(presence)
        lg[on] = a - d
    return lg


def context(kind: str, V: int, seed: int = 0) -> np.ndarray:
    r = np.random.RandomState(1000 + seed)
    if kind == "empty":
        return np.zeros(0, np.int32)
    if kind == "one":
        return np.array([r.randint(V)], np.int32)
    if kind == "same40":
        return np.full(40, r.randint(V), np.int32)
    if kind == "seven300":
        return r.choice(V, 7, replace=False)[r.randint(7, size=300)].astype(np.int32)
    if kind == "perm":
        return r.permutation(V).astype(np.int32)
    if kind == "rand2047":
        return r.randint(V, size=2047).astype(np.int32)
    raise ValueError(kind)


def logits_for(ctx, V: int, seed: int = 0) -> np.ndarray:
    """N(0, 4) float32 logits with PLANTED cycled over the context's distinct tokens, as many as it has."""
    lg = (np.random.RandomState(2000 + seed).standard_normal(V) * 2.0).astype(f32)
    ids = np.unique(np.asarray(ctx, np.int64))
    lg[ids[: PLANTED.size]] = PLANTED[: ids.size]
    return lg


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, f32).view(np.uint32)
