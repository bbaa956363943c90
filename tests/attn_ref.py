"""Test helper: a float64 reference of single-query / causal-chunk attention over fp16 caches (what
ti_attn_decode, ti_attn_decode_packed, ti_attn_decode_partials and ti_attn_prefill compute), and
seeded inputs that make every single key count.  numpy only; `merge_partials` / `check_partials`
come from qkv_attn_ref.py.

The reference (`attend`) is the operation and nothing else:
    row m, q-head h reads kv-head h // G (G = heads / kv_heads)
    scores  s_j = q[m, h] . K[j] / sqrt(head_dim)   over keys j in [0, pos[m]]
    lse     = log sum_j exp(s_j)
    row     = sum_j softmax(s)_j V[j]
in float64 from the very fp32 q and fp16 K / V values that are uploaded.  It knows nothing of splits,
slots, rings, blocks or lane layouts.  `mult`, `extra` and `kv_map` perturb the REFERENCE side (a key
counted 0 or 2 times, keys past pos admitted, kv-heads exchanged): how the sensitivity of the GPU
tests is shown in test_attn_ref.py.

Inputs (`make_inputs`, all seeded; K differs per kv-head and per stream):
  flat    K = 0.5 N(0,1), q = N(0,1): score spread about 0.5, an almost flat softmax.
  steep   K = 3 N(0,1): score spread about 3, the running maximum moves often.
  ramp    flat, with a planted direction u (one unit vector per kv-head): every q-head gets the common
          component sqrt(head_dim) u, and the last min(64, L) keys of each stream's range get + i u
          (i = 0 .. n-1), so scores rise by about 1 per key and every key rescales the running state.
          With a shared cache (one cache for all rows) the rows' ranges differ, so key j gets
          + (j % 64) u instead: a sawtooth that rises by about 1 per key up to every row's end.
          This kind exercises the rescale arithmetic only; it does not account for keys (the early
          keys carry weights far below the bound).
  values  `random`: V = N(0,1).
          `indicator`: V[kvh][j][d] = 1 if d == (j + 7 kvh) % head_dim else 0.  Output element d is then
          the sum of the softmax weights of the keys j = d - 7 kvh (mod head_dim): positive terms only, no
          cancellation; with L <= head_dim one key per element, at L = 2048 and head_dim 128 sixteen.  A
          lost, doubled or wrongly admitted key changes one element by at least 1/16 (1/32 at head_dim
          64) of itself -- every key counts at any length in a single launch.
  behind the limit (`poison`): with a cache per stream, rows > pos[m] of K and V hold NaN; with a
          shared cache, rows past the chunk's largest position hold NaN (the per-row limit inside the
          chunk is what `indicator` covers).

Bound for `indicator` outputs (`indicator_bound`), per head, derived and not measured, L <= 2048:
    |got - ref| <= 2^-10 |ref| + 2^-18 max_d |ref[h]| + 2^-23
  2^-10 |ref|          the fp16 store (2^-11), fp32 accumulation of at most 2048 positive terms (at most
                       2^-13) and the fp32 score error through exp;
  2^-18 max_d |ref[h]| small unnormalised p: the prefill kernels split p into fp16 hi + lo and lose what
                       lies below fp16's subnormal step, about 2^-24 of the largest p per key, for up to
                       16 (32) keys per element;
  2^-23                two fp16 subnormal steps of the stored value.
`random` values keep the project's rtol = atol = 4e-3 (RTOL, ATOL), now against float64.
"""
from __future__ import annotations

import numpy as np

from qkv_attn_ref import check_partials, merge_partials  # noqa: F401  (re-exported for the test modules)

f16, f32, f64 = np.float16, np.float32, np.float64

RTOL = ATOL = 4e-3          # `random` values: the project's figure for these kernels
KINDS = ("flat", "steep", "ramp")
RAMP = 64                   # keys of the planted ramp

# lengths around every slot / pass / ring boundary of the decode kernels (the M = 1 variants' sweep)
SWEEP_L = sorted(set(list(range(1, 11)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192,
                                           193, 255, 256, 257, 300]))


# ------------------------------------------------------------------ the reference
def attend(q, kc, vc, pos, heads, mult=None, extra=0, kv_map=None):
    """q [M][heads * hd] fp32; kc, vc [S][kv_heads][max_seq][hd] fp16 with S = M (a cache per stream) or
    S = 1 (one cache for all rows); pos [M] -> (row [M][heads][hd], lse [M][heads]) in float64.
    Perturbations: mult [pos + 1 + extra] times each key is counted (all rows; M = 1 or equal pos),
    extra keys past pos admitted, kv_map[i] the kv-head that kv-head i's q-heads read instead."""
    q = np.asarray(q)
    M = q.shape[0]
    S, kvh, max_seq, hd = kc.shape
    assert vc.shape == kc.shape and S in (1, M) and heads % kvh == 0 and q.shape[1] == heads * hd
    g = heads // kvh
    src = np.arange(kvh) if kv_map is None else np.asarray(kv_map)
    row = np.empty((M, heads, hd), f64)
    lse = np.empty((M, heads), f64)
    for m in range(M):
        n = int(pos[m]) + 1 + extra
        assert 1 <= n <= max_seq
        s = m if S == M else 0
        keys = kc[s, :, :n][src].astype(f64)                      # [kvh][n][hd]
        vals = vc[s, :, :n][src].astype(f64)
        qm = q[m].astype(f64).reshape(kvh, g, hd)
        z = np.matmul(qm, keys.transpose(0, 2, 1)) / np.sqrt(float(hd))      # [kvh][g][n]
        if mult is not None:
            with np.errstate(divide="ignore"):
                z = z + np.log(np.asarray(mult, f64))
        top = z.max(axis=-1, keepdims=True)
        e = np.exp(z - top)
        tot = e.sum(axis=-1, keepdims=True)
        row[m] = np.matmul(e / tot, vals).reshape(heads, hd)
        lse[m] = (top + np.log(tot)).reshape(heads)
    return row, lse


def scores(q, kc, m, heads):
    """The float64 scores [heads][max_seq] of row m against every cache row (no limit applied)."""
    S, kvh, max_seq, hd = kc.shape
    keys = kc[m if S > 1 else 0].astype(f64)
    qm = np.asarray(q)[m].astype(f64).reshape(kvh, heads // kvh, hd)
    return (np.matmul(qm, keys.transpose(0, 2, 1)) / np.sqrt(float(hd))).reshape(heads, max_seq)


def indicator_bound(ref_row):
    """The per-element bound for `indicator` values (module docstring); ref_row [..., heads, hd]."""
    a = np.abs(ref_row)
    return 2.0 ** -10 * a + 2.0 ** -18 * a.max(axis=-1, keepdims=True) + 2.0 ** -23


def random_ok(got, ref):
    return np.abs(got - ref) <= ATOL + RTOL * np.abs(ref)


# ------------------------------------------------------------------ seeded inputs
def indicator_values(kv_heads, max_seq, hd):
    v = np.zeros((kv_heads, max_seq, hd), f16)
    j = np.arange(max_seq)
    for i in range(kv_heads):
        v[i, j, (j + 7 * i) % hd] = 1
    return v


def make_inputs(kind, values, M, heads, kv_heads, hd, max_seq, pos, seed, shared=False):
    """-> q [M][heads * hd] fp32, kc, vc [S][kv_heads][max_seq][hd] fp16 (S = 1 if shared else M), every
    cache row finite (`poison` makes the copy to upload)."""
    assert kind in KINDS and values in ("random", "indicator")
    rng = np.random.default_rng([seed, M, heads, kv_heads, hd, max_seq, KINDS.index(kind)])
    S = 1 if shared else M
    q = rng.standard_normal((M, heads, hd), dtype=f32)
    k = rng.standard_normal((S, kv_heads, max_seq, hd), dtype=f32)
    k *= f32(3.0 if kind == "steep" else 0.5)
    if kind == "ramp":
        u = rng.standard_normal((kv_heads, hd))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        q += (np.sqrt(float(hd)) * np.repeat(u, heads // kv_heads, axis=0)).astype(f32)[None]
        if shared:
            k[0] += ((np.arange(max_seq) % RAMP)[None, :, None] * u[:, None, :]).astype(f32)
        else:
            for m in range(M):
                L = int(pos[m]) + 1
                n = min(RAMP, L)
                k[m, :, L - n:L] += (np.arange(n)[None, :, None] * u[:, None, :]).astype(f32)
    kc = k.astype(f16)
    del k
    if values == "indicator":
        vc = np.broadcast_to(indicator_values(kv_heads, max_seq, hd), (S, kv_heads, max_seq, hd))
    else:
        vc = rng.standard_normal((S, kv_heads, max_seq, hd), dtype=f32).astype(f16)
    return q.reshape(M, heads * hd), kc, vc


def poison(kc, vc, pos, shared=False):
    """Copies of the caches with NaN in every row the launch must not use (module docstring)."""
    kc, vc = np.array(kc, f16), np.array(vc, f16)
    if shared:
        top = int(np.max(pos))
        kc[:, :, top + 1:] = np.nan
        vc[:, :, top + 1:] = np.nan
    else:
        for m in range(kc.shape[0]):
            kc[m, :, int(pos[m]) + 1:] = np.nan
            vc[m, :, int(pos[m]) + 1:] = np.nan
    return kc, vc
