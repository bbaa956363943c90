"""The sampler with a per-row parameter table (ti_hip.h ti_sample_device_rows / ti_sample_step_rows): row m's
temperature, top_k and top_p come from rows[m] in device memory instead of the kernel's arguments.

V in {1000, 32000}, 9 rows of seeded logits (standard_normal * 3) in ONE launch, the seven parameter sets of SETS
cycled over them (so two sets occur twice), top_k capped at V.  Checked:
  1. every row equals, token and log p bit for bit, a scalar ti_sample_device launch of that row alone;
  2. every row equals the oracle's sample_token (oracle/ti_oracle_sample.cpp): same token, log p within the
     1e-5 * max(1, |lp|) of tests/test_gpu_sample.py;
  3. permuting table, logits and draws together permutes the results;
  4. table entries nobody validated -- top_k 0, -3, V + 5 -- behave as 1, 1, min(V, max_top_k), and nothing is
     written behind tokens / logprobs;
  5. max_top_k = V (every row on the workspace instance): the k > TI_SAMPLE_MAX_K rows equal ti_sample_device_ws
     bit for bit, all rows equal the oracle;
  6. the step form: rows outside their draw window leave argmax and logprobs untouched.
The seeds were picked on the CPU so that no interior draw lies within 1e-5 of a cumulative boundary of the oracle's
distribution (asserted, no row skipped); the two placed draws are decided by rule, not by a comparison's margin:
u = 0.0 returns index 0 at the reference's first comparison, and u = 1.0 sits in a one-survivor row (p = 1 exactly)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from test_gpu_attn_oracle import dev, fetch, guard_intact, guarded

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
MAX_K = 4096                      # TI_SAMPLE_MAX_K
M = 9
SETS = [(1.0, 1, 1.0), (0.7, 40, 0.9), (1.3, 1024, 0.95), (0.0, 8, 0.5), (1.0, 1500, 1.0),   # 1500: the radix route
        (0.9, 4096, 0.97), (1.0, 200, 0.0)]
SEEDS = {1000: 2, 32000: 2}
BIG_SEED = 4
ROW_U1, ROW_U0 = 0, 1             # u = 1.0 in the greedy row, u = 0.0 in the (0.7, 40, 0.9) row


def table(params):
    """ti_row_params [len(params)] as bytes: (temperature, top_k, top_p, 1, 0, 0, 0, 0)."""
    t = np.zeros(len(params), np.dtype([("t", f32), ("k", i32), ("p", f32), ("pen", f32, 3), ("res", i32, 2)]))
    assert t.itemsize == 32
    for m, (T, k, p) in enumerate(params):
        t[m] = (T, k, p, (1.0, 0.0, 0.0), (0, 0))
    return t


def inputs(V, seed, params):
    rng = np.random.RandomState(seed)
    logits = (rng.standard_normal((len(params), V)) * 3).astype(f32)
    draws = rng.uniform(0.01, 0.99, len(params)).astype(f32)
    return logits, draws


def margin(oracle, logits, params, draws, skip=()):
    """Smallest distance of a draw to a cumulative boundary of the oracle's distribution of its row."""
    worst = np.inf
    for m, (T, k, p) in enumerate(params):
        if m in skip:
            continue
        cum = np.cumsum(oracle.sample_probs(logits[m], T, k, p), dtype=f32).astype(np.float64)
        worst = min(worst, float(np.min(np.abs(cum - float(draws[m])))), float(draws[m]))
    return worst


def assert_oracle(oracle, logits, params, draws, tok, lp):
    for m, (T, k, p) in enumerate(params):
        want_t, want_lp = oracle.sample_token(logits[m], T, k, p, float(draws[m]))
        assert int(tok[m]) == want_t, (m, params[m], int(tok[m]), want_t)
        if np.isfinite(want_lp):
            assert abs(float(lp[m]) - want_lp) <= 1e-5 * max(1.0, abs(want_lp)), (m, params[m], lp[m], want_lp)
        else:
            assert not np.isfinite(lp[m]), (m, params[m], lp[m])


def launch_rows(ti, logits, params, draws, max_top_k, ws=None):
    """One ti_sample_device_rows launch over all rows -> (tokens, logprobs), the guard pattern behind both checked."""
    n, V = logits.shape
    ld, dd, td = dev(ti, logits), dev(ti, draws), dev(ti, table(params))
    tok_d, lp_d = guarded(ti, n * 4), guarded(ti, n * 4)
    ti.check(ti.lib().ti_sample_device_rows(ld.ptr, V, n, V, td.ptr, max_top_k, dd.ptr, tok_d.ptr, lp_d.ptr,
                                            ws.ptr if ws else None, None))
    ti.sync()
    guard_intact(ti, tok_d, n * 4, "the tokens")
    guard_intact(ti, lp_d, n * 4, "the logprobs")
    return fetch(ti, tok_d, 0, n * 4).view(i32), fetch(ti, lp_d, 0, n * 4).view(f32)


def launch_scalar(ti, row, T, k, p, u, ws=None):
    V = row.size
    ld, dd = dev(ti, row), dev(ti, np.array([u], f32))
    tok_d, lp_d = ti.DeviceBuffer(4), ti.DeviceBuffer(4)
    ti.check(ti.lib().ti_sample_device_ws(ld.ptr, V, 1, V, T, k, p, dd.ptr, tok_d.ptr, lp_d.ptr, ws.ptr if ws else None, None))
    ti.sync()
    return int(tok_d.download(i32, 1)[0]), lp_d.download(f32, 1)


CASES = {}


def case(ti, V):
    """The shared launch of one V: inputs, the table's results (computed once, never modified)."""
    if V not in CASES:
        params = [(T, min(k, V), p) for T, k, p in (SETS[m % len(SETS)] for m in range(M))]
        logits, draws = inputs(V, SEEDS[V], params)
        draws[ROW_U1], draws[ROW_U0] = 1.0, 0.0
        tok, lp = launch_rows(ti, logits, params, draws, min(V, MAX_K))
        for a in (logits, draws, tok, lp):
            a.setflags(write=False)
        CASES[V] = params, logits, draws, tok, lp
    return CASES[V]


@pytest.mark.parametrize("V", [1000, 32000])
def test_each_row_is_the_scalar_launch_of_its_values(ti, V):
    params, logits, draws, tok, lp = case(ti, V)
    assert params[7] == params[0] and params[8] == params[1]         # two sets occur twice
    for m, (T, k, p) in enumerate(params):
        t1, lp1 = launch_scalar(ti, logits[m], T, k, p, draws[m])
        assert int(tok[m]) == t1, (m, params[m])
        assert lp[m: m + 1].view(np.uint32)[0] == lp1.view(np.uint32)[0], (m, params[m], lp[m], lp1)


@pytest.mark.parametrize("V", [1000, 32000])
def test_each_row_is_the_oracle_sampler(ti, oracle, V):
    params, logits, draws, tok, lp = case(ti, V)
    worst = margin(oracle, logits, params, draws, skip=(ROW_U1, ROW_U0))
    print(f"\nV {V}: smallest distance of an interior draw to a cumulative boundary {worst:.3e}")
    assert worst >= 1e-5
    assert params[ROW_U1][1] == 1                                     # u = 1.0: one survivor, p = 1 exactly
    assert_oracle(oracle, logits, params, draws, tok, lp)
    assert int(tok[ROW_U0]) == 0


@pytest.mark.parametrize("V", [1000, 32000])
def test_permuting_the_rows_permutes_the_results(ti, V):
    params, logits, draws, tok, lp = case(ti, V)
    perm = np.random.RandomState(3).permutation(M)
    assert not np.array_equal(perm, np.arange(M))
    tok_p, lp_p = launch_rows(ti, logits[perm], [params[i] for i in perm], draws[perm], min(V, MAX_K))
    assert np.array_equal(tok_p, tok[perm])
    assert np.array_equal(lp_p.view(np.uint32), lp[perm].view(np.uint32))


@pytest.mark.parametrize("V", [1000, 32000])
def test_an_unvalidated_top_k_is_clamped(ti, V):
    _, logits, draws, _, _ = case(ti, V)
    cap = min(V, MAX_K)
    bad, eff = [0, -3, V + 5], [1, 1, cap]
    lg, u = logits[2:5], np.array([0.3, 0.6, 0.45], f32)
    tok, lp = launch_rows(ti, lg, [(0.9, k, 0.98) for k in bad], u, cap)       # (guards checked inside)
    for m, k in enumerate(eff):
        t1, lp1 = launch_scalar(ti, lg[m], 0.9, k, 0.98, u[m])
        assert int(tok[m]) == t1, (bad[m], k)
        assert lp[m: m + 1].view(np.uint32)[0] == lp1.view(np.uint32)[0], (bad[m], k)
    # a smaller host bound is the cap: V + 5 under max_top_k = 7 is 7
    tok7, lp7 = launch_rows(ti, lg[2:3], [(0.9, V + 5, 0.98)], u[2:3], 7)
    t1, lp1 = launch_scalar(ti, lg[2], 0.9, 7, 0.98, u[2])
    assert int(tok7[0]) == t1 and lp7.view(np.uint32)[0] == lp1.view(np.uint32)[0]


def test_workspace_instance_for_every_row(ti, oracle):
    V = 32000
    params = [(1.0, V, 0.95), (0.8, 8192, 0.9), (0.7, 40, 0.9)]
    logits, draws = inputs(V, BIG_SEED, params)
    worst = margin(oracle, logits, params, draws)
    print(f"\nsmallest distance of a draw to a cumulative boundary {worst:.3e}")
    assert worst >= 1e-5
    L = ti.lib()
    L.ti_sample_workspace_bytes.restype = C.c_size_t
    L.ti_sample_workspace_bytes.argtypes = [C.c_int, C.c_int]
    wsb = L.ti_sample_workspace_bytes(V, V)
    assert wsb > 0
    ws = guarded(ti, len(params) * wsb)
    tok, lp = launch_rows(ti, logits, params, draws, V, ws=ws)
    guard_intact(ti, ws, len(params) * wsb, "the workspace")
    ws1 = ti.DeviceBuffer(wsb)
    for m, (T, k, p) in enumerate(params):
        if k <= MAX_K:
            continue
        t1, lp1 = launch_scalar(ti, logits[m], T, k, p, draws[m], ws=ws1)
        assert int(tok[m]) == t1, (m, k)
        assert lp[m: m + 1].view(np.uint32)[0] == lp1.view(np.uint32)[0], (m, k)
    assert_oracle(oracle, logits, params, draws, tok, lp)


def test_step_form_rows_outside_their_window_do_nothing(ti):
    """n_in = (1, 3, 5, 1, 2), draw_stride 2, the counter at 3 with advance 1: t = 2 - (n_in - 1) = (2, 0, -2, 2, 1):
    rows 1 and 4 sample (draw and log p slot t), the others keep the pattern in argmax and logprobs."""
    V = 1000
    params, logits, _, _, _ = case(ti, V)
    n, stride, slots = 5, 2, 32                                 # TI_ARGMAX_SLOTS
    n_in = np.array([1, 3, 5, 1, 2], i32)
    t = 2 - (n_in - 1)
    draws = np.random.RandomState(8).uniform(0.05, 0.95, (n, stride)).astype(f32)
    ld, dd, td = dev(ti, logits[:n]), dev(ti, draws), dev(ti, table(params[:n]))
    am, lps = guarded(ti, n * slots * 8), guarded(ti, n * stride * 4)
    ctr, nin = dev(ti, np.array([3], i32)), dev(ti, n_in)
    ti.check(ti.lib().ti_sample_step_rows(ld.ptr, V, n, V, td.ptr, V, dd.ptr, stride, ctr.ptr, 1, nin.ptr, am.ptr, lps.ptr,
                                          None, None))
    ti.sync()
    guard_intact(ti, am, n * slots * 8, "argmax")
    guard_intact(ti, lps, n * stride * 4, "logprobs")
    keys = fetch(ti, am, 0, n * slots * 8).view(np.uint64).reshape(n, slots)
    got_lp = fetch(ti, lps, 0, n * stride * 4).view(np.uint32).reshape(n, stride)
    pat64, pat32 = np.uint64(0xA5A5A5A5A5A5A5A5), np.uint32(0xA5A5A5A5)
    active = 0
    for m in range(n):
        assert np.all(keys[m, 1:] == pat64), m
        if 0 <= t[m] < stride:
            active += 1
            T, k, p = params[m]
            t1, lp1 = launch_scalar(ti, logits[m], T, k, p, draws[m, t[m]])
            assert int(keys[m, 0] >> np.uint64(32)) == 0xFFFFFFFF and 0xFFFFFFFF - int(keys[m, 0] & np.uint64(0xFFFFFFFF)) == t1, m
            assert got_lp[m, t[m]] == lp1.view(np.uint32)[0] and got_lp[m, 1 - t[m]] == pat32, m
        else:
            assert keys[m, 0] == pat64 and np.all(got_lp[m] == pat32), m
    assert active == 2
