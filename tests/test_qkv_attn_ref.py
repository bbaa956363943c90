"""The float64 reference of the fused QKV + attention launch (tests/qkv_attn_ref.py) pinned to the
project's oracle, and the preconditions of its inputs -- no GPU.

  * one small shape (heads 8, kv 2, hd 64, p = 37): RoPE of q / k against oracle.apply_rope, the
    attention row against oracle.multi_head_attention, rms against oracle.rms_norm; fp32 rounding,
    rtol 1e-5 against the oracle's fp32 (atol 1e-6 for elements that cancel to near zero; values are O(1));
  * the host merge of partials against the unsplit reference, with an empty split;
  * for every shape of test_gpu_qkv_attn_oracle.py: the planted row of `needle(j)` and `new_key_only`
    holds >= 0.9 of every head's softmax in the reference;
  * the reference-side perturbations used to show the GPU tests' sensitivity (a key skipped, a split's
    range shifted by one, two kv-heads' new keys swapped) move the needle cases far past the GPU
    tests' 4e-3.
"""
from __future__ import annotations

import numpy as np
import pytest

import qkv_attn_ref as R

f16, f32, f64 = np.float16, np.float32, np.float64
THETA = 10000.0


def small_case(ti_host, oracle, p=37, heads=8, kv_heads=2, hd=64, K=256, max_seq=64, bits=8):
    rng = np.random.RandomState(5)
    N = (heads + 2 * kv_heads) * hd
    wf = R.dequantized(oracle, (rng.standard_normal((K, N)) * 0.06).astype(f32), bits)
    fx = R.make_fx(K, 1)
    h = rng.standard_normal(K).astype(f32)          # the row whose sums of squares the producer hands over
    ss = np.array([np.sum(h[a:b].astype(f64) ** 2) for a, b in ((0, 100), (100, 101), (101, K))]).astype(f32)
    cs = ti_host.rope_table(np.arange(max_seq), hd, THETA)
    kc, vc = R.flat_cache(kv_heads, max_seq, hd, 3)
    lin = R.project(fx, wf)
    pr, at = R.launch_ref(lin, ss, R.EPS, cs, p, kc, vc, K, heads, kv_heads, hd)
    return dict(pr=pr, at=at, lin=lin, ss=ss, h=h, cs=cs, kc=kc, vc=vc, fx=fx, wf=wf, K=K, heads=heads,
                kv_heads=kv_heads, hd=hd, p=p)


def test_reference_matches_oracle(ti_host, oracle):
    c = small_case(ti_host, oracle)
    pr, at, heads, kvh, hd, p, K = c["pr"], c["at"], c["heads"], c["kv_heads"], c["hd"], c["p"], c["K"]
    qd, kvd = heads * hd, kvh * hd
    tol = dict(rtol=1e-5, atol=1e-6)
    # rms: oracle.rms_norm(h, 1) = h / rms
    y = oracle.rms_norm(c["h"].reshape(1, K), np.ones(K, f32), R.EPS).reshape(-1)
    big = np.abs(c["h"]) > 0.5
    np.testing.assert_allclose(np.full(big.sum(), pr.rms), c["h"][big].astype(f64) / y[big], rtol=1e-5)
    # RoPE: the un-rotated rows through the oracle
    pre = (c["lin"] / pr.rms).astype(f32)
    pos = np.array([p], f32)
    qo = oracle.apply_rope(pre[:qd].reshape(1, heads, 1, hd), pos, THETA).reshape(heads, hd)
    ko = oracle.apply_rope(pre[qd:qd + kvd].reshape(1, kvh, 1, hd), pos, THETA).reshape(kvh, hd)
    np.testing.assert_allclose(pr.q, qo, **tol)
    np.testing.assert_allclose(pr.k, ko, **tol)
    np.testing.assert_allclose(pr.v, pre[qd + kvd:].reshape(kvh, hd), **tol)
    # attention over [0, p], row p = the fp16 new row
    g = heads // kvh
    keys = np.concatenate([c["kc"][:, :p], pr.k16[:, None]], axis=1).astype(f32)      # [kvh][p + 1][hd]
    vals = np.concatenate([c["vc"][:, :p], pr.v16[:, None]], axis=1).astype(f32)
    kx = np.repeat(keys.transpose(1, 0, 2), g, axis=1).reshape(1, p + 1, qd)
    vx = np.repeat(vals.transpose(1, 0, 2), g, axis=1).reshape(1, p + 1, qd)
    ref = oracle.multi_head_attention(pr.q.astype(f32).reshape(1, 1, qd), kx, vx, heads).reshape(heads, hd)
    np.testing.assert_allclose(at.row, ref, **tol)
    # the reference's own quantities agree with each other
    np.testing.assert_allclose(at.weights.sum(axis=1), 1.0, rtol=1e-12)
    np.testing.assert_allclose(np.log(np.exp(at.scores).sum(axis=1)), at.lse, rtol=1e-12)


def test_merge_partials_recovers_unsplit_attention(ti_host, oracle):
    c = small_case(ti_host, oracle)
    pr, at, heads, kvh, hd, p = c["pr"], c["at"], c["heads"], c["kv_heads"], c["hd"], c["p"]
    g = heads // kvh
    vals = np.concatenate([c["vc"][:, :p], pr.v16[:, None]], axis=1).astype(f64)
    bounds = [0, 11, 11, 30, p + 1]          # split 1 empty
    S = len(bounds) - 1
    po, pml = np.zeros((heads, S, hd)), np.zeros((heads, S, 2))
    for s in range(S):
        a, b = bounds[s], bounds[s + 1]
        if a == b:
            pml[:, s] = (-np.inf, 0.0)
            continue
        sc = at.scores[:, a:b]
        m = sc.max(axis=1)
        e = np.exp(sc - m[:, None])
        pml[:, s, 0], pml[:, s, 1] = m, e.sum(axis=1)
        for h in range(heads):
            po[h, s] = (e[h] / e[h].sum()) @ vals[h // g, a:b]
    R.check_partials(po, pml)
    row, lse = R.merge_partials(po, pml)
    np.testing.assert_allclose(row, at.row, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(lse, at.lse, rtol=1e-12)
    with pytest.raises(AssertionError):      # a split that claims weight with a non-finite row is malformed
        bad = po.copy()
        bad[2, 0, 5] = np.nan
        R.check_partials(bad, pml)


@pytest.mark.parametrize("shape", R.ALL_SHAPES, ids=R.shape_id)
def test_planted_rows_hold_the_share(ti_host, oracle, shape):
    """needle(j) and new_key_only reach >= 0.9 for every head, at the positions the GPU tests use."""
    bits, K, heads, kvh, hd, splits = shape
    wf = R.dequantized(oracle, R.make_weight(shape), bits)
    lin = R.project(R.make_fx(K, 0), wf)
    del wf
    ss = R.make_ss(K, 3, 0)
    cases = [(320, 100, (0, 1, 50, 98, 99)), (320, 319, (0, 158, 159, 160, 318))]
    if shape in R.BENCH_SHAPES:
        cases.append((2048, 2047, (0, 255, 256, 1791, 1792, 2046)))
    for max_seq, p, js in cases:
        cs = ti_host.rope_table(np.arange(max_seq), hd, THETA)
        kc, vc = R.flat_cache(kvh, max_seq, hd, R.shape_seed(shape))
        pr, flat = R.launch_ref(lin, ss, R.EPS, cs, p, kc, vc, K, heads, kvh, hd)
        for j in js:
            k2, v2 = kc.copy(), vc.copy()
            k2[:, j], v2[:, j] = R.needle_rows(pr, flat, j, 0)
            R.assert_share(R.Attn(pr, k2, v2), j)
    cs = ti_host.rope_table(np.arange(320), hd, THETA)
    kc, vc = R.flat_cache(kvh, 320, hd, R.shape_seed(shape))
    for p in (1, 31, 32, 33, 255, 256, 257, 319):
        pr = R.Proj(lin, ss, R.EPS, cs, p, K, heads, kvh, hd)
        k2 = kc.copy()
        k2[:, :p] = R.new_key_only_row(pr)[:, None]
        R.assert_share(R.Attn(pr, k2, vc), p)


def test_reference_side_perturbations_are_visible(ti_host, oracle):
    """What the GPU tests would see of a kernel that skips key j, shifts a split's range by one (drops its
    first key, takes the next split's first key twice) or hands a head another kv-head's new key: the
    merged row moves by far more than their rtol = atol = 4e-3."""
    c = small_case(ti_host, oracle)
    pr, heads, kvh, hd, p = c["pr"], c["heads"], c["kv_heads"], c["hd"], c["p"]

    def red(a, b):
        return np.any(np.abs(a.row - b.row) > 4e-3 + 4e-3 * np.abs(b.row))

    j = 20
    k2, v2 = c["kc"].copy(), c["vc"].copy()
    k2[:, j], v2[:, j] = R.needle_rows(pr, c["at"], j, 0)
    good = R.Attn(pr, k2, v2)
    R.assert_share(good, j)
    skip = np.ones(p + 1)
    skip[j] = 0
    assert red(R.Attn(pr, k2, v2, multiplicity=skip), good)
    shift = np.ones(p + 1)
    shift[j], shift[j + 10] = 0, 2           # a split [j, j + 10) read as [j + 1, j + 11)
    assert red(R.Attn(pr, k2, v2, multiplicity=shift), good)
    shift = np.ones(p + 1)
    shift[j - 10], shift[j] = 0, 2           # a split [j - 10, j) read as [j - 9, j + 1): the needle twice
    assert red(R.Attn(pr, k2, v2, multiplicity=shift), good)
    # new key: kv-heads 0 and 1 swapped
    k3 = c["kc"].copy()
    k3[:, :p] = R.new_key_only_row(pr)[:, None]
    good = R.Attn(pr, k3, c["vc"])
    R.assert_share(good, p)
    assert red(R.Attn(pr, k3, c["vc"], new_row_from=[1, 0]), good)
