"""The float64 attention reference of tests/attn_ref.py pinned to the project's oracle, the host merge
of partials, and the sensitivity of the `indicator` inputs -- no GPU.

  * one small GQA shape (heads 8, kv 2, hd 64, three rows): `attend` against
    oracle.multi_head_attention, rtol 1e-5 (atol 1e-6 for elements that cancel to near zero);
  * the host merge of partials (one split empty) against the unsplit reference;
  * what the GPU tests would see of a kernel that is wrong by one key: each perturbation of the
    reference side moves `flat` + `indicator` outputs past `indicator_bound` by at least 10 times at
    L in {33, 257, 2048} and head_dim in {64, 128}, while the first four at L = 2048 stay inside
    rtol = atol = 4e-3 on `random` values -- the gap the float64 modules close.
"""
from __future__ import annotations

import numpy as np
import pytest

import attn_ref as A

f16, f32, f64 = np.float16, np.float32, np.float64


def test_reference_matches_oracle(oracle):
    M, heads, kvh, hd, max_seq = 3, 8, 2, 64, 48
    pos = np.array([0, 17, 40], np.int32)
    q, kc, vc = A.make_inputs("flat", "random", M, heads, kvh, hd, max_seq, pos, seed=1)
    row, lse = A.attend(q, kc, vc, pos, heads)
    g = heads // kvh
    for m in range(M):
        n = int(pos[m]) + 1
        kx = np.repeat(kc[m, :, :n].astype(f32).transpose(1, 0, 2), g, axis=1).reshape(1, n, heads * hd)
        vx = np.repeat(vc[m, :, :n].astype(f32).transpose(1, 0, 2), g, axis=1).reshape(1, n, heads * hd)
        ref = oracle.multi_head_attention(q[m].reshape(1, 1, -1), kx, vx, heads).reshape(heads, hd)
        np.testing.assert_allclose(row[m], ref, rtol=1e-5, atol=1e-6, err_msg=f"row {m}")
        sc = A.scores(q, kc, m, heads)[:, :n]
        np.testing.assert_allclose(np.log(np.exp(sc).sum(axis=1)), lse[m], rtol=1e-12)
    # a shared cache is the same operation on cache 0, and NaN behind the limit is never read
    kp, vp = A.poison(kc[:1], vc[:1], pos, shared=True)
    row1, lse1 = A.attend(q, kp, vp, pos, heads)
    row2, lse2 = A.attend(q, kc[:1], vc[:1], pos, heads)
    np.testing.assert_array_equal(row1, row2)
    np.testing.assert_array_equal(lse1, lse2)
    np.testing.assert_array_equal(row1[0], row[0])


def test_merge_partials_recovers_unsplit_attention():
    heads, kvh, hd, max_seq = 8, 2, 64, 48
    pos = np.array([37], np.int32)
    q, kc, vc = A.make_inputs("steep", "random", 1, heads, kvh, hd, max_seq, pos, seed=2)
    row, lse = A.attend(q, kc, vc, pos, heads)
    sc = A.scores(q, kc, 0, heads)
    g = heads // kvh
    bounds = [0, 11, 11, 30, 38]          # split 1 empty
    S = len(bounds) - 1
    po, pml = np.zeros((heads, S, hd)), np.zeros((heads, S, 2))
    for s in range(S):
        a, b = bounds[s], bounds[s + 1]
        if a == b:
            pml[:, s] = (-np.inf, 0.0)
            continue
        top = sc[:, a:b].max(axis=1)
        e = np.exp(sc[:, a:b] - top[:, None])
        pml[:, s, 0], pml[:, s, 1] = top, e.sum(axis=1)
        for h in range(heads):
            po[h, s] = (e[h] / e[h].sum()) @ vc[0, h // g, a:b].astype(f64)
    A.check_partials(po, pml)
    mrow, mlse = A.merge_partials(po, pml)
    np.testing.assert_allclose(mrow, row[0], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(mlse, lse[0], rtol=1e-12)


def _perturbations(L, j):
    """(name, attend keyword arguments) for a range of L keys around key j; the first four are the small ones."""
    skip = np.ones(L)
    skip[j] = 0
    # the middle one of three splits, [a, b) read as [a + 1, b + 1).  (b - a is no multiple of head_dim here:
    # if it were, the lost key a and the doubled key b would share an output element and only their
    # difference would show -- the GPU sweeps run splits = 3 at every length for that reason.)
    shift = np.ones(L)
    a, b = -(-L // 3), 2 * -(-L // 3)
    assert (b - a) % 64
    shift[a], shift[b] = 0, 2
    slot = np.ones(L)
    slot[(j // 4) * 4:(j // 4) * 4 + 4] = 0
    block = np.ones(L)
    block[(j // 16) * 16:(j // 16) * 16 + 16] = 0
    return [("one key skipped", dict(mult=skip)), ("split range shifted by one", dict(mult=shift)),
            ("key pos + 1 admitted", dict(extra=1)), ("one 4-key slot lost", dict(mult=slot)),
            ("one 16-key block lost", dict(mult=block)), ("two kv-heads swapped", dict(kv_map=[1, 0]))]


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("L", [33, 257, 2048])
def test_reference_side_perturbations_are_visible(L, hd):
    """Two heads on two kv-heads, one row of L keys, seed 0; key j is head 0's median-score key (a key of
    ordinary weight: neither the easiest nor the hardest to lose).
    The second assertion is a statement about seeded inputs, so its margin is recorded here: over seeds
    0 .. 19 of this shape the worst element of the `random` output moves by (median / worst over seeds, in
    units of 4e-3 + 4e-3 |ref|) 0.33 / 0.91 (key skipped), 0.49 / 0.91 (range shifted), 0.30 / 0.87 (key
    admitted) and 0.80 / 1.53 (4-key slot): single keys are invisible at that tolerance, a lost slot of four
    sits AT it (seen at some seeds, not at others).  Seed 0 gives 0.26-0.54, 0.35-0.42, 0.20-0.39, 0.69."""
    heads, kvh, max_seq = 2, 2, L + 1
    pos = np.array([L - 1], np.int32)
    q, kc, vc = A.make_inputs("flat", "indicator", 1, heads, kvh, hd, max_seq, pos, seed=0)
    good, _ = A.attend(q, kc, vc, pos, heads)
    bound = A.indicator_bound(good)
    qr, kr, vr = A.make_inputs("flat", "random", 1, heads, kvh, hd, max_seq, pos, seed=0)
    assert np.array_equal(q, qr) and np.array_equal(kc, kr)
    good_r, _ = A.attend(qr, kr, vr, pos, heads)
    j = int(np.argsort(A.scores(q, kc, 0, heads)[0, :L])[L // 2])
    for n, (name, kw) in enumerate(_perturbations(L, j)):
        bad, _ = A.attend(q, kc, vc, pos, heads, **kw)
        over = np.abs(bad - good) / bound
        # every head sees it, not only the most exposed one
        assert np.all(over.max(axis=-1) >= 10), f"{name}: only {over.max(axis=-1).min():.1f} x the bound at L={L}"
        if L == 2048 and n < 4:
            bad_r, _ = A.attend(qr, kr, vr, pos, heads, **kw)
            assert np.all(A.random_ok(bad_r, good_r)), f"{name}: visible at atol 4e-3 after all"
