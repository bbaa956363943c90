"""The NumPy statement of the device sampler's contract (tests/sample_ref.py) checked on the CPU, and the case
table of tests/test_gpu_sample_edges.py (tests/sample_edge_cases.py) checked against it:

  * on tie-free rows the reference IS the oracle sampler (oracle.sample_token): same token, log p within 1e-6
    relative (floor 1.0), over the (T, k, p) grid of test_gpu_sample.py at V = 63, 1000 and 32769, for three
    placed draws, u = 0 and u = 1;
  * on tied rows it is the oracle wherever the oracle's std::sort happens to leave the lowest indices;
  * every case of the GPU table is decidable by the reference alone: placed draw margins >= 1e-5, top-p margin
    >= 1e-5 where top_p < 1, rank gap at the cut exactly 0 or >= 1e-5; u = 0 is decided by its rule, u = 1 is
    either decided or has exactly two stated answers (sample_ref.py);
  * every case labelled a tie case changes under the reversed tie rule, and no other case does.
"""
from __future__ import annotations

import numpy as np
import pytest

import sample_edge_cases as E
import sample_ref as R

f32 = np.float32
GRID = [(1.0, 1, 1.0), (0.7, 40, 0.9), (1.0, 50, 1.0), (1.3, 1024, 0.95), (0.0, 8, 0.5), (1.0, 200, 0.0),
        (1.0, 1500, 1.0), (0.9, 2500, 0.97), (1.0, 4096, 0.9)]
TIED_SETTINGS = [(1.0, 2, 1.0), (1.0, 3, 1.0), (0.7, 40, 0.9), (2.0, 7, 0.99), (0.9, 9, 1.0), (1.0, 50, 0.9),
                 (0.5, 1000, 0.5)]


def same_answer(d, tok, lp, tol):
    if d.token != tok:
        return False
    if np.isfinite(d.logprob):
        return abs(lp - d.logprob) <= tol * max(1.0, abs(d.logprob))
    return lp == d.logprob


def check_against_oracle(oracle, logits, T, k, p):
    """Three placed draws, u = 0 and u = 1 of one row: the reference's answer is the oracle's."""
    cut = R.top_p_cut(R.survivors(logits, T, k), p)
    assert E.decidable_cut(cut), (T, k, p, cut.top_p_margin, cut.rank_gap)
    for u in [R.place_draw(cut.row, w) for w in E.DRAWS] + [f32(0), f32(1)]:
        d = R.draw(cut.row, u)
        tok, lp = oracle.sample_token(logits, T, k, p, float(u))
        assert d.decided or u == 1, (T, k, p, u, d)
        assert same_answer(d, tok, lp, 1e-6) or (d.alt is not None and same_answer(d._replace(
            token=d.alt[0], logprob=d.alt[1]), tok, lp, 1e-6)), (T, k, p, u, d, tok, lp)


def test_tiny_rows_by_hand():
    """Rows small enough to do on paper."""
    d = R.sample([1.0, 1.0, 1.0, 1.0], 1.0, 2, 1.0, 0.75)            # ties: indices 0 and 1 survive, p = 1/2 each
    assert (d.token, d.logprob) == (1, float(np.log(f32(0.5))))
    assert R.sample([1.0, 1.0, 1.0, 1.0], 1.0, 2, 1.0, 0.75, _ties_high=True).token == 3
    row = R.survivors([-0.0, 0.0, -0.0, 0.0, -1.0], 1.0, 2)         # zeros of both signs are one value
    assert row.idx.tolist() == [0, 1] and row.exact
    cut = R.top_p_cut(R.survivors([0.0, 0.0, 0.0, 0.0], 0.5, 4), 0.6)   # p = 1/4 each; 0.25, 0.5, 0.75 >= 0.6
    assert cut.row.p.tolist() == [f32(0.25) / f32(0.75)] * 3 + [0.0] and cut.rank_gap == 0.0
    assert abs(cut.top_p_margin - 0.1) < 1e-6
    d = R.draw(cut.row, 0.0)
    assert (d.token, d.decided) == (0, True)
    d = R.sample([0.0, 5.0, 0.0], 1.0, 1, 1.0, 0.0)                  # u = 0: token 0, which did not survive
    assert (d.token, d.logprob) == (0, -np.inf)
    d = R.sample([0.0, 5.0, 0.0], 1.0, 1, 1.0, 1.0)                  # the one survivor has p = 1: u <= 1 finds it
    assert (d.token, d.logprob, d.decided) == (1, 0.0, True)
    d = R.sample([0.0, 1.0], 0.0, 2, 1.0, 0.5)                       # T <= 0: no scaling; p = 1/(1+e), e/(1+e)
    assert d.token == 1 and abs(d.margin - (0.5 - 1 / (1 + np.e))) < 1e-6


@pytest.mark.parametrize("V", [63, 1000, 32769])
def test_reference_is_the_oracle_on_tie_free_rows(oracle, V):
    rng = np.random.RandomState(V)
    for T, k, p in GRID:
        if k > V:
            continue
        g = (rng.standard_normal(2 * V) * 3).astype(f32)
        first = np.unique(g / f32(T) if T > 0 and T != 1 else g, return_index=True)[1]
        logits = g[rng.permutation(first)[:V]]                          # distinct, also after the temperature
        assert np.unique(logits / f32(T) if T > 0 and T != 1 else logits).size == V
        check_against_oracle(oracle, logits, T, k, p)


def test_reference_is_the_oracle_where_its_tie_order_is_lowest_index(oracle):
    """The plumbing logits of test_gpu_sample.py (every value twice) and a row rounded to steps of 0.5."""
    V = 1000
    rows = [oracle.plumbing_generate(V, 256, 4, [1, 15, 25, 35], s + 1)[1] for s in range(2)]
    rows.append((np.round(np.random.RandomState(3).standard_normal(V) * 6) / 2).astype(f32))
    agree = 0
    for logits in rows:
        for T, k, p in TIED_SETTINGS:
            row = R.survivors(logits, T, k)
            cut = R.top_p_cut(row, p)
            kept = set(cut.row.idx[cut.row.p > 0].tolist())
            if kept != set(np.flatnonzero(oracle.sample_probs(logits, T, k, p) > 0).tolist()):
                continue
            if not E.decidable_cut(cut):
                continue
            check_against_oracle(oracle, logits, T, k, p)
            agree += 1
    assert agree >= 8, agree


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_gpu_case_is_decidable(name):
    r = E.realise(name)
    assert r.case.near >= 1 or r.top_p < 1
    assert E.decidable_cut(r.cut), (r.cut.top_p_margin, r.cut.rank_gap)
    for u, d in zip(r.draws[:4], r.want[:4]):
        assert d.decided and d.margin >= R.MARGIN, (u, d)
    last = r.want[4]
    assert last.decided or last.alt is not None
    # the placed draws land on different survivors wherever there are that many
    assert len({d.token for d in r.want[:3]}) == min(3, int((r.cut.row.p >= R.MIN_PLACED_P).sum()))


def changed_by_reversed_ties(logits, T, k, top_p, draws, cut, want):
    hi = R.top_p_cut(R.survivors(logits, T, k, _ties_high=True), top_p, _ties_high=True).row
    if set(hi.idx[hi.p > 0].tolist()) != set(cut.row.idx[cut.row.p > 0].tolist()):
        return True
    return any((d.token, d.logprob) != (w.token, w.logprob) for d, w in zip((R.draw(hi, u) for u in draws[:3]), want))


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_tie_cases_are_the_ones_the_rule_decides(name):
    r = E.realise(name)
    changed = changed_by_reversed_ties(r.logits, r.case.T, r.case.k, r.top_p, r.draws, r.cut, r.want)
    assert changed == (name in E.TIE_CASES)


def test_the_table_reaches_what_it_is_for():
    names = {c.name for c in E.CASES}
    assert E.TIE_CASES <= names and set(E.PAD_CASES) <= names
    for kind in E.TIE_KINDS:                                            # every tie row decides in several settings
        assert sum(n.startswith(kind) for n in E.TIE_CASES) >= 2, kind
    assert {c.V for c in E.CASES if c.kind == "gauss"} == set(E.GAUSS_V)
    assert any(c.V == 32769 and c.k == 4097 for c in E.CASES)
    for n in (2048, 2049):
        row = E.make_row(f"max{n}", E.TIE_V)
        assert int((row == row.max()).sum()) == n
        # every wave's segment of the kernel (16 waves, segments of 64-multiples) holds some of them
        seg = ((E.TIE_V + 15) // 16 + 63) // 64 * 64
        assert all((row[w * seg:(w + 1) * seg] == row.max()).any() for w in range((E.TIE_V + seg - 1) // seg))
    # zeros: lowest-index-first and "+0.0 before -0.0" keep different survivors at k = 40
    z = E.make_row("zeros", E.TIE_V)
    low = R.survivors(z, 1.0, 40).idx
    plus_first = np.sort(np.lexsort((np.arange(z.size), np.signbit(z), -z))[:40])
    assert np.signbit(z[low]).any() and not np.array_equal(low, plus_first)
    # clip at k = 700: the kept ties span several waves' segments
    c = R.survivors(E.make_row("clip", E.TIE_V), 0.7, 700).idx
    assert len(set((c // seg).tolist())) >= 3


def test_step_rows_are_decidable_and_stream_one_is_a_tie_row():
    for T, k in E.STEP_SETTINGS:
        logits, draws, want = E.step_rows(T, k)
        assert all(d.decided for d in want.values())
        for m in range(E.STEP_M):
            assert len({want[m, t].token for t in range(4)}) >= 3
    T, k = E.STEP_SETTINGS[0]
    logits, draws, want = E.step_rows(T, k)
    row = R.survivors(logits[1], T, k)
    assert changed_by_reversed_ties(logits[1], T, k, 1.0, draws[1], R.top_p_cut(row, 1.0), [want[1, t] for t in range(3)])
    # each stream passes t < 0, 0, a middle value, stride - 1 and stride
    for m in range(E.STEP_M):
        ts = {E.step_t(c, a, m) for c, a in E.STEP_LAUNCHES}
        assert {-1, 0, E.STEP_STRIDE - 1, E.STEP_STRIDE} <= ts and ts & set(range(1, E.STEP_STRIDE - 1))
