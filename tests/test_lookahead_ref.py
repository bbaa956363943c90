"""The plain-Python model of lookahead decoding (tests/lookahead_ref.py), the reference the GPU tests of
ti_lookahead_begin / ti_lookahead_accept / ti_engine_generate_lookahead compare with: the draft rule's two tie
rules, and the properties of a whole request -- the output is the greedy sequence whatever the corpus, every step
emits between 1 and k + 1 tokens, steps <= max_new, truncation at a stop token and at max_new."""
from __future__ import annotations

import numpy as np
import pytest

import lookahead_ref as R


def test_longest_suffix_wins():
    # suffix (1, 2, 3): the 1-gram and 2-gram matches later in the text lose against the 3-gram at index 0
    hist = [1, 2, 3, 9, 8, 2, 3, 7, 3, 6, 1, 2, 3]
    assert R.draft(hist, 3, 2) == [9, 8]
    assert R.draft(hist, 2, 2) == [7, 3]      # ngram 2: the most recent (2, 3), index 5
    assert R.draft(hist, 1, 2) == [6, 1]      # ngram 1: the most recent 3, index 8


def test_most_recent_match_wins():
    hist = [5, 6, 1, 5, 6, 2, 5, 6, 3, 5, 6]
    assert R.draft(hist, 2, 1) == [3]
    assert R.draft(hist, 8, 3) == [3, 5, 6]   # no longer suffix matches: falls through to (5, 6)


def test_followers_run_out_and_no_match():
    assert R.draft([4, 4], 3, 5) == [4]                 # i = 0, one follower before L
    assert R.draft([7, 1, 7], 3, 4) == [1, 7]           # followers stop at L
    assert R.draft([1, 2, 3], 3, 4) == []               # the last token never occurred before
    assert R.draft([1], 3, 4) == []
    assert R.draft([1, 1, 1, 1], 2, 0) == []            # no drafts allowed


def test_match_may_overlap_the_suffix():
    # i <= L - g - 1: the match may overlap the suffix itself, but not be it
    assert R.draft([2, 2, 2], 2, 3) == [2]              # g = 2 at i = 0, follower hist[2]


def _rand_case(seed):
    rng = np.random.default_rng(seed)
    vocab = int(rng.integers(3, 9))
    prompt = rng.integers(0, vocab, int(rng.integers(1, 12))).tolist()
    G = rng.integers(0, vocab, 40).tolist()
    corpus = [[], G[:30], rng.integers(0, vocab, 50).tolist(), (prompt + G)[:25]][seed % 4]
    return prompt, corpus, G, int(rng.integers(1, 16)), int(rng.integers(1, 9)), int(rng.integers(1, 41))


@pytest.mark.parametrize("seed", range(200))
def test_simulate_properties(seed):
    prompt, corpus, G, k, ngram, max_new = _rand_case(seed)
    out, st, emitted = R.simulate(prompt, corpus, G, k, ngram, max_new)
    assert out == G[:max_new]
    assert st["produced"] == max_new and sum(emitted) == max_new
    assert 1 <= st["steps"] <= max_new and st["steps"] == len(emitted)
    assert all(1 <= n <= k + 1 for n in emitted)
    assert 0 <= st["accepted"] <= st["drafted"] <= st["steps"] * k
    assert st["accepted"] == max_new - st["steps"]      # every step emits its accepted drafts and one more


@pytest.mark.parametrize("seed", range(60))
def test_simulate_stop_token(seed):
    prompt, corpus, G, k, ngram, max_new = _rand_case(seed)
    stop = G[min(max_new - 1, seed % 7)]
    first = G.index(stop)
    out, st, emitted = R.simulate(prompt, corpus, G, k, ngram, max_new, stop)
    n = min(first + 1, max_new)
    assert out == G[:n] + [-1] * (max_new - n)
    assert st["produced"] == n and st["steps"] <= n and all(1 <= e <= k + 1 for e in emitted)


def test_true_corpus_accepts_and_unrelated_corpus_does_not():
    G = list(range(100, 124))
    prompt = [3, 500, 1023, 17, 250]
    _, st, em = R.simulate(prompt, G, G, 15, 3, 24)
    # step 0 has nothing to match (the prompt's last token is not in the corpus) and emits one token; then the
    # corpus supplies 15 right drafts per step
    assert st["steps"] == 3 and em == [1, 16, 7] and st["accepted"] == 21
    _, st, em = R.simulate(prompt, [], G, 15, 3, 24)
    assert st["steps"] == 24 and st["accepted"] == 0 and st["drafted"] == 0
    _, st, _ = R.simulate(prompt, [900 + i for i in range(50)], G, 4, 3, 24)
    assert st["steps"] == 24 and st["accepted"] == 0


def test_keff_is_cut_by_max_new():
    G = list(range(10, 40))
    out, st, em = R.simulate([9], [9] + G, G, 15, 3, 5)
    assert out == G[:5] and em == [5] and st["drafted"] == 4      # Keff = min(15, 5 - 0 - 1)
    out, st, em = R.simulate([9], [9] + G, G, 2, 3, 5)
    assert em == [3, 2] and st["drafted"] == 2 + 1
    # a run of one token: the most recent match has one follower before the end of the history
    out, st, em = R.simulate([1, 1, 1], [], [1] * 30, 15, 3, 5)
    assert out == [1] * 5 and em == [2, 2, 1] and st["drafted"] == 2


def test_begin_and_accept_with_done_set():
    st = dict.fromkeys(R.STATE, 0)
    st.update(hist_len=4, pos=9, produced=5, done=1, nd=3)
    hist = [1, 2, 1, 2, 0, 0]
    row_tok, pos, nd = R.begin(st, hist, 3, 2, 8, max_pos=10)
    assert row_tok == [2, 2, 2, 2] and pos == [9, 10, 10, 10] and nd == 0 and st["nd"] == 3
    before = dict(st)
    R.accept(st, hist, [0] * 8, row_tok, [5, 5, 5, 5], 3, 8)
    assert st == before and hist == [1, 2, 1, 2, 0, 0]
