"""Test helper: a plain-Python model of lookahead greedy decoding's bookkeeping (include/ti_hip.h
ti_lookahead_begin / ti_lookahead_accept, ti_engine_generate_lookahead).  Lists and loops only: the draft rule is
the literal one of the header (longest suffix first, then the most recent match), nothing of the kernel's
single-reduction form.

  draft(hist, ngram, keff)          -> the drafted tokens of a step
  begin(state, hist, k, ngram, max_new, max_pos) -> (row_tok [k + 1], pos [k + 1], nd)
  accept(state, hist, out, row_tok, greedy, k, max_new, stop) updates state / hist / out in place
  simulate(prompt, corpus, G, k, ngram, max_new, stop) -> (tokens, stats) for the greedy continuation G

state: dict(hist_len, pos, produced, done, steps, drafted, accepted, nd) -- the eight device words.
"""
from __future__ import annotations

STATE = ("hist_len", "pos", "produced", "done", "steps", "drafted", "accepted", "nd")


def draft(hist, ngram, keff):
    """For g from min(ngram, L - 1) down to 1: the largest i <= L - g - 1 with hist[i : i + g] == hist[L - g : L]
    gives hist[i + g : min(i + g + keff, L)]; no match or keff < 1: no drafts."""
    L = len(hist)
    if keff < 1:
        return []
    for g in range(min(ngram, L - 1), 0, -1):
        suffix = hist[L - g:L]
        for i in range(L - g - 1, -1, -1):
            if hist[i:i + g] == suffix:
                return list(hist[i + g:min(i + g + keff, L)])
    return []


def begin(state, hist, k, ngram, max_new, max_pos=1 << 30):
    """The head of a step: rows' tokens and positions; state['nd'] is set unless done."""
    L = state["hist_len"]
    h = list(hist[:L])
    d = [] if state["done"] else draft(h, ngram, min(k, max_new - state["produced"] - 1))
    row_tok = [h[L - 1]] + d + [h[L - 1]] * (k - len(d))
    pos = [min(state["pos"] + j, max_pos) for j in range(k + 1)]
    if not state["done"]:
        state["nd"] = len(d)
    return row_tok, pos, len(d)


def accept(state, hist, out, row_tok, greedy, k, max_new, stop=-1):
    """greedy[j] = row j's greedy token.  hist and out are lists indexed by position (long enough)."""
    if state["done"]:
        return
    nd, L, produced = state["nd"], state["hist_len"], state["produced"]
    a = 0
    while a < nd and row_tok[a + 1] == greedy[a]:
        a += 1
    n, done = 0, 0
    while n <= a and produced + n < max_new:
        tok = greedy[n]
        hist[L + n] = tok
        out[produced + n] = tok
        n += 1
        if stop >= 0 and tok == stop:
            done = 1
            break
    if produced + n >= max_new:
        done = 1
    state["hist_len"] = L + n
    state["pos"] += n
    state["produced"] = produced + n
    state["done"] = done
    state["steps"] += 1
    state["drafted"] += nd
    state["accepted"] += min(n, a)


def simulate(prompt, corpus, G, k, ngram, max_new, stop=-1):
    """The whole request against a model whose greedy continuation of `prompt` is G (len(G) >= max_new): row j of
    a step is fed its token after the rows before it, so while the drafts are right its greedy token is the next
    token of G, and the first wrong draft's row still predicts the right token.  -> (tokens [max_new] padded
    with -1 after a stop token, stats dict, per-step emitted counts)."""
    corpus = list(corpus or [])
    cap = len(corpus) + len(prompt) + max_new
    hist = corpus + list(prompt) + [0] * max_new
    out = [-1] * max_new
    state = dict.fromkeys(STATE, 0)
    state["hist_len"] = len(corpus) + len(prompt)
    state["pos"] = len(prompt) - 1
    emitted = []
    while not state["done"] and state["steps"] < max_new:
        row_tok, _, nd = begin(state, hist, k, ngram, max_new)
        p = state["produced"]
        # row j sees G[:p + j] only if rows 1 .. j are G[p : p + j]; a row behind a wrong draft is never read
        greedy = []
        for j in range(k + 1):
            ok = j <= nd and all(row_tok[i + 1] == G[p + i] for i in range(j))
            greedy.append(G[p + j] if ok else -7)
        before = state["produced"]
        accept(state, hist, out, row_tok, greedy, k, max_new, stop)
        emitted.append(state["produced"] - before)
    assert state["hist_len"] <= cap
    stats = dict(steps=state["steps"], drafted=state["drafted"], accepted=state["accepted"], produced=state["produced"])
    return out, stats, emitted
