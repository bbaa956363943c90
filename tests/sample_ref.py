"""Test helper: a plain NumPy statement of the device sampler's contract (include/ti_hip.h, "on-device
sampling"; sample.hip).  Not a port of the oracle: every tie is decided here, by the documented rule.

  temperature  fp32 / fp32 unless T == 1 or T <= 0
  top-k        order by (value descending, index ascending), values compared as numbers (-0.0 == +0.0);
               keep k; the survivors stay in index order
  softmax      exp(v - max) in fp32; every sum strictly sequential fp32 in index order (a cumsum's last element)
  top-p        (top_p < 1) order by (probability descending, survivor position ascending); cut at the first
               running sum >= top_p, zero the rest, re-sum in index order, divide if the sum is positive
  draw         u <= 0: token 0, log p[0] if token 0 survived else -inf; otherwise the first survivor whose
               running sum satisfies u <= cum; none: token V - 1, -inf unless it survived

  survivors(logits, T, k)            -> Row: idx (ascending), p (softmax over the survivors), V
  sorted_cumsum(row)                 -> the running sums of the probabilities in top-p order
  top_p_cut(row, top_p)              -> Row after the cut + the top-p margin and the rank gap at the cut
  draw(row, u)                       -> Draw(token, logprob, margin, decided, alt)
  sample(logits, T, k, top_p, u)     -> Draw, the whole sampler for one draw
  place_draw(row, which)             -> a draw in the middle of a chosen survivor's interval
  place_top_p(sorted_cs, near)       -> a top_p in the middle of the gap between two running sums next to `near`

What makes a case comparable with an implementation whose exp / log are within 1 ulp of these (a moved sum is
relative 1e-6 at the most, test_gpu_sample.py):
  draw margin   distance from u to the nearest cumulative boundary (0 included)
  top-p margin  distance from top_p to the nearest sorted running sum
  rank gap      relative difference between the last kept and the first dropped probability at the top-p cut;
                exactly 0.0 when the two come from equal logits (then both sides compute the same bits and the
                index rule decides)
Draw.decided is margin >= MARGIN, with two cases of its own.  u <= 0 is decided by its rule, no sum involved.  A
draw at or past the last boundary (u = 1: the last running sum is 1 give or take an ulp) is decided only when both
sides of that boundary give the same answer, i.e. when the last survivor that kept probability is token V - 1 (the
margin is then taken to the boundary before it), or when every survivor has the same logit (`Row.exact`: all
exp(0) = 1, nothing but correctly rounded adds and divides of equal numbers).  Otherwise Draw.alt holds the
answer of the other side: (V - 1, -inf or log p[V - 1]) against the last survivor with probability.

`_ties_high` reverses the tie rule (highest index first, in top-k and in top-p); test_sample_ref.py uses it to
prove that a case labelled as a tie case is one the rule decides.  Nothing else may pass it.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

f32 = np.float32
MARGIN = 1e-5          # ten times the 1e-6 boundary sensitivity of an exp / log within 1 ulp
MIN_PLACED_P = 4e-5    # place_draw picks among survivors at least this probable: margin >= 2e-5

Row = namedtuple("Row", "idx p V exact v")
Cut = namedtuple("Cut", "row top_p_margin rank_gap")
Draw = namedtuple("Draw", "token logprob margin decided alt")


def seq_sum(x):
    return np.cumsum(x, dtype=f32)[-1]


def survivors(logits, T, k, _ties_high=False):
    v = np.asarray(logits, f32).reshape(-1)
    V = v.size
    assert 1 <= k <= V
    T = f32(T)
    if T != 1 and T > 0:
        v = (v / T).astype(f32)
    ar = np.arange(V)
    order = np.lexsort((-ar if _ties_high else ar, -v))        # value descending, then the index rule
    idx = np.sort(order[:k])
    s = v[idx]
    e = np.exp((s - s.max()).astype(f32)).astype(f32)
    p = (e / seq_sum(e)).astype(f32)
    return Row(idx, p, V, bool(np.all(s == s[0])), s)


def _top_p_order(row, _ties_high=False):
    pos = np.arange(row.p.size)
    return np.lexsort((-pos if _ties_high else pos, -row.p))


def sorted_cumsum(row, _ties_high=False):
    return np.cumsum(row.p[_top_p_order(row, _ties_high)], dtype=f32)


def top_p_cut(row, top_p, _ties_high=False):
    top_p = f32(top_p)
    if not top_p < 1:
        return Cut(row, np.inf, np.inf)
    order = _top_p_order(row, _ties_high)
    cs = np.cumsum(row.p[order], dtype=f32)
    hit = np.flatnonzero(cs >= top_p)
    cut = int(hit[0]) + 1 if hit.size else order.size
    p = row.p.copy()
    p[order[cut:]] = 0
    s = seq_sum(p)
    if s > 0:
        p = (p / s).astype(f32)
    margin = float(np.min(np.abs(cs.astype(np.float64) - float(top_p))))
    gap = np.inf
    if cut < order.size:
        a, b = order[cut - 1], order[cut]
        if row.v[a] == row.v[b]:
            gap = 0.0
        else:       # (different logits: never "exactly equal", whatever fp32 made of their exps)
            gap = max(float(row.p[a] - row.p[b]) / float(row.p[a]), float(np.finfo(f32).tiny))
    return Cut(row._replace(p=p), margin, gap)


def draw(row, u):
    u = f32(u)
    idx, p, V = row.idx, row.p, row.V
    if u <= 0:
        lp = np.log(p[0]) if idx[0] == 0 and p[0] > 0 else f32(-np.inf)
        return Draw(0, float(lp), np.inf, True, None)
    cum = np.cumsum(p, dtype=f32)
    hit = np.flatnonzero(u <= cum)
    fall = (V - 1, float(np.log(p[-1])) if idx[-1] == V - 1 and p[-1] > 0 else -np.inf)
    live = np.flatnonzero(p > 0)
    last = int(live[-1])
    bounds = np.concatenate(([0.0], cum[live].astype(np.float64)))
    if hit.size:
        j = int(hit[0])
        got = (int(idx[j]), float(np.log(p[j])))
    else:
        j, got = -1, fall
    alt = None
    if j == last or j < 0:
        # next to the last boundary: the other side of it
        other = fall if j == last else (int(idx[last]), float(np.log(p[last])))
        if other == got:
            bounds = bounds[:-1]
        else:
            alt = other
    margin = float(np.min(np.abs(bounds - float(u))))
    if row.exact:
        margin, alt = np.inf, None
    return Draw(got[0], got[1], margin, margin >= MARGIN, alt if margin < MARGIN else None)


def sample(logits, T, k, top_p, u, _ties_high=False):
    return draw(top_p_cut(survivors(logits, T, k, _ties_high), top_p, _ties_high).row, u)


def place_draw(row, which):
    """The fp32 midpoint of the cumulative interval of one survivor: the 'first', 'middle' or 'last' of those
    with probability >= MIN_PLACED_P, or the 'top' (most probable) one -- also when none is that probable."""
    cum = np.concatenate(([f32(0)], np.cumsum(row.p, dtype=f32)))
    big = np.flatnonzero(row.p >= MIN_PLACED_P)
    if which == "top" or big.size == 0:
        j = int(np.argmax(row.p))
    else:
        j = int(big[{"first": 0, "middle": big.size // 2, "last": -1}[which]])
    return f32((np.float64(cum[j]) + np.float64(cum[j + 1])) / 2)


def place_top_p(sorted_cs, near):
    """The fp32 midpoint between the two adjacent sorted running sums (0 before the first) that bracket `near`,
    moved down to the last pair that lies below 1: a placed top_p always cuts."""
    cs = np.concatenate(([0.0], np.asarray(sorted_cs, np.float64)))
    j = int(np.clip(np.searchsorted(cs, near), 1, cs.size - 1))
    while j > 1 and not (cs[j - 1] + cs[j]) / 2 < 1.0 - 1e-6:
        j -= 1
    while j > 1 and cs[j] == cs[j - 1]:
        j -= 1
    return f32((cs[j - 1] + cs[j]) / 2)
