"""Test helper: the rows and the case table of the sampler edge tests (test_gpu_sample_edges.py on the GPU,
test_sample_ref.py for the reference side on the CPU).  numpy only; every row comes from a RandomState.

Row kinds (one row of V logits each):
  max2048  exactly 2048 entries equal the row maximum (index V - 1 among them), scattered over every wave's
           segment, the rest at least 3 below: C_tot == kCand, the last row that stays on the candidate path
           (at top_k 40 and 700; at 1024 fewer than 1024 threads own an element of a 4099-entry row, the k-th
           thread maximum is the empty key, all V keys are candidates and the radix select takes over)
  max2049  the same with 2049: the first row of the radix fallback at top_k <= 1024
  clip     min(normal * 3, 1.5): about 1300 of 4099 at the maximum
  quant    round(normal * 6) / 2: about 40 distinct values, ties at every rank
  zeros    -|normal * 3| with 300 +0.0 and 300 -0.0 scattered as the maximum (the two signs interleaved, so
           "every +0.0 before any -0.0" and "lowest index first" keep different survivors)
  gauss    normal * 3, its maximum moved to index V - 1 (so u = 1 has one answer, sample_ref.py)

A case is (row kind, V, T, top_k, `near`); near = 1: top_p = 1, else top_p is placed next to `near`
(placed_top_p).  Every case runs five draws: three placed (first / middle / last survivor with probability
>= 4e-5), u = 0 and u = 1.  TIE_CASES names the cases in which the tie rule decides something (checked both ways
by test_sample_ref.py: reversing the rule changes a survivor set, a token or a log p there and nowhere else).
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import sample_ref as R

f32 = np.float32
MAX_K = 4096                     # TI_SAMPLE_MAX_K: above it the survivors live in the HBM workspace
TIE_V = 4099                     # not a multiple of 4
DRAWS = ("first", "middle", "last")

Case = namedtuple("Case", "name kind V T k near")


def make_row(kind, V, seed=0):
    rng = np.random.RandomState(7919 * seed + V + sum(map(ord, kind)))
    g = rng.standard_normal(V)
    if kind == "gauss":
        row = (g * 3).astype(f32)
        j = int(np.argmax(row))
        row[j], row[V - 1] = row[V - 1], row[j]
    elif kind in ("max2048", "max2049"):
        n = int(kind[3:])
        row = (-3.0 - np.abs(g)).astype(f32)
        at = rng.permutation(V - 1)[:n - 1]
        row[at] = 2.0
        row[V - 1] = 2.0
        assert int((row == row.max()).sum()) == n
    elif kind == "clip":
        row = np.minimum(g * 3, 1.5).astype(f32)
        row[V - 1] = 1.5
    elif kind == "quant":
        row = (np.round(g * 6) / 2).astype(f32)
        row[V - 1] = row.max()
    elif kind == "zeros":
        row = (-np.abs(g * 3) - 1e-3).astype(f32)
        at = np.sort(rng.permutation(V - 1)[:599])
        at = np.concatenate((at, [V - 1]))
        row[at[0::2]] = 0.0
        row[at[1::2]] = -0.0
        assert int(((row == 0) & ~np.signbit(row)).sum()) == 300 and int(((row == 0) & np.signbit(row)).sum()) == 300
    else:
        raise ValueError(kind)
    return row


TIE_SETTINGS = [(1.0, 40, 1.0), (0.7, 700, 0.9), (1.0, 1024, 0.5), (1.3, 2500, 0.95), (1.0, TIE_V, 0.8)]
TIE_KINDS = ("max2048", "max2049", "clip", "quant", "zeros")
GAUSS_V = (1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049, 32768, 32769)


def _cases():
    out = []
    for kind in TIE_KINDS:
        for T, k, near in TIE_SETTINGS:
            out.append(Case(f"{kind}-T{T}-k{k}-p{near}", kind, TIE_V, T, k, near))
    for V in GAUSS_V:
        ks = sorted({1, min(V, 8)} | ({V} if V <= MAX_K else set()))
        if V == 32769:
            ks.append(4097)                      # uncached keys and HBM survivors together
        for k in ks:
            for near in (1.0, 0.9):
                out.append(Case(f"gauss-V{V}-k{k}-p{near}", "gauss", V, 1.0 if k != 8 else 0.8, k, near))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# the cases on tie rows that the tie rule decides (in the others the k-th place and the top-p cut fall between two
# different values: every entry of the tied groups above them survives both)
TIE_CASES = frozenset(c.name for c in CASES if c.kind in TIE_KINDS) - frozenset((
    "clip-T1.3-k2500-p0.95", "clip-T1.0-k4099-p0.8", "quant-T1.0-k40-p1.0", "quant-T1.0-k1024-p0.5",
    "zeros-T0.7-k700-p0.9", "zeros-T1.3-k2500-p0.95", "zeros-T1.0-k4099-p0.8"))
PAD = 37
PAD_CASES = ("quant-T0.7-k700-p0.9", "gauss-V1025-k8-p0.9")


def decidable_cut(cut):
    return cut.top_p_margin >= R.MARGIN and (cut.rank_gap == 0.0 or cut.rank_gap >= R.MARGIN)


def placed_top_p(row, near):
    """place_top_p at the pair of sorted running sums nearest `near` whose cut is decidable (top-p margin and rank
    gap, sample_ref.py): nothing is left to the seed."""
    cs = R.sorted_cumsum(row)
    j0 = int(np.searchsorted(cs, near))
    for d in range(cs.size + 1):
        for j in (j0 + d, j0 - d):
            if 0 <= j < cs.size:
                tp = R.place_top_p(cs, cs[j])
                if tp < 1 and decidable_cut(R.top_p_cut(row, tp)):
                    return tp
    raise AssertionError("no decidable top_p")


Real = namedtuple("Real", "case logits top_p draws cut want")


def realise_row(logits, T, k, near):
    """-> (top_p, draws [5], Cut, [Draw] * 5) of one row under the documented rule."""
    row = R.survivors(logits, T, k)
    top_p = f32(1.0) if near >= 1 else placed_top_p(row, near)
    cut = R.top_p_cut(row, top_p)
    draws = np.array([R.place_draw(cut.row, w) for w in DRAWS] + [0.0, 1.0], f32)
    return top_p, draws, cut, [R.draw(cut.row, u) for u in draws]


@functools.lru_cache(maxsize=None)
def realise(name):
    c = BY_NAME[name]
    logits = make_row(c.kind, c.V)
    logits.setflags(write=False)
    return Real(c, logits, *realise_row(logits, c.T, c.k, c.near))


def lp_matches(got, want):
    """log p within 1e-5 * max(1, |log p|); -inf is -inf."""
    if np.isfinite(want):
        return bool(np.isfinite(got)) and abs(float(got) - want) <= 1e-5 * max(1.0, abs(want))
    return float(got) == want


def assert_draw(got_tok, got_lp, d, last, ctx):
    """A sampler's (token, log p) for one draw against the reference's Draw.  `last`: the u = 1 draw, the only
    one that may have two stated answers (sample_ref.py); every other must be decided."""
    assert d.decided or (last and d.alt is not None), (ctx, d)
    answers = [(d.token, d.logprob)] + ([d.alt] if d.alt is not None else [])
    assert any(int(got_tok) == t and lp_matches(got_lp, lp) for t, lp in answers), (ctx, int(got_tok), float(got_lp), d)


# ---- ti_sample_step: M = 3 streams, draw_stride 5, n_in = [1, 3, 6]
STEP_M, STEP_STRIDE, STEP_N_IN, STEP_V = 3, 5, (1, 3, 6), TIE_V
STEP_KINDS = ("gauss", "quant", "clip")          # stream 1 and 2 are tie rows
# (step_ctr, advance): s = step_ctr - advance; stream m's t = s - (n_in[m] - 1) passes -1, 0, a middle value,
# draw_stride - 1 and draw_stride for every m
STEP_LAUNCHES = ((0, 1), (0, 0), (2, 1), (5, 3), (4, 0), (6, 1), (9, 3), (7, 0), (12, 3), (10, 0))
STEP_SETTINGS = ((0.8, 40), (1.0, STEP_V))       # the second: top_k > TI_SAMPLE_MAX_K, ti_sample_step_ws


def step_t(ctr, adv, m):
    return (ctr - adv) - (STEP_N_IN[m] - 1)


@functools.lru_cache(maxsize=None)
def step_rows(T, k):
    """-> logits [M][V], draws [M][stride] (each placed in its row: first, middle, last, top, first), the
    reference's Draw for every (m, t)."""
    logits = np.stack([make_row(kind, STEP_V, seed=1) for kind in STEP_KINDS])
    draws = np.zeros((STEP_M, STEP_STRIDE), f32)
    want = {}
    for m in range(STEP_M):
        row = R.survivors(logits[m], T, k)
        for t, w in enumerate(("first", "middle", "last", "top", "first")):
            draws[m, t] = R.place_draw(row, w)
            want[m, t] = R.draw(row, draws[m, t])
    logits.setflags(write=False)
    return logits, draws, want
