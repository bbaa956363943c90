"""NumPy restatement of token-automaton guided decoding (ti_engine.h ti_guide, ti_hip.h ti_guide_step), and the
shared automata of the guide tests.

A guide is (row_ptr, tokens, next, start): state s allows tokens[row_ptr[s] : row_ptr[s + 1]] (strictly ascending)
and moves to the next entry beside the token it consumes.  A slot's state is an int, -1 = free or dead.
    advance(g, s, tok): s < 0 or tok < 0 -> s; the transition's next state; -1 when s has none on tok
    mask(g, s, row):    s < 0 -> the row's bits; else -inf (0xFF800000) at every id s does not allow
    run(g, tokens):     the states a request passes through, from start, and whether every token was allowed"""
from __future__ import annotations

import numpy as np

f32, i32, i64 = np.float32, np.int32, np.int64
NEG_INF_BITS = 0xFF800000


class Guide:
    def __init__(self, rows, start=0):
        """rows: per state, a list of (token, next state) pairs (any order; stored ascending by token)."""
        rows = [sorted(r) for r in rows]
        self.row_ptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(i64)
        self.tokens = np.array([t for r in rows for t, _ in r], i32)
        self.next = np.array([n for r in rows for _, n in r], i32)
        self.start = start
        self.n_states = len(rows)

    @property
    def csr(self):
        return self.row_ptr, self.tokens, self.next

    @property
    def args(self):
        return self.row_ptr, self.tokens, self.next, self.start

    def allowed(self, s) -> np.ndarray:
        return self.tokens[self.row_ptr[s]: self.row_ptr[s + 1]]

    def bitmask(self, V) -> np.ndarray:
        """uint32 [n_states][ceil(V / 32)]: bit (v & 31) of word (v >> 5) set iff the state allows v."""
        W = (V + 31) // 32
        m = np.zeros((self.n_states, W), np.uint32)
        for s in range(self.n_states):
            a = self.allowed(s).astype(np.int64)
            np.bitwise_or.at(m[s], a >> 5, (np.uint32(1) << (a & 31).astype(np.uint32)))
        return m


def check(g: Guide, V: int) -> str | None:
    """None when g meets the contract for a vocabulary of V ids, else what it violates."""
    n = g.n_states
    if n < 1:
        return "n_states"
    if not 0 <= g.start < n:
        return "start"
    rp = g.row_ptr
    if len(rp) != n + 1 or rp[0] != 0 or np.any(np.diff(rp) < 0) or rp[-1] != len(g.tokens) or len(g.tokens) != len(g.next):
        return "row_ptr"
    for s in range(n):
        a = g.allowed(s)
        if a.size == 0:
            return "empty state"
        if a.min() < 0 or a.max() >= V:
            return "token range"
        if np.any(np.diff(a.astype(i64)) <= 0):
            return "order"
    if g.next.min() < 0 or g.next.max() >= n:
        return "next range"
    return None


def advance(g: Guide, s: int, tok: int) -> int:
    if s < 0 or tok < 0:
        return s
    a = g.allowed(s)
    i = int(np.searchsorted(a, tok))
    return int(g.next[g.row_ptr[s] + i]) if i < a.size and a[i] == tok else -1


def mask(g: Guide, s: int, row) -> np.ndarray:
    out = np.array(row, f32).reshape(-1)
    if s < 0:
        return out
    keep = np.zeros(out.size, bool)
    keep[g.allowed(s)] = True
    out.view(np.uint32)[~keep] = NEG_INF_BITS
    return out


def run(g: Guide, tokens):
    """-> (states, accepted): states[i] is the state token i was drawn in (states[0] = start), states[len(tokens)]
    the state after the last; accepted iff no state on the way is dead."""
    states = [g.start]
    for t in tokens:
        states.append(advance(g, states[-1], int(t)))
    return states, all(s >= 0 for s in states)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the four automata of the engine tests (vocab 1024)
FORCED = [17, 901, 3, 3, 512, 1023]


def forced(V, path=FORCED) -> Guide:
    """A chain of one-transition states, then a free state."""
    n = len(path)
    return Guide([[(t, i + 1)] for i, t in enumerate(path)] + [[(v, n) for v in range(V)]])


def cycle(V, n=3) -> Guide:
    """State i allows the ids = i (mod n) and moves to i + 1 (mod n)."""
    return Guide([[(v, (i + 1) % n) for v in range(i, V, n)] for i in range(n)])


def ban(V, banned) -> Guide:
    """One state that omits some ids."""
    banned = set(banned)
    return Guide([[(v, 0) for v in range(V) if v not in banned]])


def digits_then_stop(digits, stop) -> Guide:
    """A digit; then digits or the stop token; behind the stop token only the stop token."""
    return Guide([[(d, 1) for d in digits], [(d, 1) for d in digits] + [(stop, 2)], [(stop, 2)]])
