"""ti_lookahead_begin / ti_lookahead_accept (lookahead.hip) stand-alone against the plain-Python model of
tests/lookahead_ref.py.  Histories over a 4-symbol alphabet (many matches of every length) of 1, 2, 17, 1025 and
20000 tokens -- fewer than, exactly and many times the workgroup's 1024 candidates per pass --, ngram 1 / 3 / 8,
k 1 / 4 / 15, matches whose followers run out before k, Keff cut by max_new; accept with hand-written argmax keys
spread over the slots.  Everything compared is exact: row_tok, pos, the h rows (the fp16 embedding table as
fp32), the cleared keys, the state words, hist and out_tokens."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import lookahead_ref as R

pytestmark = pytest.mark.gpu

VOCAB, HIDDEN, SLOTS = 8, 72, 32      # hidden % 8 == 0: the 16-byte gather; test_begin_scalar_gather takes 36
EMB = (np.arange(VOCAB * HIDDEN, dtype=np.float32).reshape(VOCAB, HIDDEN) / 64 - 3).astype(np.float16)


class Rig:
    """Device buffers of one ti_lookahead_args."""

    def __init__(self, ti, k, cap, max_new, hidden=HIDDEN, max_pos=1 << 20):
        self.ti, self.k, self.cap, self.max_new, self.hidden = ti, k, cap, max_new, hidden
        self.emb_h = np.ascontiguousarray(EMB[:, :hidden])
        D = ti.DeviceBuffer
        self.state, self.cfg, self.hist = D(32), D(16), D(4 * cap)
        self.emb = D.from_array(self.emb_h)
        self.h, self.row_tok, self.pos = D(4 * (k + 1) * hidden), D(4 * (k + 1)), D(4 * (k + 1))
        self.argmax, self.out = D(8 * (k + 1) * SLOTS), D(4 * max_new)
        self.args = ti.LookaheadArgs(state=self.state.ptr, cfg=self.cfg.ptr, hist=self.hist.ptr, k=k, hidden=hidden,
                                     vocab=VOCAB, max_pos=max_pos, emb=self.emb.ptr, h=self.h.ptr,
                                     row_tok=self.row_tok.ptr, pos=self.pos.ptr, argmax=self.argmax.ptr,
                                     out_tokens=self.out.ptr)

    def put(self, state, hist, ngram, stop=-1, out=None):
        self.state.upload(np.array([state[n] for n in R.STATE], np.int32))
        self.cfg.upload(np.array([ngram, self.max_new, stop, self.cap], np.int32))
        hh = np.full(self.cap, 5, np.int32)
        hh[:len(hist)] = hist
        self.hist.upload(hh)
        self.out.upload(np.full(self.max_new, -9, np.int32) if out is None else np.asarray(out, np.int32))

    def get_state(self):
        return dict(zip(R.STATE, self.state.download(np.int32, 8).tolist()))


def fresh_state(L, pos, produced=0, done=0):
    st = dict.fromkeys(R.STATE, 0)
    st.update(hist_len=L, pos=pos, produced=produced, done=done, nd=-1)
    return st


def check_begin(ti, rig, state, hist, ngram):
    rig.put(state, hist, ngram)
    rig.argmax.upload(np.full((rig.k + 1) * SLOTS, 0xDEADBEEF12345678, np.uint64))
    rig.h.upload(np.full((rig.k + 1) * rig.hidden, -77.0, np.float32))
    ti.check(ti.lib().ti_lookahead_begin(C.byref(rig.args), None))
    ti.sync()
    want = dict(state)
    row_tok, pos, nd = R.begin(want, list(hist), rig.k, ngram, rig.max_new, rig.args.max_pos)
    assert rig.row_tok.download(np.int32, rig.k + 1).tolist() == row_tok
    assert rig.pos.download(np.int32, rig.k + 1).tolist() == pos
    assert rig.get_state() == want
    assert not rig.argmax.download(np.uint64, (rig.k + 1) * SLOTS).any()
    h = rig.h.download(np.float32, (rig.k + 1, rig.hidden))
    assert np.array_equal(h, rig.emb_h[np.asarray(row_tok)].astype(np.float32))
    assert np.array_equal(rig.hist.download(np.int32, len(hist)), np.asarray(hist, np.int32))
    return nd


@pytest.mark.parametrize("k", [1, 4, 15])
@pytest.mark.parametrize("ngram", [1, 3, 8])
@pytest.mark.parametrize("L", [1, 2, 17, 1025, 20000])
def test_begin_matches_the_model(ti, L, ngram, k):
    rng = np.random.default_rng([L, ngram, k])
    max_new = 40
    rig = Rig(ti, k, L + max_new, max_new)
    seen = set()
    for trial in range(4):
        hist = rng.integers(0, 4, L).tolist()
        if trial == 1 and L > 8:          # the only long match sits at the very start
            hist[L - 8:] = hist[:8]
        if trial == 2 and L > 2:          # the followers of the most recent match run out before k
            hist[L - 2] = hist[L - 1] = 6
        if trial == 3:                    # no match at all: the last token is new
            hist[L - 1] = 7
        produced = max_new - 3 if trial == 1 else 0      # trial 1: Keff = 2 whatever k
        nd = check_begin(ti, rig, fresh_state(L, 100 + trial, produced), hist, ngram)
        seen.add(nd)
    if L >= 17:
        assert 0 in seen and max(seen) >= 1


def test_begin_keff_cut_by_max_new_and_done(ti):
    hist = [1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3]
    for k in (4, 15):
        rig = Rig(ti, k, 64, 10, max_pos=25)
        assert check_begin(ti, rig, fresh_state(11, 20, produced=0), hist, 3) == min(k, 4)   # followers: 4 before L
        assert check_begin(ti, rig, fresh_state(11, 20, produced=7), hist, 3) == 2           # Keff = 10 - 7 - 1
        assert check_begin(ti, rig, fresh_state(11, 20, produced=9), hist, 3) == 0           # Keff = 0
        st = fresh_state(11, 20, produced=10, done=1)
        st["nd"] = 3
        assert check_begin(ti, rig, st, hist, 3) == 0        # done: padding rows, positions clamped at max_pos
        assert rig.get_state()["nd"] == 3


def test_begin_scalar_gather(ti):
    rig = Rig(ti, 4, 64, 10, hidden=36)
    check_begin(ti, rig, fresh_state(6, 3), [1, 2, 1, 2, 1, 2], 3)


def key_of(value, token):
    """A TI_EPI_LOGITS_ARGMAX key: order-preserving bits of the logit << 32 | 0xFFFFFFFF - token."""
    b = int(np.float32(value).view(np.uint32))
    b = b ^ 0xFFFFFFFF if b & 0x80000000 else b | 0x80000000
    return (b << 32) | (0xFFFFFFFF - token)


def keys_for(k, greedy, rng):
    """Row j's winning key in a slot of its own choice, smaller keys of other tokens around it."""
    am = np.zeros((k + 1, SLOTS), np.uint64)
    for j, g in enumerate(greedy):
        for s in rng.choice(SLOTS, 5, replace=False):
            am[j, s] = key_of(float(rng.uniform(-3, 1)), int(rng.integers(0, VOCAB)))
        am[j, (7 * j + 3) % SLOTS] = key_of(2.5, g)
    return am


ACCEPT = [
    # name, k, drafts (rows 1 ..), greedy per row, produced, max_new, stop, done
    ("none_accepted", 4, [1, 2, 3], [5, 2, 3, 4, 0], 2, 20, -1, 0),
    ("partial", 4, [1, 2, 3, 4], [1, 2, 6, 4, 0], 2, 20, -1, 0),
    ("full", 4, [1, 2, 3, 4], [1, 2, 3, 4, 7], 2, 20, -1, 0),
    ("full_k15", 15, list(range(15)), [i % 8 for i in range(15)] + [3], 0, 40, -1, 0),
    ("no_drafts", 4, [], [6, 0, 0, 0, 0], 2, 20, -1, 0),
    ("stop_inside_run", 4, [1, 2, 3, 4], [1, 2, 3, 4, 7], 2, 20, 2, 0),
    ("stop_is_bonus", 4, [1, 2], [1, 2, 7, 0, 0], 2, 20, 7, 0),
    ("max_new_reached", 4, [1, 2, 3], [1, 2, 3, 5, 0], 16, 20, -1, 0),
    ("done_on_entry", 4, [1, 2, 3], [1, 2, 3, 5, 0], 5, 20, -1, 1),
]


@pytest.mark.parametrize("case", ACCEPT, ids=[c[0] for c in ACCEPT])
def test_accept_matches_the_model(ti, case):
    name, k, drafts, greedy, produced, max_new, stop, done = case
    drafts = [d % VOCAB for d in drafts]
    rng = np.random.default_rng(len(name))
    L, cap = 9, 9 + max_new
    hist = rng.integers(0, 4, L).tolist()
    rig = Rig(ti, k, cap, max_new)
    st = fresh_state(L, 50, produced, done)
    st.update(nd=len(drafts), steps=3, drafted=11, accepted=4)
    out0 = rng.integers(0, VOCAB, max_new).tolist()
    rig.put(st, hist, 3, stop, out0)
    row_tok = [hist[-1]] + drafts + [hist[-1]] * (k - len(drafts))
    rig.row_tok.upload(np.asarray(row_tok, np.int32))
    rig.argmax.upload(keys_for(k, greedy, rng))
    ti.check(ti.lib().ti_lookahead_accept(C.byref(rig.args), None))
    ti.sync()
    want, whist, wout = dict(st), hist + [5] * (cap - L), list(out0)
    R.accept(want, whist, wout, row_tok, greedy, k, max_new, stop)
    assert rig.get_state() == want
    assert rig.hist.download(np.int32, cap).tolist() == whist
    assert rig.out.download(np.int32, max_new).tolist() == wout
    if name == "stop_inside_run":
        assert want["done"] == 1 and want["produced"] == produced + 2 and want["accepted"] == 4 + 2
    if name == "max_new_reached":
        assert want["done"] == 1 and want["produced"] == 20
    if name == "full":
        assert want["produced"] == produced + 5 and want["accepted"] == 4 + 4 and not want["done"]
