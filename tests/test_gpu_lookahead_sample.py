"""ti_lookahead_sample (sample.hip, the sampler's verify-row mode) alone against the ORACLE's sampler
(oracle.sample_token, as tests/test_gpu_sample.py): R = 1 / 5 / 16 rows of seeded logits at V = 1024 and 32000,
state[produced] = 0 and 7, nd = 0 / 2 / R - 1, that file's (T, k, p) grid (the settings with k <= V), one row of
tied logits, one top_k above TI_SAMPLE_MAX_K.  max_new = produced + max(R - 1, 1), so with R > 1 the last row is a
token past the budget.  A live row j (j <= nd, produced + j < max_new, done clear): slot 0 of its argmax slots
holds the feedback key of oracle.sample_token(row, T, k, p, draws[produced + j]), the other slots are as they
were, logprobs[produced + j] is the oracle's to 1e-5.  Every other row's slots and every other logprobs entry are
bit-for-bit what they were pre-filled with; with done set, everything is."""
from __future__ import annotations

import numpy as np
import pytest

import sample_edge_cases as E

pytestmark = pytest.mark.gpu

f32 = np.float32
SLOTS, CAP = 32, 40
GRID = [(1.0, 1, 1.0), (0.7, 40, 0.9), (1.0, 50, 1.0), (1.3, 1024, 0.95), (0.0, 8, 0.5), (1.0, 200, 0.0),
        (1.0, 1500, 1.0), (0.9, 2500, 0.97), (1.0, 4096, 0.9)]
LP_FILL = np.frombuffer(np.array([0xC2F6CDEF], np.uint32).tobytes(), f32)[0]   # a recognisable bit pattern


def key_of(tok):
    return (0xFFFFFFFF << 32) | (0xFFFFFFFF - tok)


class Rig:
    def __init__(self, ti, logits, ws_bytes=0):
        self.ti, self.logits = ti, logits
        self.R, self.V = logits.shape
        D = ti.DeviceBuffer
        self.ld = D.from_array(np.ascontiguousarray(logits))
        self.draws_h = np.random.RandomState(self.R * 7 + self.V).uniform(0, 1, CAP).astype(f32)
        self.dd = D.from_array(self.draws_h)
        self.state, self.cfg = D(32), D(16)
        self.argmax, self.lps = D(8 * self.R * SLOTS), D(4 * CAP)
        self.ws = D(ws_bytes) if ws_bytes else None
        self.keys0 = (np.arange(self.R * SLOTS, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(1)

    def run(self, T, k, p, produced, nd, max_new, done=0):
        """-> (argmax keys [R][SLOTS], logprobs [CAP]) after one launch over pre-filled buffers."""
        self.state.upload(np.array([9, 9, produced, done, 0, 0, 0, nd], np.int32))
        self.cfg.upload(np.array([3, max_new, -1, 1 << 20], np.int32))
        self.argmax.upload(self.keys0)
        self.lps.upload(np.full(CAP, LP_FILL, f32))
        self.ti.check(self.ti.lib().ti_lookahead_sample(self.ld.ptr, self.V, self.R, self.V, T, k, p, self.dd.ptr, CAP,
                                                        self.state.ptr, self.cfg.ptr, self.argmax.ptr, self.lps.ptr,
                                                        self.ws.ptr if self.ws else None, None))
        self.ti.sync()
        return self.argmax.download(np.uint64, (self.R, SLOTS)), self.lps.download(f32, CAP)

    def check(self, oracle, T, k, p, produced, nd, max_new, done=0, rows=None):
        keys, lps = self.run(T, k, p, produced, nd, max_new, done)
        keys0 = self.keys0.reshape(self.R, SLOTS)
        want_lps = np.full(CAP, LP_FILL, f32)
        live = 0
        for j in range(self.R):
            t = produced + j
            if done or j > nd or t >= max_new:
                assert np.array_equal(keys[j], keys0[j]), (j, "a dead row's slots changed")
                continue
            live += 1
            assert np.array_equal(keys[j, 1:], keys0[j, 1:]), (j, "slots 1.. changed")
            if rows is not None and j not in rows:      # (a row the caller compares itself)
                want_lps[t] = lps[t]
                continue
            tok, lp = oracle.sample_token(self.logits[j], T, k, p, float(self.draws_h[t]))
            assert int(keys[j, 0]) == key_of(tok), (T, k, p, j, 0xFFFFFFFF - (int(keys[j, 0]) & 0xFFFFFFFF), tok)
            if np.isfinite(lp):
                assert abs(float(lps[t]) - lp) <= 1e-5 * max(1.0, abs(lp)), (T, k, p, j, lps[t], lp)
            else:
                assert not np.isfinite(lps[t])
            want_lps[t] = lps[t]
        assert np.array_equal(lps.view(np.uint32), want_lps.view(np.uint32)), "a logprobs entry of no live row changed"
        return live


def seeded(R, V):
    return (np.random.RandomState(1000 * R + V).standard_normal((R, V)) * 3).astype(f32)


@pytest.mark.parametrize("produced", [0, 7])
@pytest.mark.parametrize("R", [1, 5, 16])
@pytest.mark.parametrize("V", [1024, 32000])
def test_rows_match_the_oracle_sampler(ti, oracle, V, R, produced):
    rig = Rig(ti, seeded(R, V))
    max_new = produced + max(R - 1, 1)
    for nd in sorted({0, min(2, R - 1), R - 1}):
        for T, k, p in GRID:
            if k > V:
                continue
            live = rig.check(oracle, T, k, p, produced, nd, max_new)
            assert live == min(nd + 1, max_new - produced)
    # done set: nothing at all is written, whatever nd says
    assert rig.check(oracle, 0.7, 40, 0.9, produced, R - 1, max_new, done=1) == 0


def test_budget_and_padding_rows_untouched(ti, oracle):
    """R = 5 at produced 7: max_new 9 leaves rows 0 and 1 live whatever nd allows; nd 0 leaves row 0."""
    rig = Rig(ti, seeded(5, 1024))
    assert rig.check(oracle, 1.0, 50, 1.0, 7, 4, 9) == 2
    assert rig.check(oracle, 1.0, 50, 1.0, 7, 0, 40) == 1
    assert rig.check(oracle, 1.0, 50, 1.0, 7, 4, 7) == 0          # every row past the budget


def test_tied_logits_row(ti, oracle):
    """Row 2 holds every value twice (the second half repeats the first).  Equal logits at the k-th place go
    lowest index first on the device and wherever std::sort leaves them in the reference (test_gpu_sample.py): the
    tied row is compared with the oracle in the settings where the two agree, the other rows always.  In every
    setting the tied row is also compared with tests/sample_ref.py, which states the lowest-index rule itself: five
    copies of it as the rows of one step, top_p placed next to p, draws[0 .. 4] = three placed draws, 0 and 1."""
    V, R = 1024, 5
    lg = seeded(R, V)
    lg[2, V // 2:] = lg[2, :V // 2]
    rig = Rig(ti, lg)
    tied = Rig(ti, np.tile(lg[2], (R, 1)))
    agree = 0
    for T, k, p in [(1.0, 2, 1.0), (1.0, 3, 1.0), (0.7, 40, 0.9), (2.0, 7, 0.99), (0.9, 9, 1.0), (1.0, 50, 0.9),
                    (0.5, 1000, 0.5)]:
        low = set(np.lexsort((np.arange(V), -lg[2]))[:k].tolist())
        ref = set(np.flatnonzero(oracle.sample_probs(lg[2], 1.0, k, 1.0) > 0).tolist())
        same = low == ref
        agree += same
        rig.check(oracle, T, k, p, 0, R - 1, 40, rows=None if same else {0, 1, 3, 4})
        top_p, draws, cut, want = E.realise_row(lg[2], T, k, p)
        assert E.decidable_cut(cut), (T, k, p, cut.top_p_margin, cut.rank_gap)
        tied.draws_h[:R] = draws
        tied.dd.upload(tied.draws_h)
        keys, lps = tied.run(T, k, float(top_p), 0, R - 1, 40)
        for j in range(R):
            assert int(keys[j, 0]) >> 32 == 0xFFFFFFFF and np.array_equal(keys[j, 1:], tied.keys0.reshape(R, SLOTS)[j, 1:])
            E.assert_draw(0xFFFFFFFF - (int(keys[j, 0]) & 0xFFFFFFFF), lps[j], want[j], j == R - 1, (T, k, p, j))
        assert np.array_equal(lps[R:].view(np.uint32), np.full(CAP - R, LP_FILL, f32).view(np.uint32))
    assert agree >= 3


def test_top_k_above_the_lds_capacity(ti, oracle):
    """top_k 8192 > TI_SAMPLE_MAX_K: the survivors of each row live in its part of the workspace."""
    V, R, k = 32000, 5, 8192
    wsb = ti.lib().ti_sample_workspace_bytes(V, k)
    assert wsb > 0
    rig = Rig(ti, seeded(R, V), ws_bytes=R * wsb)
    assert rig.check(oracle, 0.8, k, 0.9, 7, R - 1, 40) == R
    assert rig.check(oracle, 1.0, k, 1.0, 0, 2, 40) == 3
    rig.ws = None                                       # without a workspace: refused before any launch
    with pytest.raises(ti.TiError, match="ti error 1"):
        rig.run(1.0, k, 1.0, 0, 2, 40)
