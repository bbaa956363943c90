"""ti_logprob_rows alone (kernels/logprob.hip) against a float64 numpy log-softmax of the same fp32
logits.

Bars.  out_top1 exact (lowest index on ties).  |lp - lp64| <= 1e-4 absolute, for |logit| <= 80 and
vocab <= 128256: a lane sums at most about 500 terms serially before the tree merge, so the
worst-case relative error of the sum is about 500 * 2^-24 ~ 3e-5 (an absolute error of log(sum));
the subtraction and the hardware exp add about 1e-5; the bar is three times that.

Rows are N(0, 5^2) with uniform targets, except the planted ones (PLANTS).  A case has a fixed row
count, so the planted rows fill the rows of as many launches as they need (one more row than plants
is always random); the first plant lands on row 0 of the first launch, whose base is 16-byte
aligned: at vocab 1003 its last 3 elements are the scalar tail.  At ld 1005 row 1 starts 4 bytes
past a boundary, so its first 3 elements are the scalar head (the second plant)."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 1e-4
CASES = [(1, 16, 16), (5, 1003, 1005), (64, 32000, 32000), (2, 128256, 128256)]


def _max_last(x, V):      # the maximum is the last element (of the tail, where the row has one)
    x[V - 1] = 60.0
    return V - 1


def _max_first(x, V):     # ... the first element (of the head, where the row has one)
    x[0] = 60.0
    return 0


def _spike(x, V):         # +80 over a floor of -80: overflows without the max subtraction; lp ~ 0
    x[:] = -80.0
    x[V // 2] = 80.0
    return V // 2


def _spike_floor(x, V):   # the same row scored at a floor element: lp ~ -160
    _spike(x, V)
    return V // 2 + 1


def _all_equal(x, V):     # lp = -log(vocab), top1 = 0
    x[:] = 1.5
    return V - 2


def _dup_max(x, V):       # the maximum at two indices: top1 is the lower
    x[V // 3] = x[2 * V // 3 + 1] = 50.0
    return 2 * V // 3 + 1


def _no_target(x, V):     # exactly 0.0f
    return -1


def _bad_target_hi(x, V):  # exactly -20.0f
    return V


def _bad_target_lo(x, V):
    return -2


PLANTS = [_max_last, _max_first, _spike, _spike_floor, _all_equal, _dup_max, _no_target, _bad_target_hi,
          _bad_target_lo]


def _expected(x, tg, V):
    x64 = x[:, :V].astype(np.float64)
    mx = x64.max(axis=1)
    lse = mx + np.log(np.exp(x64 - mx[:, None]).sum(axis=1))
    lp = np.zeros(len(tg), np.float64)
    for r, t in enumerate(tg):
        lp[r] = 0.0 if t == -1 else (-20.0 if not 0 <= t < V else x64[r, t] - lse[r])
    return lp, np.argmax(x64, axis=1)   # (first occurrence = lowest index)


@pytest.mark.parametrize("rows,V,ld", CASES, ids=[f"{r}x{v}_ld{l}" for r, v, l in CASES])
def test_logprob_rows_vs_float64(ti, rows, V, ld):
    rng = np.random.RandomState(1000 + rows)
    n_launch = (len(PLANTS) + 1 + rows - 1) // rows
    worst, planted = 0.0, 0
    for k in range(n_launch):
        x = np.full((rows, ld), 1e30, np.float32)            # (padding past vocab must not be read as logits)
        x[:, :V] = (rng.standard_normal((rows, V)) * 5.0).astype(np.float32)
        tg = rng.randint(0, V, size=rows).astype(np.int32)
        exact = {}
        for r in range(rows):
            p = k * rows + r
            if p < len(PLANTS):
                tg[r] = PLANTS[p](x[r, :V], V)
                planted += 1
                if PLANTS[p] in (_no_target, _bad_target_hi, _bad_target_lo):
                    exact[r] = 0.0 if PLANTS[p] is _no_target else -20.0
        xd, td = ti.DeviceBuffer.from_array(x), ti.DeviceBuffer.from_array(tg)
        od, id_ = ti.DeviceBuffer(rows * 4), ti.DeviceBuffer(rows * 4)
        ti.logprob_rows(xd, ld, rows, V, td, od, id_)
        ti.sync()
        lp, top1 = od.download(np.float32, (rows,)), id_.download(np.int32, (rows,))
        ref_lp, ref_top1 = _expected(x, tg, V)
        err = np.abs(lp.astype(np.float64) - ref_lp)
        worst = max(worst, float(err.max()))
        print(f"launch {k}: max |lp - lp64| {err.max():.3e} (row {int(err.argmax())}), lp range "
              f"[{lp.min():.4g}, {lp.max():.4g}]")
        assert np.array_equal(top1, ref_top1), f"launch {k}: top1 {top1.tolist()} != {ref_top1.tolist()}"
        assert float(err.max()) <= BAR, f"launch {k}: |lp - lp64| {err.max():.3e} > {BAR} at row {int(err.argmax())}"
        for r, v in exact.items():
            assert lp[r] == np.float32(v), f"launch {k} row {r}: {lp[r]} is not exactly {v}"
        # a null out_top1 is allowed and leaves the log-probabilities unchanged
        o2 = ti.DeviceBuffer(rows * 4)
        ti.logprob_rows(xd, ld, rows, V, td, o2)
        ti.sync()
        assert np.array_equal(o2.download(np.float32, (rows,)), lp)
        for b in (xd, td, od, id_, o2):
            b.free()
    assert planted == len(PLANTS)
    print(f"worst |lp - lp64| over {n_launch} launches: {worst:.3e} (bar {BAR})")


def test_logprob_rows_planted_values(ti):
    """The planted rows' values themselves, at the odd shape (what the float64 reference must also say)."""
    V, ld = 1003, 1005
    x = np.zeros((3, ld), np.float32)
    tg = np.array([_spike(x[0, :V], V), _spike_floor(x[1, :V], V), _all_equal(x[2, :V], V)], np.int32)
    xd, td, od = ti.DeviceBuffer.from_array(x), ti.DeviceBuffer.from_array(tg), ti.DeviceBuffer(12)
    ti.logprob_rows(xd, ld, 3, V, td, od)
    ti.sync()
    lp = od.download(np.float32, (3,)).astype(np.float64)
    assert abs(lp[0]) <= BAR and abs(lp[1] + 160.0) <= BAR and abs(lp[2] + np.log(V)) <= BAR, lp.tolist()
