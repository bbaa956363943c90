"""The bound test_gpu_gemv_mbr.py holds gemv_mbr_kernel's fp32 outputs to (assert_close_dot,
rel 2e-5) sees the faults the kernel could have: on the expected matrix of that file's NTL = 6 case
(no GPU: host packer, oracle and plan query only), two adjacent output columns swapped in a
workgroup's last tile, and one k-group's contribution dropped from one tile, are both rejected,
while the fp32 rounding of the exact result passes."""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_gemv_mbr import expect_plan, n_of, store_case, tile_ranges
from test_gpu_kernels import assert_close_dot

f32 = np.float32


@pytest.fixture(scope="module")
def case(ti_host, oracle):
    M, N, K = 13, n_of(6), 384
    expect_plan(ti_host, M, N, K, 256, 6, {5: 219, 6: 37})
    x, _, _, wf, ref = store_case(ti_host, oracle, M, N, K)
    t0, t1 = next(r for r in tile_ranges(N, 256) if r[1] - r[0] == 6)
    return x.astype(f32), wf, ref, 16 * (t1 - 1)      # ..., first column of a 6-tile workgroup's last tile


def test_bound_passes_the_rounded_result(case):
    xa, wf, ref, _ = case
    assert_close_dot(ref.astype(f32), ref, xa, wf)


def test_bound_rejects_swapped_columns(case):
    xa, wf, ref, c0 = case
    bad = ref.astype(f32)
    bad[:, [c0 + 4, c0 + 5]] = bad[:, [c0 + 5, c0 + 4]]
    with pytest.raises(AssertionError):
        assert_close_dot(bad, ref, xa, wf)


def test_bound_rejects_a_dropped_k_group(case):
    xa, wf, ref, c0 = case
    cols = slice(c0, c0 + 16)
    bad = ref.copy()
    bad[:, cols] -= xa[:, 128:256].astype(np.float64) @ wf[128:256, cols].astype(np.float64)
    with pytest.raises(AssertionError):
        assert_close_dot(bad.astype(f32), ref, xa, wf)
