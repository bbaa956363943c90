"""ti_kv_copy_slots (kv_copy_kernel, kernels/misc.hip) against kv_copy_ref of tests/step_ref.py.

The caches are uint16 arrays of an index hash (no two elements of an aligned block of 65536 equal, buffers told
apart), each inside a larger allocation with guard elements on both sides; after the call the WHOLE of every
allocation must equal the model's, so a chunk copied to the wrong place, dropped, or written past a row shows.
Before every call the test checks on the host that the rows lie inside the caches."""
from __future__ import annotations

import numpy as np
import pytest

from step_ref import assert_buffers_equal, index_hash, kv_copy_ref

pytestmark = pytest.mark.gpu

GUARD = 32      # uint16 elements on each side of every cache (64 bytes: rows stay 16-byte aligned)


class Caches:
    """n_tab caches of n uint16 elements on the device and their pointer table."""

    def __init__(self, ti, n_tab: int, n: int):
        self.ti, self.n = ti, n
        self.host = [index_hash(n + 2 * GUARD, salt=t + 1) for t in range(n_tab)]
        self.dev = [ti.DeviceBuffer.from_array(h) for h in self.host]
        self.tab = ti.DeviceBuffer.from_array(np.array([d.ptr + 2 * GUARD for d in self.dev], np.uint64))

    def copy(self, src_off, dst_off, rows, row_pitch, row_elems, n_tab=None) -> int:
        last = (rows - 1) * row_pitch + row_elems
        assert src_off >= -GUARD and dst_off >= 0 and max(src_off, dst_off) + max(last, 0) <= self.n, "outside the cache"
        rc = self.ti.lib().ti_kv_copy_slots(self.tab.ptr, len(self.dev) if n_tab is None else n_tab, src_off, dst_off,
                                            rows, row_pitch, row_elems, None)
        self.ti.sync()
        return rc

    def download(self):
        return [d.download(np.uint16, self.n + 2 * GUARD) for d in self.dev]

    def expect(self, src_off, dst_off, rows, row_pitch, row_elems):
        """The model on the host copies (offsets counted from the cache base, behind the guard)."""
        self.host = kv_copy_ref(self.host, GUARD + src_off, GUARD + dst_off, rows, row_pitch, row_elems)

    def check(self):
        assert_buffers_equal(self.download(), self.host)


def fork_args(src, dst, n, kv_heads, max_seq, head_dim, d=1):
    """ti_eng::fork_slot's arguments (host/engine_beam.cpp); d = 2 for an e4m3 cache."""
    kv_stride = kv_heads * max_seq * head_dim
    return src * kv_stride // d, dst * kv_stride // d, kv_heads, max_seq * head_dim // d, n * head_dim // d


@pytest.mark.parametrize("kv8", [False, True], ids=["fp16", "e4m3"])
@pytest.mark.parametrize("n", [1, 17, 40])
@pytest.mark.parametrize("head_dim", [64, 128])
def test_engine_form(ti, head_dim, n, kv8):
    """fork_slot for 2 layers (a table of 4 pointers), kv_heads 2, max_seq 40, 4 slots: slot 1 -> 3, then 3 -> 0.
    An e4m3 cache holds one byte per element and goes as the same bytes in 2-byte units at half the counts;
    head_dim 64 with n = 1 is its smallest count, 32 units."""
    kv_heads, max_seq, slots, d = 2, 40, 4, 2 if kv8 else 1
    c = Caches(ti, 4, slots * kv_heads * max_seq * head_dim // d)
    for src, dst in ((1, 3), (3, 0)):
        args = fork_args(src, dst, n, kv_heads, max_seq, head_dim, d)
        assert all(a % 8 == 0 for a in args[:2] + args[3:])
        assert c.copy(*args) == 0, ti.lib().ti_last_error()
        c.expect(*args)
        c.check()
    if kv8 and head_dim == 64 and n == 1:
        assert args[4] == 32
    # slot 0 now holds slot 1's prefix, and slot 2 was never touched
    cache = c.host[2][GUARD:GUARD + c.n].reshape(slots, kv_heads, max_seq * head_dim // d)
    orig = index_hash(c.n + 2 * GUARD, salt=3)[GUARD:GUARD + c.n].reshape(cache.shape)
    w = n * head_dim // d
    assert np.array_equal(cache[0, :, :w], orig[1, :, :w]) and np.array_equal(cache[0, :, w:], orig[0, :, w:])
    assert np.array_equal(cache[2], orig[2]) and np.array_equal(cache[1], orig[1])


@pytest.mark.parametrize("chunks", [1, 255, 256, 257, 16385])
def test_chunks_per_row(ti, chunks):
    """16-byte chunks per row around the 256-thread block, and 16385: one more than the 64 x 256 threads of the
    capped grid, so the grid-stride loop runs a second trip for exactly one chunk.  The pitch is one chunk wider
    than the row: a copy that ignores it, or runs past the row, lands in the gap column."""
    rows, row_elems = 2, 8 * chunks
    pitch = row_elems + 8
    src_off, dst_off = 8, 8 + rows * pitch + 16
    c = Caches(ti, 2, dst_off + rows * pitch + 8)
    args = (src_off, dst_off, rows, pitch, row_elems)
    assert c.copy(*args) == 0, ti.lib().ti_last_error()
    c.expect(*args)
    c.check()
    got = c.host[1][GUARD:]
    assert np.array_equal(got[dst_off + pitch: dst_off + pitch + row_elems], got[src_off + pitch: src_off + pitch + row_elems])
    assert c.copy(dst_off, src_off + 8, rows, pitch, row_elems - 8) == 0       # back, shifted by one chunk
    c.expect(dst_off, src_off + 8, rows, pitch, row_elems - 8)
    c.check()


def test_noops_and_refusals(ti):
    rows, row_elems, pitch = 2, 64, 72
    src_off, dst_off = 8, 8 + rows * pitch + 16
    c = Caches(ti, 2, dst_off + rows * pitch + 8)
    ok = (src_off, dst_off, rows, pitch, row_elems)
    assert c.copy(src_off, dst_off, rows, pitch, 0) == 0            # nothing to copy
    c.check()
    assert c.copy(src_off, src_off, rows, pitch, row_elems) == 0    # onto itself
    c.check()
    refused = {
        "src_off % 8": (src_off + 4, dst_off, rows, pitch, row_elems),
        "dst_off % 8": (src_off, dst_off + 4, rows, pitch, row_elems),
        "row_pitch % 8": (src_off, dst_off, rows, pitch + 4, row_elems),
        "row_elems % 8": (src_off, dst_off, rows, pitch, row_elems - 4),
        "row_pitch < row_elems": (src_off, dst_off, rows, row_elems - 8, row_elems),
        "src_off < 0": (-8, dst_off, rows, pitch, row_elems),
        "rows = 0": (src_off, dst_off, 0, pitch, row_elems),
    }
    for name, args in refused.items():
        assert c.copy(*args) != 0, name
        assert b"ti_kv_copy_slots" in ti.lib().ti_last_error(), name
        c.check()
    assert c.copy(*ok, n_tab=0) != 0
    c.check()
    assert ti.lib().ti_kv_copy_slots(None, 2, *ok, None) != 0       # no table
    c.check()
    assert c.copy(*ok) == 0                                          # the same arguments do copy
    c.expect(*ok)
    c.check()
