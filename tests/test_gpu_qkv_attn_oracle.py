"""ti_qkv_attn_partials (qkv_attn.hip) against a float64 reference of the launch.

tests/qkv_attn_ref.py computes the operation (rms, q / k / v, RoPE, the new cache row, per-head
scores over keys [0, p], their logsumexp and the attention row) in float64 from the same fp16 inputs
and the dequantized weight, and merges the launch's part_o / part_ml on the host; nothing here knows
the kernel's split bounds, ring or tile ownership.  Inputs: `flat` (an almost uniform softmax),
`needle(j)` (row j of the cache holds >= 0.9 of every head's softmax: one dropped, masked or
misplaced key moves the output by ~|v|, not 1 / p) and `new_key_only` (the step's own key, read from
the exchange granules, holds >= 0.9); the share is asserted on the reference before every launch.

Checked after EVERY launch (Rig.check):
  * the new K / V row p against the reference, rtol = atol = 2e-3 (test_gpu_kernels.py's figure for
    the same epilogue); every other cache row bit-identical to what was uploaded;
  * the merged attention row, rtol = atol = 4e-3 (the project's figure for ti_attn_decode);
  * the merged logsumexp within LSE_TOL (below);
  * every split either empty (l == 0, m == -inf, a zero row) or live (l > 0, finite m, finite row);
  * the exchange's error word pair zero;
  * part_o, part_ml, the exchange and both caches sit at exactly their advertised sizes inside larger
    buffers: the 0xA5 pattern behind each is intact.
Shapes: the smallest per code path (qkv_attn_ref.BASE_SHAPES: every kernel instance, every k / v tile
ownership pattern, heads 12 / 24) and the two bench shapes, max_seq 320 (2048 for the bench positions).
The issue's shape table lists nine base shapes (its text says ten); all nine are here.

Measured on an MI355X over every case of this module (1744 launches; worst |got - reference|):
  row p of K 1.98e-3, of V 1.82e-3 (elements of magnitude > 4, where fp16 steps by 3.9e-3);
  the merged row 2.69e-3; the logsumexp 8.49e-4 (5.00e-4 over the flat cases alone: the fp32 GEMV rounding of q and k_p in
  the q . k_p term, supposed, not broken down further);
  the O output 1.66e-4 = 0.014 of its bound.
LSE_TOL = 4 x the worst logsumexp = 3.4e-3: below 0.5 / (p + 1) for every p <= 64 (7.7e-3 at p = 64), so
the logsumexp check alone sees one lost key of the flat softmax at those positions.
The tails of part_o (k_p, v_p copies: 2 heads head_dim fp16 behind [heads][S][hd]) and part_ml (q:
heads head_dim fp32 behind [heads][S][2]) that ti_hip.h's sizes reserve: the launch never writes them
(the 0xA5 fill is intact after every launch); asserted here so the header can be corrected against a test.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import qkv_attn_ref as R

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64
THETA = 10000.0
GUARD = 4096            # pattern bytes behind every buffer the launch writes
PAT = 0xA5
LSE_TOL = 3.4e-3        # 4 x the measured worst (module docstring)
KEEP_W_ELEMS = 8 << 20  # dequantized weights up to this size stay on the host (other fx than seed 0)

WORST = {"k_row": 0.0, "v_row": 0.0, "row": 0.0, "lse": 0.0, "lse_flat": 0.0, "o_out": 0.0, "o_out_over_bound": 0.0, "launches": 0}
_WEIGHTS: dict = {}
_RIGS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    _RIGS.clear()
    _WEIGHTS.clear()
    print("\nqkv_attn oracle, worst |got - reference| over %d launches: " % WORST["launches"]
          + ", ".join(f"{k} {v:.3e}" for k, v in WORST.items() if k != "launches"))


def dev(ti, a):
    return ti.DeviceBuffer.from_array(np.ascontiguousarray(a))


class Weights:
    """One shape's packed q | k | v weight on the device, and fx @ W in float64 per fx seed."""

    def __init__(self, ti, oracle, shape):
        bits, K, heads, kvh, hd, splits = shape
        w = R.make_weight(shape)
        t, sc = ti.wpack_host(w, bits)
        self.td, self.sd = dev(ti, t), dev(ti, sc)
        wf = R.dequantized(oracle, w, bits)
        del w, t, sc
        self.K = K
        self._lin = {0: R.project(R.make_fx(K, 0), wf)}
        self.wf = wf if wf.size <= KEEP_W_ELEMS else None

    def lin(self, seed):
        if seed not in self._lin:
            assert self.wf is not None, "only fx seed 0 at this shape"
            self._lin[seed] = R.project(R.make_fx(self.K, seed), self.wf)
        return self._lin[seed]


class Rig:
    """One (shape, max_seq): device buffers at their exact sizes with a pattern behind them, a host
    mirror of the caches, the launch and its checks."""

    def __init__(self, ti, oracle, shape, max_seq):
        self.ti, self.L, self.shape, self.max_seq = ti, ti.lib(), shape, max_seq
        bits, K, heads, kvh, hd, splits = shape
        assert heads * splits <= 256
        assert self.L.ti_qkv_attn_supported(bits, K, heads, kvh, hd, splits) == 1
        if shape not in _WEIGHTS:
            _WEIGHTS[shape] = Weights(ti, oracle, shape)
        self.w = _WEIGHTS[shape]
        self.cs = ti.rope_table(np.arange(max_seq), hd, THETA)
        self.csd = dev(ti, self.cs)
        self.fxd, self.ssd, self.posd = ti.DeviceBuffer(K * 2), ti.DeviceBuffer(256 * 4), ti.DeviceBuffer(4)
        self.po_main = heads * splits * hd
        self.po_bytes = self.L.ti_qkv_attn_part_o_elems(heads, hd, splits) * 2
        self.pml_main = heads * splits * 2
        self.pml_bytes = self.L.ti_qkv_attn_part_ml_elems(heads, hd, splits) * 4
        self.xg_bytes = self.L.ti_qkv_attn_xchg_bytes(heads, splits)
        self.err_off = self.L.ti_qkv_attn_error_offset(heads, splits)
        assert self.po_bytes >= self.po_main * 2 and self.pml_bytes >= self.pml_main * 4
        assert self.err_off + 8 <= self.xg_bytes
        self.cache_bytes = kvh * max_seq * hd * 2
        self.po, self.pml = ti.DeviceBuffer(self.po_bytes + GUARD), ti.DeviceBuffer(self.pml_bytes + GUARD)
        self.xg = ti.DeviceBuffer(self.xg_bytes + GUARD)
        self.kcd, self.vcd = ti.DeviceBuffer(self.cache_bytes + GUARD), ti.DeviceBuffer(self.cache_bytes + GUARD)
        for b in (self.xg, self.kcd, self.vcd):
            self.fill(b, 0, b.nbytes, PAT)
        self.zero_exchange()
        self.flat = R.flat_cache(kvh, max_seq, hd, R.shape_seed(shape))
        self.set_fx(0)
        self.set_ss(R.make_ss(K, 3, 0))
        self.load_cache(*self.flat)

    # ---- device plumbing
    def fill(self, buf, off, nbytes, byte):
        self.ti.check(self.L.ti_memset(buf.ptr + off, byte, nbytes, None))

    def fetch(self, buf, off, nbytes):
        out = np.empty(nbytes, np.uint8)
        self.ti.check(self.L.ti_memcpy_d2h(C.c_void_p(out.ctypes.data), buf.ptr + off, nbytes, None))
        return out

    def put(self, buf, off, a):
        a = np.ascontiguousarray(a)
        assert off + a.nbytes <= buf.nbytes
        self.ti.check(self.L.ti_memcpy_h2d(buf.ptr + off, C.c_void_p(a.ctypes.data), a.nbytes, None))

    def zero_exchange(self):
        self.fill(self.xg, 0, self.xg_bytes, 0)

    # ---- inputs
    def set_fx(self, seed):
        self.fx_seed = seed
        self.put(self.fxd, 0, R.make_fx(self.shape[1], seed))

    def set_ss(self, ss):
        """ss[0 .. n_ss) and 1e30 in the rest of the 256 floats: a read past n_ss shows in rms at once."""
        self.ss = np.asarray(ss, f32)
        full = np.full(256, 1e30, f32)
        full[:self.ss.size] = self.ss
        self.put(self.ssd, 0, full)

    def load_cache(self, kc, vc):
        """Whole-cache upload; the mirror is what the device must still hold outside row p."""
        self.kc, self.vc = kc.copy(), vc.copy()
        self.base_flat, self.planted = kc is self.flat[0], set()
        self.put(self.kcd, 0, self.kc)
        self.put(self.vcd, 0, self.vc)

    def set_row(self, j, krow, vrow):
        """Rows j of every kv-head, in place on the device (row-sized copies) and in the mirror."""
        bits, K, heads, kvh, hd, splits = self.shape
        self.kc[:, j], self.vc[:, j] = krow, vrow
        self.planted.add(j)
        for i in range(kvh):
            off = (i * self.max_seq + j) * hd * 2
            self.put(self.kcd, off, self.kc[i, j])
            self.put(self.vcd, off, self.vc[i, j])

    def restore_row(self, j):
        self.set_row(j, self.flat[0][:, j], self.flat[1][:, j])
        self.planted.discard(j)

    def proj(self, p):
        bits, K, heads, kvh, hd, splits = self.shape
        return R.Proj(self.w.lin(self.fx_seed), self.ss, R.EPS, self.cs, p, K, heads, kvh, hd)

    # ---- the launch
    def launch(self, p):
        bits, K, heads, kvh, hd, splits = self.shape
        assert 0 <= p < self.max_seq
        self.put(self.posd, 0, np.array([p], np.int32))
        self.fill(self.po, 0, self.po.nbytes, PAT)
        self.fill(self.pml, 0, self.pml.nbytes, PAT)
        self.ti.check(self.L.ti_qkv_attn_partials(self.w.td.ptr, self.w.sd.ptr, bits, self.fxd.ptr, self.ssd.ptr,
                                                  self.ss.size, R.EPS, self.csd.ptr, self.posd.ptr, self.kcd.ptr,
                                                  self.vcd.ptr, self.max_seq, K, heads, kvh, hd, splits, self.po.ptr,
                                                  self.pml.ptr, self.xg.ptr, None))
        self.ti.sync()
        WORST["launches"] += 1

    def check(self, p, pr=None, at=None, adopt=False):
        """Every check of the module docstring against the reference of the rig's current inputs;
        -> (pr, at, merged row, device V row p)."""
        bits, K, heads, kvh, hd, splits = self.shape
        if pr is None:
            pr = self.proj(p)
        if at is None:
            at = R.Attn(pr, self.kc, self.vc)
        pat16, pat32 = np.uint16(PAT * 0x0101), np.uint32(PAT * 0x01010101)
        # buffers: sizes and what lies behind them
        po_raw = self.fetch(self.po, 0, self.po.nbytes)
        pml_raw = self.fetch(self.pml, 0, self.pml.nbytes)
        assert np.all(po_raw[self.po_bytes:] == PAT), "written behind part_o"
        assert np.all(pml_raw[self.pml_bytes:] == PAT), "written behind part_ml"
        assert np.all(self.fetch(self.xg, self.xg_bytes, GUARD) == PAT), "written behind the exchange"
        part_o = po_raw[:self.po_main * 2].view(f16).reshape(heads, splits, hd)
        part_ml = pml_raw[:self.pml_main * 4].view(f32).reshape(heads, splits, 2)
        # (the reserved tails: the launch leaves them alone)
        assert np.all(po_raw[self.po_main * 2:self.po_bytes].view(np.uint16) == pat16), "part_o tail written"
        assert np.all(pml_raw[self.pml_main * 4:self.pml_bytes].view(np.uint32) == pat32), "part_ml tail written"
        err = self.fetch(self.xg, self.err_off, 8).view(np.uint32)
        assert not err.any(), f"exchange error words {err.tolist()}"
        # caches: row p against the reference, every other row untouched, nothing behind them
        rows = {}
        for name, buf, mirror, ref in (("k_row", self.kcd, self.kc, pr.k), ("v_row", self.vcd, self.vc, pr.v)):
            raw = self.fetch(buf, 0, buf.nbytes)
            assert np.all(raw[self.cache_bytes:] == PAT), f"written behind the {name[0]} cache"
            got = raw[:self.cache_bytes].view(np.uint16).reshape(kvh, self.max_seq, hd)
            exp = mirror.view(np.uint16)
            same = got == exp
            same[:, p] = True
            assert np.all(same), f"{name[0]} cache rows other than {p} changed: {np.argwhere(~same)[:4].tolist()}"
            new = got[:, p].view(f16).astype(f64)
            WORST[name] = max(WORST[name], float(np.abs(new - ref).max()))
            np.testing.assert_allclose(new, ref, rtol=2e-3, atol=2e-3, err_msg=f"{name} p={p}")
            rows[name] = new
            if adopt:
                mirror[:, p] = got[:, p].view(f16)
        # partials and their merge
        R.check_partials(part_o, part_ml)
        row, lse = R.merge_partials(part_o, part_ml)
        WORST["row"] = max(WORST["row"], float(np.abs(row - at.row).max()))
        d_lse = float(np.abs(lse - at.lse).max())
        WORST["lse"] = max(WORST["lse"], d_lse)
        if self.base_flat and not self.planted:
            WORST["lse_flat"] = max(WORST["lse_flat"], d_lse)
        np.testing.assert_allclose(row, at.row, rtol=4e-3, atol=4e-3, err_msg=f"attention row p={p}")
        assert d_lse <= LSE_TOL, f"logsumexp p={p}: |d| {d_lse} (head {int(np.abs(lse - at.lse).argmax())})"
        return pr, at, row, rows["v_row"]


def rig(ti, oracle, shape, max_seq=320):
    key = (shape, max_seq)
    if key not in _RIGS:
        _RIGS[key] = Rig(ti, oracle, shape, max_seq)
    r = _RIGS[key]
    r.set_fx(0)
    r.set_ss(R.make_ss(shape[1], 3, 0))
    r.load_cache(*r.flat)
    return r


SWEEP = sorted(set(list(range(10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193,
                                      255, 256, 257, 300]))


@pytest.mark.parametrize("shape", R.BASE_SHAPES, ids=R.shape_id)
def test_position_sweep_flat(ti, oracle, shape):
    """Positions around every split / slot / ring boundary and last_extra, and max_seq - 1, on one
    upload of the flat cache (row p put back after each launch).  At p <= 64 the logsumexp bound is
    below 0.5 / (p + 1): a lost key of the flat softmax (about 1 / (p + 1) of it) shows there too."""
    r = rig(ti, oracle, shape)
    for p in sorted(set(min(q, r.max_seq - 1) for q in SWEEP + [r.max_seq - 1])):
        if p <= 64:
            assert LSE_TOL < 0.5 / (p + 1)
        r.launch(p)
        r.check(p)
        r.restore_row(p)


def needle_walk(r, p, js):
    pr = r.proj(p)
    flat = R.Attn(pr, r.kc, r.vc)
    prev = None
    for j in js:
        if prev is not None:
            r.restore_row(prev)
        r.set_row(j, *R.needle_rows(pr, flat, j, 0))
        at = R.Attn(pr, r.kc, r.vc)
        R.assert_share(at, j)
        r.launch(p)
        r.check(p, pr, at)
        prev = j


@pytest.mark.parametrize("shape", R.ALL_SHAPES, ids=R.shape_id)
def test_needle_walk_p100(ti, oracle, shape):
    """The needle at every j of [0, 100): every split bound, ring slot and lane group holds it once."""
    needle_walk(rig(ti, oracle, shape), 100, range(100))


@pytest.mark.parametrize("shape", R.ALL_SHAPES, ids=R.shape_id)
def test_needle_p319(ti, oracle, shape):
    needle_walk(rig(ti, oracle, shape), 319,
                [0, 1, 7, 8, 39, 40, 79, 80, 158, 159, 160, 254, 255, 256, 309, 310, 317, 318])


@pytest.mark.parametrize("shape", R.ALL_SHAPES, ids=R.shape_id)
def test_new_key_only(ti, oracle, shape):
    """The step's own key, computed in the launch and read from the k / v tile owners' granules."""
    r = rig(ti, oracle, shape)
    r.launch(0)
    pr, at, row, v_dev = r.check(0)
    # p = 0: one key with weight 1, so the merged row is the cache's new V row, up to the fp16
    # rounding of the split's normalised row
    g = shape[2] // shape[3]
    v_h = np.repeat(v_dev, g, axis=0)
    assert np.all(np.abs(row - v_h) <= 2.0 ** -11 * np.abs(v_h) + 2.0 ** -25)
    for p in (1, 31, 32, 33, 255, 256, 257, 319):
        pr = r.proj(p)
        kc = r.flat[0].copy()
        kc[:, :p] = R.new_key_only_row(pr)[:, None]
        r.load_cache(kc, r.flat[1])
        at = R.Attn(pr, r.kc, r.vc)
        R.assert_share(at, p)
        r.launch(p)
        r.check(p, pr, at)


@pytest.mark.parametrize("shape", R.BENCH_SHAPES, ids=R.shape_id)
def test_bench_positions(ti, oracle, shape):
    """The bench position (p = 2047 of max_seq 2048: nothing behind the caches' last row is touched)."""
    r = rig(ti, oracle, shape, max_seq=2048)
    p = 2047
    r.launch(p)
    r.check(p)
    needle_walk(r, p, [0, 255, 256, 1791, 1792, 2046])


@pytest.mark.parametrize("shape", [R.BASE_SHAPES[0], R.BASE_SHAPES[7]], ids=R.shape_id)
def test_n_ss(ti, oracle, shape):
    """1..256 partial sums of squares (ss[lane + 64 j], j < 4), 1e30 behind them."""
    r = rig(ti, oracle, shape)
    p = 40
    for n_ss in (1, 2, 63, 64, 65, 128, 200, 256):
        r.set_ss(R.make_ss(shape[1], n_ss, n_ss, total=0.8 * shape[1]))
        assert abs(float(r.ss.astype(f64).sum()) / (0.8 * shape[1]) - 1) < 1e-5
        r.launch(p)
        r.check(p)


@pytest.mark.parametrize("shape", R.BASE_SHAPES[:3], ids=R.shape_id)
def test_exchange_reuse(ti, oracle, shape):
    """Six launches on one exchange zeroed once, a different fx and p each (p may go down): a granule
    left by the previous launch would give a wrong q or a wrong new key.  One shape per k / v tile
    count of a workgroup (zero or one, one, two).  The rows the launches write stay in the cache."""
    r = rig(ti, oracle, shape)
    r.zero_exchange()
    for n, p in enumerate((0, 5, 4, 200, 1, 319)):
        r.set_fx(100 + n)
        r.launch(p)
        r.check(p, adopt=True)
    gens = r.fetch(r.xg, 0, r.err_off).view(np.uint32).reshape(-1, 32, 2)[:, :16, 1]
    assert np.all(gens == 6), "every workgroup's q granules carry the sixth generation"


@pytest.mark.parametrize("shape", R.BENCH_SHAPES, ids=R.shape_id)
def test_through_o_projection(ti, oracle, shape):
    """The consumer (TI_X_ATTN_SPLITS) on the fused partials against float64: the reference attention
    row times the dequantized W_o, within test_gpu_fold.py's split-merge bound."""
    bits, K, heads, kvh, hd, splits = shape
    r = rig(ti, oracle, shape)
    p, H, qd = 300, 1024, heads * hd
    r.launch(p)
    pr, at, row, _ = r.check(p)
    wo = (np.random.RandomState(77).standard_normal((qd, H)) * 0.03).astype(f32)
    to, so = ti.wpack_host(wo, 4)
    tod, sod, yd = dev(ti, to), dev(ti, so), ti.DeviceBuffer(H * 4)
    ep = ti.Epilogue()
    ep.kind, ep.ldo, ep.out, ep.ss_in, ep.n_ss, ep.head_dim = ti.EPI_STORE_F32, H, yd.ptr, r.pml.ptr, splits, hd
    ti.check(ti.lib().ti_gemm_wq_a16(tod.ptr, sod.ptr, 4, r.po.ptr, ti.X_ATTN_SPLITS, qd, None, 1e-5, 1, H, qd,
                                     C.byref(ep), None))
    ti.sync()
    got = yd.download(f32, H).astype(f64)
    wf = R.dequantized(oracle, wo, 4).astype(f64)
    x = at.row.reshape(-1)
    bound = 2.5e-3 * (np.abs(x) @ np.abs(wf)) + 1e-6
    err = np.abs(got - x @ wf)
    WORST["o_out"] = max(WORST["o_out"], float(err.max()))
    WORST["o_out_over_bound"] = max(WORST["o_out_over_bound"], float((err / bound).max()))
    assert np.all(np.isfinite(got))
    assert np.all(err <= bound), f"max err {err.max()} (bound {bound.min()})"
