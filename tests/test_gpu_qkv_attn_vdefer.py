"""The two orders of the head_dim-128 fused QKV + attention launch write the same bytes.

The default order defers the v tile's items into the attention loop, gathers q off the K/V ring's wait chain and
publishes the v row behind a barrier inside the attention; TI_QA_VDEFER=0 keeps the old order (k and v tiles,
gather, attention).  Nothing is computed differently, so this process (ti_qkv_attn_v_deferred == 1) and a fresh
child process under the knob (== 0; the knob is read once per process) must agree byte for byte on
  * part_o and part_ml, whole buffers: the [heads][S][hd] / [heads][S][2] partials, the k_p / v_p / q areas behind
    them and a guard behind the advertised sizes (a fill pattern the launch must leave alone),
  * the exchange buffer: every granule (values and generations), the error words (asserted zero) and a guard,
  * row p of both caches after every launch, and both whole caches after each position's last launch.

Shapes: the two smallest head_dim-128 shapes of qkv_attn_ref.py, max_seq 2048, inputs from that module.
Positions (a ring slot is 4 keys, a split's slots go round its 8 waves, split S - 1 is 32 keys short), by a wave's
slot count: p = 0 none anywhere; 1 and 5: one slot in wave 0 (and 1) of split 0 only; 100: 1 or 0; 250: 2 in wave 0,
1 in the others; 520: 3 and 2 -- the waves of a workgroup on both sides of the first ring round, some with fewer
slots than the four deferred v items; 1000 and 1023: 5 and 4 (one round and a tail); 2047 = max_seq - 1: 9 and 8,
7 in split S - 1 (two or three rounds, tails of 0, 1 and 2).
Each position runs six consecutive launches (a fresh fx per launch) on one exchange buffer that is zeroed once
per shape, so every launch's generation tags follow the previous launch's.

Nothing is compared with a reference here: the arithmetic is pinned by test_gpu_qkv_attn_oracle.py.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import qkv_attn_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4096, 8, 8, 128, 8), (8, 4096, 24, 24, 128, 8)]
assert all(s in R.BASE_SHAPES for s in SHAPES)
MAX_SEQ = 2048
POSITIONS = [0, 1, 5, 100, 250, 520, 1000, 1023, MAX_SEQ - 1]
LAUNCHES = 6
FILL, GUARD = 0xA5, 256


def run_shape(ti, shape):
    """Every position's six launches -> {name: bytes (uint8)}."""
    L = ti.lib()
    bits, K, heads, kvh, hd, S = shape
    sid = R.shape_id(shape)
    assert L.ti_qkv_attn_supported(bits, K, heads, kvh, hd, S) == 1
    seed = R.shape_seed(shape)
    t, sc = ti.wpack_host(R.make_weight(shape), bits)
    dev = lambda a: ti.DeviceBuffer.from_array(np.ascontiguousarray(a))   # noqa: E731
    td, sd = dev(t), dev(sc)
    fxs = [dev(R.make_fx(K, i)) for i in range(LAUNCHES)]
    sss = [dev(R.make_ss(K, 3, i)) for i in range(LAUNCHES)]
    csd = dev(ti.rope_table(np.arange(MAX_SEQ), hd, 10000.0))
    kc, vc = R.flat_cache(kvh, MAX_SEQ, hd, seed)
    kcd, vcd = dev(kc), dev(vc)
    po_n = L.ti_qkv_attn_part_o_elems(heads, hd, S) * 2 + GUARD
    pml_n = L.ti_qkv_attn_part_ml_elems(heads, hd, S) * 4 + GUARD
    xg_n = L.ti_qkv_attn_xchg_bytes(heads, S)
    err_off = L.ti_qkv_attn_error_offset(heads, S)
    po, pml = dev(np.full(po_n, FILL, np.uint8)), dev(np.full(pml_n, FILL, np.uint8))
    xg_host = np.full(xg_n + GUARD, FILL, np.uint8)
    xg_host[:xg_n] = 0
    xg = dev(xg_host)
    res = {f"{sid}/deferred": np.array([L.ti_qkv_attn_v_deferred(bits, hd)], np.int64),
           f"{sid}/err_off": np.array([err_off], np.int64)}
    row = np.empty((kvh, hd), np.uint16)
    for p in POSITIONS:
        pd = dev(np.array([p], np.int32))
        for i in range(LAUNCHES):
            ti.check(L.ti_qkv_attn_partials(td.ptr, sd.ptr, bits, fxs[i].ptr, sss[i].ptr, 3, R.EPS, csd.ptr, pd.ptr,
                                            kcd.ptr, vcd.ptr, MAX_SEQ, K, heads, kvh, hd, S, po.ptr, pml.ptr, xg.ptr,
                                            None))
            ti.sync()
            key = f"{sid}/p{p}/l{i}/"
            res[key + "part_o"] = po.download(np.uint8, po_n)
            res[key + "part_ml"] = pml.download(np.uint8, pml_n)
            res[key + "xchg"] = xg.download(np.uint8, xg_n + GUARD)
            for name, buf in (("k_row", kcd), ("v_row", vcd)):
                for j in range(kvh):
                    ti.check(L.ti_memcpy_d2h(C.c_void_p(row[j].ctypes.data), buf.ptr + (j * MAX_SEQ + p) * hd * 2,
                                             hd * 2, None))
                res[key + name] = row.view(np.uint8).copy()
        res[f"{sid}/p{p}/k_cache"] = kcd.download(np.uint8, kc.nbytes)
        res[f"{sid}/p{p}/v_cache"] = vcd.download(np.uint8, vc.nbytes)
        pd.free()
    for b in [td, sd, csd, kcd, vcd, po, pml, xg] + fxs + sss:
        b.free()
    return res


def run_all(ti):
    res = {}
    for shape in SHAPES:
        res.update(run_shape(ti, shape))
    return res


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import turboinfer_amd as T
from test_gpu_qkv_attn_vdefer import run_all
T.init(0)
np.savez(sys.argv[2], **run_all(T))
"""


@pytest.fixture(scope="module")
def both(ti, tmp_path_factory):
    assert not os.environ.get("TI_QA_VDEFER"), "this process must run the deferred order"
    new = run_all(ti)
    out = str(tmp_path_factory.mktemp("vdefer") / "old_order.npz")
    env = dict(os.environ, TI_QA_VDEFER="0")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return new, dict(np.load(out))


@pytest.mark.parametrize("shape", SHAPES, ids=R.shape_id)
def test_orders_are_the_ones_asked_for(both, shape):
    new, old = both
    sid = R.shape_id(shape)
    assert int(new[sid + "/deferred"][0]) == 1, "this process did not take the deferred order"
    assert int(old[sid + "/deferred"][0]) == 0, "TI_QA_VDEFER=0 did not select the old order"
    assert sorted(new) == sorted(old)


@pytest.mark.parametrize("p", POSITIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=R.shape_id)
def test_deferred_order_matches_old_order_bytes(both, shape, p):
    new, old = both
    bits, K, heads, kvh, hd, S = shape
    sid = R.shape_id(shape)
    err_off = int(new[sid + "/err_off"][0])
    pre = f"{sid}/p{p}/"
    keys = sorted(k for k in new if k.startswith(pre))
    assert len(keys) == 5 * LAUNCHES + 2
    for i in range(LAUNCHES):
        for side, r in (("deferred", new), ("old", old)):
            x = r[f"{pre}l{i}/xchg"]
            assert not x[err_off:err_off + 8].any(), f"launch {i}, {side} order: a granule wait expired"
            gens = x[:err_off].view(np.uint32)[1::2]
            assert np.all(gens == gens[0]) and gens[0] > 0, f"launch {i}, {side} order: generations {np.unique(gens)}"
    for k in keys:
        a, b = new[k], old[k]
        assert a.shape == b.shape and a.size > 0
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{k}: {bad.size} bytes differ, first at {bad[:8]}"
    # the launches wrote their partials, left the guards alone, and consecutive launches (a fresh fx) differ
    for i in range(LAUNCHES):
        po, pml, x = new[f"{pre}l{i}/part_o"], new[f"{pre}l{i}/part_ml"], new[f"{pre}l{i}/xchg"]
        assert np.all(po[-GUARD:] == FILL) and np.all(pml[-GUARD:] == FILL) and np.all(x[-GUARD:] == FILL)
        assert np.any(pml[:heads * S * 8] != FILL)
        if i:
            assert np.any(new[f"{pre}l{i}/k_row"] != new[f"{pre}l{i - 1}/k_row"])
            assert np.any(new[f"{pre}l{i}/v_row"] != new[f"{pre}l{i - 1}/v_row"])
