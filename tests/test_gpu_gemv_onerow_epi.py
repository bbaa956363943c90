"""One-row instances of gemv_wq_kernel (epilogue kind fixed at compile time) against the generic
instance of the same launch.

Each case runs one ti_gemm_wq_a16 launch on inputs built from the case's name: here as built (the one-row
instance), and in a fresh child process with TI_GEMV_EPI_GENERIC=1 (the knob is read once per process, so the
child sets it before its first GPU call).  Every output buffer must be byte-identical, bytes the launch does
not write included (the buffers start from a fill pattern): out / fold_x / fold_ss of the residual kind, act of
the SiLU kind, the logits, the 32 argmax slots and the step counter of the argmax kind, q and the whole K and V
caches of the RoPE kind.  ti_gemm_onerow_epi_launches must count the launch here and must not count it in the
child, so a silent fall-back to the generic instance cannot pass.

Weights are random packed bytes and fp16 group scales (any nibble / byte is a valid weight); nothing is compared
with a reference here -- the arithmetic of both instances is pinned elsewhere (test_gpu_kernels.py, test_gpu_fold.py).

Shapes (256 workgroups on an MI355X): K 512 (waves without k-tiles), 1024 (one k-tile per wave), 4096, 11008
(86 k-tiles, uneven over the waves); N 4096 (one tile per workgroup: the wave-0 fold), 4144 (1 and 2 tiles), 6144
(RoPE: 1 and 2 tiles), 22016 (5 and 6 tiles: two epilogue waves, the barrier form of the fold), 32000 (7 and 8 tiles).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

f16, f32 = np.float16, np.float32
FILL = 0xAB
MAX_SEQ = 64


def _cases():
    cs = []
    for bits in (4, 8):
        b = f"w{bits}"
        # XM_F16F (folded rms_norm input) + SiLU * up
        for K, N in ((4096, 22016), (1024, 4144), (512, 4096)):
            cs.append(dict(name=f"f16f_silu_{b}_k{K}_n{N}", x="f16f", kind="silu", bits=bits, K=K, N=N))
        # XM_F16F + logits / argmax
        for K, N in ((4096, 32000), (1024, 4144)):
            cs.append(dict(name=f"f16f_argmax_{b}_k{K}_n{N}", x="f16f", kind="argmax", bits=bits, K=K, N=N))
        # XM_F16F + RoPE / KV append (the unfused route): head_dim 128 and 64, positions 0, 5, max_seq - 1
        for K, heads, kvh, hd, pos, fp8 in ((4096, 32, 8, 128, 5, 0), (1024, 32, 8, 128, MAX_SEQ - 1, 1),
                                            (512, 8, 2, 64, 0, 0), (1024, 8, 2, 64, MAX_SEQ - 1, 0)):
            cs.append(dict(name=f"f16f_rope_{b}_k{K}_hd{hd}_p{pos}_f8{fp8}", x="f16f", kind="rope", bits=bits, K=K,
                           N=(heads + 2 * kvh) * hd, heads=heads, kvh=kvh, hd=hd, pos=pos, fp8=fp8))
        # XM_ATTN (split partials merged while staging) + residual, with and without the fold
        for heads, hd, N, S, fold in ((32, 128, 4096, 8, 1), (16, 64, 4144, 2, 1), (32, 128, 22016, 8, 1),
                                      (16, 64, 4096, 2, 0)):
            cs.append(dict(name=f"attn_resid_{b}_k{heads * hd}_n{N}_s{S}_fold{fold}", x="attn", kind="resid", bits=bits,
                           K=heads * hd, N=N, heads=heads, hd=hd, S=S, fold=fold))
        # XM_F16 (one fp16 row) + residual
        for K, N, fold in ((11008, 4096, 1), (512, 4144, 1), (4096, 22016, 1), (1024, 4144, 0)):
            cs.append(dict(name=f"f16_resid_{b}_k{K}_n{N}_fold{fold}", x="f16", kind="resid", bits=bits, K=K, N=N,
                           fold=fold))
        # XM_NORM1 (rms_norm of one fp32 row in the prologue): the fold-off route's forms
        cs.append(dict(name=f"norm1_silu_{b}_k4096_n4144", x="norm1", kind="silu", bits=bits, K=4096, N=4144))
        cs.append(dict(name=f"norm1_argmax_{b}_k1024_n32000", x="norm1", kind="argmax", bits=bits, K=1024, N=32000))
        cs.append(dict(name=f"norm1_rope_{b}_k4096_hd128_p5", x="norm1", kind="rope", bits=bits, K=4096,
                       N=(32 + 2 * 8) * 128, heads=32, kvh=8, hd=128, pos=5, fp8=0))
        cs.append(dict(name=f"norm1_rope_{b}_k512_hd64_p0", x="norm1", kind="rope", bits=bits, K=512,
                       N=(8 + 2 * 2) * 64, heads=8, kvh=2, hd=64, pos=0, fp8=1))
    return cs


CASES = _cases()
NAMES = [c["name"] for c in CASES]


def run_case(ti, c):
    """One launch of the case -> ({output name: bytes as a uint8 array}, one-row launches counted)."""
    L = ti.lib()
    rng = np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7fffffff)
    keep = []

    def dev(a):
        keep.append(ti.DeviceBuffer.from_array(np.ascontiguousarray(a)))
        return keep[-1]

    def filled(nbytes):
        return dev(np.full(nbytes, FILL, np.uint8))

    bits, K, N = c["bits"], c["K"], c["N"]
    block = rng.randint(0, 256, size=1 << 20).astype(np.uint8)
    td = dev(np.resize(block, L.ti_wpack_tile_bytes(bits, K, N)))
    sd = dev(np.resize((0.005 + 0.015 * rng.rand(1 << 16)).astype(f16), L.ti_wpack_scale_bytes(bits, K, N) // 2))
    ep = ti.Epilogue()
    norm_ptr = None
    if c["x"] == "f16f":
        xd, xk = dev(rng.standard_normal(K).astype(f16)), ti.X_F16_FOLDED
        n_ss = 200
        ssd = dev((rng.rand(n_ss) * K / n_ss * 2).astype(f32))
        ep.ss_in, ep.n_ss = ssd.ptr, n_ss
    elif c["x"] == "f16":
        xd, xk = dev(rng.standard_normal(K).astype(f16)), ti.X_F16
    elif c["x"] == "norm1":
        xd, xk = dev((rng.standard_normal(K) * 3).astype(f32)), ti.X_F32_RMSNORM
        norm_ptr = dev((1 + 0.1 * rng.standard_normal(K)).astype(f32)).ptr
    else:   # the attention's split partials: normalised rows, (max, sum) pairs; the last split empty
        heads, hd, S = c["heads"], c["hd"], c["S"]
        po = rng.standard_normal((heads, S, hd)).astype(f16)
        ml = np.stack([rng.standard_normal((heads, S)) * 3, 1 + 10 * rng.rand(heads, S)], axis=-1).astype(f32)
        po[:, S - 1], ml[:, S - 1, 0], ml[:, S - 1, 1] = 0, -np.inf, 0
        xd, xk = dev(po), ti.X_ATTN_SPLITS
        mld = dev(ml)
        ep.ss_in, ep.n_ss, ep.head_dim = mld.ptr, S, hd
    outs = {}
    if c["kind"] == "resid":
        hd_ = dev((rng.standard_normal(N) * 2).astype(f32))
        ep.kind, ep.ldo, ep.out = ti.EPI_RESID_F32, N, hd_.ptr
        outs["out"] = (hd_, N * 4)
        if c["fold"]:
            fw, fx, fs = dev((1 + 0.1 * rng.standard_normal(N)).astype(f32)), filled(N * 2), filled(256 * 4)
            ep.fold_w, ep.fold_x, ep.fold_ss = fw.ptr, fx.ptr, fs.ptr
            outs["fold_x"], outs["fold_ss"] = (fx, N * 2), (fs, 256 * 4)
    elif c["kind"] == "silu":
        act = filled(N)
        ep.kind, ep.ldo, ep.out = ti.EPI_SILU_MUL_F16, N // 2, act.ptr
        outs["act"] = (act, N)
    elif c["kind"] == "argmax":
        lg, am, ctr = filled(N * 4), dev(np.zeros(ti.ARGMAX_SLOTS, np.uint64)), dev(np.array([7, 0, 0, 0], np.int32))
        ep.kind, ep.ldo, ep.out, ep.argmax, ep.step_ctr, ep.advance = ti.EPI_LOGITS_ARGMAX, N, lg.ptr, am.ptr, ctr.ptr, 3
        outs["logits"], outs["argmax"], outs["step_ctr"] = (lg, N * 4), (am, ti.ARGMAX_SLOTS * 8), (ctr, 16)
    else:
        heads, kvh, hd, esz = c["heads"], c["kvh"], c["hd"], 1 if c["fp8"] else 2
        q, kc, vc = filled(heads * hd * 4), filled(kvh * MAX_SEQ * hd * esz), filled(kvh * MAX_SEQ * hd * esz)
        pos = dev(np.array([c["pos"], 0, 0, 0], np.int32))
        cs_ = dev(rng.uniform(-1, 1, (MAX_SEQ, hd)).astype(f32))
        ep.kind, ep.ldo, ep.out = ti.EPI_QKV_ROPE_KV, heads * hd, q.ptr
        ep.q_dim, ep.kv_dim, ep.head_dim, ep.max_seq = heads * hd, kvh * hd, hd, MAX_SEQ
        ep.pos, ep.rope_cs, ep.k_cache, ep.v_cache, ep.kv_stream_stride, ep.kv_fp8 = pos.ptr, cs_.ptr, kc.ptr, vc.ptr, 0, c["fp8"]
        outs["q"], outs["k_cache"], outs["v_cache"] = (q, heads * hd * 4), (kc, kvh * MAX_SEQ * hd * esz), (vc, kvh * MAX_SEQ * hd * esz)
    n0 = L.ti_gemm_onerow_epi_launches()
    ti.check(L.ti_gemm_wq_a16(td.ptr, sd.ptr, bits, xd.ptr, xk, K, norm_ptr, 1e-5, 1, N, K, C.byref(ep), None))
    ti.sync()
    counted = int(L.ti_gemm_onerow_epi_launches() - n0)
    got = {k: b.download(np.uint8, n) for k, (b, n) in outs.items()}
    for b in keep:
        b.free()
    return got, counted


def run_all(ti):
    res = {}
    for c in CASES:
        got, counted = run_case(ti, c)
        res.update({f"{c['name']}/{k}": v for k, v in got.items()})
        res[f"{c['name']}/counted"] = np.array([counted], np.int64)
    return res


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import turboinfer_amd as T
from test_gpu_gemv_onerow_epi import run_all
T.init(0)
np.savez(sys.argv[2], **run_all(T))
"""


@pytest.fixture(scope="module")
def both(ti, tmp_path_factory):
    assert not os.environ.get("TI_GEMV_EPI_GENERIC"), "this process must run the one-row instances"
    spec = run_all(ti)
    out = str(tmp_path_factory.mktemp("onerow") / "generic.npz")
    env = dict(os.environ, TI_GEMV_EPI_GENERIC="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return spec, dict(np.load(out))


@pytest.mark.parametrize("name", NAMES)
def test_onerow_instance_matches_generic_bytes(both, name):
    spec, gen = both
    keys = sorted(k for k in spec if k.startswith(name + "/") and not k.endswith("/counted"))
    assert keys and keys == sorted(k for k in gen if k.startswith(name + "/") and not k.endswith("/counted"))
    assert int(spec[name + "/counted"][0]) == 1, "the one-row instance did not run"
    assert int(gen[name + "/counted"][0]) == 0, "TI_GEMV_EPI_GENERIC=1 did not route to the generic instance"
    for k in keys:
        a, b = spec[k], gen[k]
        assert a.shape == b.shape and a.size > 0
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{k}: {bad.size} bytes differ, first at {bad[:8]}"
    # the launch wrote something: no output is still the fill pattern
    for k in keys:
        if not k.endswith(("k_cache", "v_cache")):
            assert np.any(spec[k] != FILL), k
    if "rope" in name:   # exactly the row at p of every kv head was written
        for k in (name + "/k_cache", name + "/v_cache"):
            assert 0 < np.count_nonzero(spec[k] != FILL) <= spec[k].size // MAX_SEQ
