#!/usr/bin/env python3
"""Measurements behind gemm_mx_kernel; the output is kept as profiles/mx_rows_ab.txt.

    python tools/ab_mx_rows.py [--rounds 3] [--layers-7b 32] [--part gpd]

The two routes of MXFP4 rows above 16: `mx` (TI_GEMM_MX_ROWS=1: one gemm_mx_kernel launch) and `pieces`
(TI_GEMM_MX_ROWS=0, the default: the same rows as 16-row launches of the fused gemv_mx_kernel, the only route before
this kernel).  An engine samples the switch when it is created, so every (route, round) is a fresh child process
with the switch set by its environment, and the rounds interleave pieces, mx, pieces, mx ..; every child runs under
its own `timeout` and the first one that fails ends the run.  Every figure is the median [min .. max] over the rounds.
(g) us per call of M fp16 rows (STORE_F32) at M in {17, 64, 512, 1024}, REP calls between two device
    synchronisations after one untimed call: TinyLlama-1.1B QKV and gate/up, the Llama-2-7B shape's QKV, O, down and
    lm_head.  Beside each: gemm_w4a_kernel's median of the same shape from profiles/w4a_rows_ab.txt where that file
    has it (`q4_1`, an earlier run of tools/ab_w4a_rows.py, for information; x = mx / q4_1).
(p) A 512-token prompt to its first token (Engine.generate, 1 new token, wall clock, two untimed calls first).
(d) 64 streams decoding --new tokens each from one-token prompts: tok/s after the first token.
Every layer of an engine holds the same random blocks (timing only).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ab_w8_rows import REP, models  # noqa: E402

ROWS = (17, 64, 512, 1024)
SHAPES = {"tinyllama-1.1b": ("qkv", "gate/up"), "llama2-7b": ("qkv", "o", "down", "lm_head")}
CHILD_SECONDS = 600


def mx_blocks(np, K, N):
    """Random MXFP4 blocks (codes 0..15 [K][N], e8m0 [K/32][N] within 2x of 0.1 / sqrt(K)), for timing."""
    rng = np.random.default_rng(K + N)
    e = 127 + int(np.round(np.log2(0.1 / np.sqrt(K)))) + rng.integers(-1, 2, (K // 32, N))
    return rng.integers(0, 16, (K, N), dtype=np.uint8), e.astype(np.uint8)


def mx_engine(T, np, m):
    e = T.Engine(m["V"], m["H"], m["layers"], m["nh"], m["nkv"], m["hd"], m["I"], bits=4 | T.BITS_G32 | T.BITS_MX,
                 max_seq=640, max_batch=64, rope_theta=m["theta"])
    H, I, qd, kvd = m["H"], m["I"], m["nh"] * m["hd"], m["nkv"] * m["hd"]
    e.set_tensor(T.E_EMBED, 0, (np.random.default_rng(1).standard_normal((m["V"], H)) * 0.02).astype(np.float32))
    e.set_tensor(T.V_OUT_NORM, 0, np.ones(H, np.float32))
    e.set_tensor_mx(T.W_LM_HEAD, 0, *mx_blocks(np, H, m["V"]))
    slots = [(T.W_Q, H, qd), (T.W_K, H, kvd), (T.W_V, H, kvd), (T.W_O, qd, H), (T.W_GATE, H, I), (T.W_UP, H, I),
             (T.W_DOWN, I, H)]
    blocks = [mx_blocks(np, K, N) for _, K, N in slots]
    for l in range(m["layers"]):
        e.set_tensor(T.V_ATTN_NORM, l, np.ones(H, np.float32))
        e.set_tensor(T.V_FFN_NORM, l, np.ones(H, np.float32))
        for (slot, _, _), b in zip(slots, blocks):
            e.set_tensor_mx(slot, l, *b)
    return e


def child(args) -> int:
    import numpy as np
    import turboinfer_amd as T
    T.init(0)
    L = T.lib()
    res, bits = {}, 4 | T.BITS_G32 | T.BITS_MX
    for name, m in models(args.layers_7b).items():
        qd, kvd = m["nh"] * m["hd"], m["nkv"] * m["hd"]
        shapes = {"qkv": (m["H"], qd + 2 * kvd), "o": (qd, m["H"]), "gate/up": (m["H"], 2 * m["I"]),
                  "down": (m["I"], m["H"]), "lm_head": (m["H"], m["V"])}
        if "g" in args.part:
            for sn in SHAPES[name]:
                K, N = shapes[sn]
                td, sd = (T.DeviceBuffer.from_array(a) for a in T.wpack_mx(*mx_blocks(np, K, N)))
                xd = T.DeviceBuffer.from_array(np.random.RandomState(1).standard_normal((1024, K)).astype(np.float16))
                yd = T.DeviceBuffer(1024 * N * 4)
                for M in ROWS:
                    piece = M if L.ti_gemm_mx_rows(M, N, K) else 16   # (switch off: the engine's pieces)

                    def call():
                        for m0 in range(0, M, piece):
                            ep = T.Epilogue()
                            ep.kind, ep.ldo, ep.out = T.EPI_STORE_F32, N, yd.ptr + m0 * N * 4
                            T.check(L.ti_gemm_wq_a16(td.ptr, sd.ptr, bits, xd.ptr + m0 * K * 2, T.X_F16, K, None, 1e-5,
                                                     min(piece, M - m0), N, K, C.byref(ep), None))
                    call()
                    T.sync()
                    t0 = time.perf_counter()
                    for _ in range(REP):
                        call()
                    T.sync()
                    res[f"g {name} {sn} {N}x{K} M={M}"] = (time.perf_counter() - t0) / REP * 1e6
                for buf in (td, sd, xd, yd):
                    buf.free()
        if "p" in args.part or "d" in args.part:
            e = mx_engine(T, np, m)
            rng = np.random.default_rng(7)
            if "p" in args.part:
                prompt = rng.integers(3, m["V"], 512).tolist()
                for i in range(3):
                    t0 = time.perf_counter()
                    e.generate([prompt], 1)
                    dt = time.perf_counter() - t0
                res[f"p {name} ({m['layers']} layers) 512-token prompt to first token, ms"] = dt * 1e3
            if "d" in args.part:
                own = [[int(t)] for t in rng.integers(3, m["V"], 64)]
                ts = {}
                for new in (1, args.new, 1, args.new):          # the first pair untimed (graph capture)
                    t0 = time.perf_counter()
                    e.generate(own, new)
                    ts[new] = time.perf_counter() - t0
                res[f"d {name} ({m['layers']} layers) 64-stream decode, tok/s"] = 64 * (args.new - 1) / (ts[args.new] - ts[1])
            e.close()
    print("RESULT " + json.dumps(res))
    return 0


def q4_1_medians():
    """{key: gemm_w4a_kernel's median us} from profiles/w4a_rows_ab.txt (absent: {})."""
    out, path = {}, os.path.join(ROOT, "profiles", "w4a_rows_ab.txt")
    if os.path.exists(path):
        for ln in open(path):
            mt = re.match(r"(g .*? M=\d+)\s+pieces .*? w4a\s+([0-9.]+) \[", ln)
            if mt:
                out[mt.group(1)] = float(mt.group(2))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers-7b", type=int, default=32)
    ap.add_argument("--new", type=int, default=33)
    ap.add_argument("--part", default="gpd")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    routes = {"pieces": "0", "mx": "1"}
    got = {r: {} for r in routes}
    for rnd in range(args.rounds):
        for r, knob in routes.items():
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__),
                                "--child", "--layers-7b", str(args.layers_7b), "--new", str(args.new), "--part", args.part],
                               env=dict(os.environ, TI_GEMM_MX_ROWS=knob), capture_output=True, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:   # nothing more starts on the GPU after a failure
                print(f"# round {rnd} {r}: exit status {p.returncode}", p.stdout[-2000:], p.stderr[-2000:])
                return 1
            for k, v in json.loads(line[-1][7:]).items():
                got[r].setdefault(k, []).append(v)
            print(f"# round {rnd} {r} done", flush=True)
    print(f"MXFP4 rows above 16: pieces (TI_GEMM_MX_ROWS=0, 16-row gemv_mx_kernel launches) against mx (TI_GEMM_MX_ROWS=1, "
          f"gemm_mx_kernel); median [min .. max] of {args.rounds} interleaved rounds, one process per route and round; "
          f"g: us per call, x = pieces / mx; q4_1: gemm_w4a_kernel's median from profiles/w4a_rows_ab.txt (an earlier "
          f"run), x = mx / q4_1 (byte model 1088 / 1280 = 0.85)")

    def spread(v):
        return f"{statistics.median(v):10.1f} [{min(v):9.1f} .. {max(v):9.1f}]"
    q41 = q4_1_medians()
    for k in got["mx"]:
        a, b = got["pieces"][k], got["mx"][k]
        ratio = statistics.median(a) / statistics.median(b)
        apart = min(a) > max(b) if k[0] != "d" else max(a) < min(b)   # faster by more than both routes' spreads
        beside = f"   q4_1 {q41[k]:10.1f}   x{statistics.median(b) / q41[k]:5.2f}" if k in q41 else ""
        print(f"{k:72s} pieces {spread(a)}   mx {spread(b)}   x{ratio if k[0] != 'd' else 1 / ratio:6.2f}"
              f"{'' if apart else '  (spreads overlap)'}{beside}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
