#!/usr/bin/env python3
"""Measurements behind gemm_w16_kernel; the output is kept as profiles/w16_rows_ab.txt.

    python tools/ab_w16_rows.py [--rounds 3] [--layers-7b 32] [--part gpd]

The two routes of fp16-weight rows above 16: `w16` (one gemm_w16_kernel launch) and `pieces` (TI_GEMM_W16_ROWS=0:
the same rows as launches of the fused gemv_wq_kernel<16, ..>, ti_gemm_max_rows rows each, what the engine did
before).  The knob is read once per process, so every (route, round) is a child process of its own and the rounds
interleave pieces, w16, pieces, w16 ..; every figure is the median [min .. max] over the rounds.
(g) Per projection shape of TinyLlama-1.1B and of the Llama-2-7B shape as fp16 (QKV, O, gate/up, down, lm_head) at
    M in {17, 64, 512, 1024}: us per call of M fp16 rows (STORE_F32), REP calls between two device synchronisations
    after one untimed call.  The w16 children also time the group-128 INT8 weight of the shape on gemm_w8_kernel
    (`int8 w8`, same process).
(p) A 512-token prompt to its first token (Engine.generate, 1 new token, wall clock, two untimed calls first).
(d) 64 streams decoding --new tokens each from one-token prompts: tok/s after the first token.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ab_w8_rows import REP, models  # noqa: E402

ROWS = (17, 64, 512, 1024)


def child(args) -> int:
    import numpy as np
    import turboinfer_amd as T
    T.init(0)
    L = T.lib()
    res = {}
    for name, m in models(args.layers_7b).items():
        qd, kvd = m["nh"] * m["hd"], m["nkv"] * m["hd"]
        shapes = {"qkv": (m["H"], qd + 2 * kvd), "o": (qd, m["H"]), "gate/up": (m["H"], 2 * m["I"]),
                  "down": (m["I"], m["H"]), "lm_head": (m["H"], m["V"])}
        if "g" in args.part:
            for sn, (K, N), b in [(sn, kn, b) for sn, kn in shapes.items()
                                  for b in ((16, 8) if L.ti_gemm_w16_rows(17, 16, 128) else (16,))]:
                td = T.DeviceBuffer(L.ti_wpack_tile_bytes(b, K, N))
                sd = T.DeviceBuffer(max(L.ti_wpack_scale_bytes(b, K, N), 16))
                T.check(L.ti_wsynth_device(7, 1, K, N, N, b, 0, 0, td.ptr, sd.ptr, None))
                xd = T.DeviceBuffer.from_array(np.random.RandomState(1).standard_normal((1024, K)).astype(np.float16))
                yd = T.DeviceBuffer(1024 * N * 4)
                for M in ROWS:
                    one = T.gemm_kernel_name(b, T.X_F16, M, N, K) in ("gemm_w16_kernel", "gemm_w8_kernel")
                    piece = M if one else L.ti_gemm_max_rows(b, T.X_F16, N, K)   # the engine's pieces (16, fewer at long K)

                    def call():
                        for m0 in range(0, M, piece):
                            ep = T.Epilogue()
                            ep.kind, ep.ldo, ep.out = T.EPI_STORE_F32, N, yd.ptr + m0 * N * 4
                            T.check(L.ti_gemm_wq_a16(td.ptr, sd.ptr, b, xd.ptr + m0 * K * 2, T.X_F16, K, None, 1e-5,
                                                     min(piece, M - m0), N, K, C.byref(ep), None))
                    call()
                    T.sync()
                    t0 = time.perf_counter()
                    for _ in range(REP):
                        call()
                    T.sync()
                    res[f"{'g' if b == 16 else 'int8'} {name} {sn} {N}x{K} M={M}"] = (time.perf_counter() - t0) / REP * 1e6
                for buf in (td, sd, xd, yd):
                    buf.free()
        if "p" in args.part or "d" in args.part:
            e = T.Engine(m["V"], m["H"], m["layers"], m["nh"], m["nkv"], m["hd"], m["I"], bits=16, max_seq=640,
                         max_batch=64, rope_theta=m["theta"])
            e.synth(0x7157, 0.0)
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
    routes = {"pieces": "0", "w16": "1"}
    got = {r: {} for r in routes}
    for rnd in range(args.rounds):
        for r, knob in routes.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--layers-7b", str(args.layers_7b),
                                "--new", str(args.new), "--part", args.part],
                               env=dict(os.environ, TI_GEMM_W16_ROWS=knob), capture_output=True, text=True, timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-2000:])
                return 1
            for k, v in json.loads(line[-1][7:]).items():
                got[r].setdefault(k, []).append(v)
            print(f"# round {rnd} {r} done", flush=True)
    print(f"fp16-weight rows above 16: pieces (TI_GEMM_W16_ROWS=0, 16-row gemv_wq_kernel<16> launches) against w16 "
          f"(gemm_w16_kernel); median [min .. max] of {args.rounds} interleaved rounds, one process per route and round; "
          f"g: us per call, x = pieces / w16; int8 w8: the group-128 INT8 weight of the shape on gemm_w8_kernel in the "
          f"w16 process, x = w16 / int8 w8")

    def spread(v):
        return f"{statistics.median(v):10.1f} [{min(v):9.1f} .. {max(v):9.1f}]"
    for k in got["w16"]:
        if k.startswith("int8"):
            continue
        a, b = got["pieces"][k], got["w16"][k]
        ratio = statistics.median(a) / statistics.median(b)
        i8 = got["w16"].get("int8" + k[1:])
        beside = f"   int8 w8 {spread(i8)}   x{statistics.median(b) / statistics.median(i8):5.2f}" if i8 else ""
        print(f"{k:72s} pieces {spread(a)}   w16 {spread(b)}   x{ratio if k[0] != 'd' else 1 / ratio:6.2f}{beside}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
