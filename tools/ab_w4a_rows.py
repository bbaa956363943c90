#!/usr/bin/env python3
"""Measurements behind gemm_w4a_kernel; the output is kept as profiles/w4a_rows_ab.txt.

    python tools/ab_w4a_rows.py [--rounds 3] [--layers-7b 32] [--part gpd]

The two routes of Q4_1 rows above 16: `w4a` (one gemm_w4a_kernel launch) and `pieces` (TI_GEMM_W4A_ROWS=0: the same
rows as 16-row launches of the fused gemv_wq_kernel<4, .., G32, AFF>, what the engine did before).  The knob is read
once per process, so every (route, round) is a child process of its own and the rounds interleave pieces, w4a,
pieces, w4a ..; every figure is the median [min .. max] over the rounds.
(g) Per projection shape of TinyLlama-1.1B and of the Llama-2-7B shape as Q4_1 (QKV, O, gate/up, down, lm_head) at
    M in {17, 64, 512, 1024}: us per call of M fp16 rows (STORE_F32), REP calls between two device synchronisations
    after one untimed call.  The w4a children also time the Q4_0 weight of the shape (4 | BITS_G32, the same nibbles
    and scales without minimums) on the rows / tile kernels (`q4_0`, same process; for information).
(p) A 512-token prompt to its first token (Engine.generate, 1 new token, wall clock, two untimed calls first).
(d) 64 streams decoding --new tokens each from one-token prompts: tok/s after the first token.
Every layer of an engine holds the same random blocks (timing only).
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


def q4_1_blocks(np, K, N):
    """Random Q4_1 blocks (q 0..15 [K][N], fp16 d and m [K/32][N]) of test_gpu_g32.py's amplitude."""
    rng = np.random.default_rng(K + N)
    q = rng.integers(0, 16, (K, N), dtype=np.uint8)
    d = (rng.uniform(0.5, 1.5, (K // 32, N)) * (0.3 / np.sqrt(K) / 4.0)).astype(np.float16)
    return q, d, (-d.astype(np.float32) * rng.uniform(5.0, 11.0, d.shape)).astype(np.float16)


def device_weight(T, np, bits, K, N):
    L = T.lib()
    q, d, m = q4_1_blocks(np, K, N)
    tiles = np.zeros(L.ti_wpack_tile_bytes(bits, K, N), np.uint8)
    scales = np.zeros(L.ti_wpack_scale_bytes(bits, K, N) // 2, np.uint16)
    if bits & T.BITS_AFF:
        T.check(L.ti_wpack_q1_host(q.ctypes.data, d.view(np.uint16).ctypes.data, m.view(np.uint16).ctypes.data, K, N, N,
                                   0, 0, tiles.ctypes.data, scales.ctypes.data))
    else:
        q0 = (q.astype(np.int8) - 8)
        T.check(L.ti_wpack_q_host(q0.ctypes.data, d.view(np.uint16).ctypes.data, K, N, N, 4, 0, 0, tiles.ctypes.data,
                                  scales.ctypes.data))
    return T.DeviceBuffer.from_array(tiles), T.DeviceBuffer.from_array(scales)


def q4_1_engine(T, np, m):
    e = T.Engine(m["V"], m["H"], m["layers"], m["nh"], m["nkv"], m["hd"], m["I"], bits=4 | T.BITS_G32 | T.BITS_AFF,
                 max_seq=640, max_batch=64, rope_theta=m["theta"])
    H, I, qd, kvd = m["H"], m["I"], m["nh"] * m["hd"], m["nkv"] * m["hd"]
    e.set_tensor(T.E_EMBED, 0, (np.random.default_rng(1).standard_normal((m["V"], H)) * 0.02).astype(np.float32))
    e.set_tensor(T.V_OUT_NORM, 0, np.ones(H, np.float32))
    e.set_tensor_q1(T.W_LM_HEAD, 0, *q4_1_blocks(np, H, m["V"]))
    slots = [(T.W_Q, H, qd), (T.W_K, H, kvd), (T.W_V, H, kvd), (T.W_O, qd, H), (T.W_GATE, H, I), (T.W_UP, H, I),
             (T.W_DOWN, I, H)]
    blocks = [q4_1_blocks(np, K, N) for _, K, N in slots]
    for l in range(m["layers"]):
        e.set_tensor(T.V_ATTN_NORM, l, np.ones(H, np.float32))
        e.set_tensor(T.V_FFN_NORM, l, np.ones(H, np.float32))
        for (slot, _, _), b in zip(slots, blocks):
            e.set_tensor_q1(slot, l, *b)
    return e


def child(args) -> int:
    import numpy as np
    import turboinfer_amd as T
    T.init(0)
    L = T.lib()
    res, q41 = {}, 4 | T.BITS_G32 | T.BITS_AFF
    for name, m in models(args.layers_7b).items():
        qd, kvd = m["nh"] * m["hd"], m["nkv"] * m["hd"]
        shapes = {"qkv": (m["H"], qd + 2 * kvd), "o": (qd, m["H"]), "gate/up": (m["H"], 2 * m["I"]),
                  "down": (m["I"], m["H"]), "lm_head": (m["H"], m["V"])}
        if "g" in args.part:
            for sn, (K, N), b in [(sn, kn, b) for sn, kn in shapes.items()
                                  for b in ((q41, 4 | T.BITS_G32) if L.ti_gemm_w4a_rows(17, 16, 128) else (q41,))]:
                td, sd = device_weight(T, np, b, K, N)
                xd = T.DeviceBuffer.from_array(np.random.RandomState(1).standard_normal((1024, K)).astype(np.float16))
                yd = T.DeviceBuffer(1024 * N * 4)
                for M in ROWS:
                    piece = 16 if b == q41 and not L.ti_gemm_w4a_rows(M, N, K) else M   # the engine's pieces

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
                    res[f"{'g' if b == q41 else 'q4_0'} {name} {sn} {N}x{K} M={M}"] = (time.perf_counter() - t0) / REP * 1e6
                for buf in (td, sd, xd, yd):
                    buf.free()
        if "p" in args.part or "d" in args.part:
            e = q4_1_engine(T, np, m)
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
    routes = {"pieces": "0", "w4a": "1"}
    got = {r: {} for r in routes}
    for rnd in range(args.rounds):
        for r, knob in routes.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--layers-7b", str(args.layers_7b),
                                "--new", str(args.new), "--part", args.part],
                               env=dict(os.environ, TI_GEMM_W4A_ROWS=knob), capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-2000:])
                return 1
            for k, v in json.loads(line[-1][7:]).items():
                got[r].setdefault(k, []).append(v)
            print(f"# round {rnd} {r} done", flush=True)
    print(f"Q4_1 rows above 16: pieces (TI_GEMM_W4A_ROWS=0, 16-row gemv_wq_kernel<4, G32, AFF> launches) against w4a "
          f"(gemm_w4a_kernel); median [min .. max] of {args.rounds} interleaved rounds, one process per route and round; "
          f"g: us per call, x = pieces / w4a; q4_0: the Q4_0 weight of the shape on the rows / tile kernels in the w4a "
          f"process, x = w4a / q4_0")

    def spread(v):
        return f"{statistics.median(v):10.1f} [{min(v):9.1f} .. {max(v):9.1f}]"
    for k in got["w4a"]:
        if k.startswith("q4_0"):
            continue
        a, b = got["pieces"][k], got["w4a"][k]
        ratio = statistics.median(a) / statistics.median(b)
        q0 = got["w4a"].get("q4_0" + k[1:])
        beside = f"   q4_0 {spread(q0)}   x{statistics.median(b) / statistics.median(q0):5.2f}" if q0 else ""
        print(f"{k:72s} pieces {spread(a)}   w4a {spread(b)}   x{ratio if k[0] != 'd' else 1 / ratio:6.2f}{beside}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
