#!/usr/bin/env python3
"""Measurements behind gemm_w8_kernel; the output is kept as profiles/w8_rows_ab.txt and, with
--g32 (Q8_0 blocks, bits 8 | BITS_G32), as profiles/w8_g32_rows_ab.txt.

    python tools/ab_w8_rows.py [--g32] [--rounds 3] [--layers-7b 32] [--part gpd]

The two routes of INT8 rows above 16: `w8` (one gemm_w8_kernel launch) and `pieces` (TI_GEMM_W8_ROWS=0: the same
rows as launches of the fused gemv_wq_kernel, ti_gemm_max_rows rows each (16, fewer at long K), what the engine did before).  The knob is read once per
process, so every (route, round) is a child process of its own and the rounds interleave pieces, w8, pieces, w8 ..;
every figure is the median [min .. max] over the rounds.
(g) Per projection shape of TinyLlama-1.1B and of the Llama-2-7B shape as INT8 (QKV, O, gate/up, down, lm_head) at
    M in {17, 32, 64, 128, 512, 1024}: us per call of M fp16 rows (STORE_F32), REP calls between two device
    synchronisations after one untimed call.
(p) A 512-token prompt to its first token (Engine.generate, 1 new token, wall clock, one untimed call first).
(d) 64 streams decoding --new tokens each from one-token prompts: tok/s after the first token.
--g32: the weights are random Q8_0 blocks packed on the host (ti_wpack_q_host / set_tensor_q: the synthesiser has
no group-32 format), `pieces` is what ti_gemm_wq_a16 and the engine do with TI_GEMM_W8_ROWS=0 and did before the
group-32 instance, and (g) also times the group-128 INT8 weight of the same shape on gemm_w8_kernel (`g128`).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import MODELS  # noqa: E402

REP = 10
ROWS = (17, 32, 64, 128, 512, 1024)


def models(layers_7b):
    out = {}
    for name in ("tinyllama-1.1b", "llama2-7b"):
        V, H, layers, nh, nkv, hd, I, _, theta = MODELS[name]
        out[name] = dict(V=V, H=H, layers=layers_7b if name == "llama2-7b" else layers, nh=nh, nkv=nkv, hd=hd, I=I, theta=theta)
    return out


def q8_0_blocks(np, K, N):
    """Random Q8_0 blocks (q int8 [K][N], d fp16 [K/32][N]) of test_gpu_g32.py's amplitude, for timing."""
    rng = np.random.default_rng(K + N)
    q = rng.integers(-127, 128, (K, N), dtype=np.int8)
    d = (rng.uniform(0.5, 1.5, (K // 32, N)) * (0.3 / np.sqrt(K) / 64.0)).astype(np.float16)
    return q, d


def device_weight(T, np, bits, K, N):
    L = T.lib()
    td, sd = T.DeviceBuffer(L.ti_wpack_tile_bytes(bits, K, N)), T.DeviceBuffer(L.ti_wpack_scale_bytes(bits, K, N))
    if bits & T.BITS_G32:
        q, d = q8_0_blocks(np, K, N)
        tiles, scales = np.zeros(td.nbytes, np.uint8), np.zeros(sd.nbytes // 2, np.uint16)
        T.check(L.ti_wpack_q_host(q.ctypes.data, d.view(np.uint16).ctypes.data, K, N, N, 8, 0, 0, tiles.ctypes.data,
                                  scales.ctypes.data))
        td.upload(tiles), sd.upload(scales)
    else:
        T.check(L.ti_wsynth_device(7, 1, K, N, N, bits, 0, 0, td.ptr, sd.ptr, None))
    return td, sd


def q8_0_engine(T, np, m):
    """An 8 | BITS_G32 engine of model m; every layer holds the same random blocks (timing only)."""
    e = T.Engine(m["V"], m["H"], m["layers"], m["nh"], m["nkv"], m["hd"], m["I"], bits=8 | T.BITS_G32, max_seq=640,
                 max_batch=64, rope_theta=m["theta"])
    H, I, qd, kvd = m["H"], m["I"], m["nh"] * m["hd"], m["nkv"] * m["hd"]
    e.set_tensor(T.E_EMBED, 0, (np.random.default_rng(1).standard_normal((m["V"], H)) * 0.02).astype(np.float32))
    e.set_tensor(T.V_OUT_NORM, 0, np.ones(H, np.float32))
    e.set_tensor_q(T.W_LM_HEAD, 0, *q8_0_blocks(np, H, m["V"]))
    slots = [(T.W_Q, H, qd), (T.W_K, H, kvd), (T.W_V, H, kvd), (T.W_O, qd, H), (T.W_GATE, H, I), (T.W_UP, H, I),
             (T.W_DOWN, I, H)]
    blocks = [q8_0_blocks(np, K, N) for _, K, N in slots]
    for l in range(m["layers"]):
        e.set_tensor(T.V_ATTN_NORM, l, np.ones(H, np.float32))
        e.set_tensor(T.V_FFN_NORM, l, np.ones(H, np.float32))
        for (slot, _, _), (q, d) in zip(slots, blocks):
            e.set_tensor_q(slot, l, q, d)
    return e


def child(args) -> int:
    import numpy as np
    import turboinfer_amd as T
    T.init(0)
    L = T.lib()
    res = {}
    bits = 8 | T.BITS_G32 if args.g32 else 8
    for name, m in models(args.layers_7b).items():
        qd, kvd = m["nh"] * m["hd"], m["nkv"] * m["hd"]
        shapes = {"qkv": (m["H"], qd + 2 * kvd), "o": (qd, m["H"]), "gate/up": (m["H"], 2 * m["I"]),
                  "down": (m["I"], m["H"]), "lm_head": (m["H"], m["V"])}
        if "g" in args.part:
            # (--g32, route on: the group-128 weight of the shape as well)
            for sn, (K, N), b in [(sn, kn, b) for sn, kn in shapes.items()
                                  for b in ((bits, 8) if args.g32 and L.ti_gemm_w8_rows(17, 16, 128) else (bits,))]:
                td, sd = device_weight(T, np, b, K, N)
                xd = T.DeviceBuffer.from_array(np.random.RandomState(1).standard_normal((1024, K)).astype(np.float16))
                yd = T.DeviceBuffer(1024 * N * 4)
                for M in ROWS:
                    w8 = T.gemm_kernel_name(b, T.X_F16, M, N, K) == "gemm_w8_kernel"
                    piece = M if w8 else L.ti_gemm_max_rows(b, T.X_F16, N, K)     # the engine's pieces (16, fewer at long K)

                    def call():
                        for m0 in range(0, M, piece):
                            mm = min(piece, M - m0)
                            ep = T.Epilogue()
                            ep.kind, ep.ldo, ep.out = T.EPI_STORE_F32, N, yd.ptr + m0 * N * 4
                            T.check(L.ti_gemm_wq_a16(td.ptr, sd.ptr, b, xd.ptr + m0 * K * 2, T.X_F16, K, None, 1e-5, mm, N, K,
                                                     C.byref(ep), None))
                    call()
                    T.sync()
                    t0 = time.perf_counter()
                    for _ in range(REP):
                        call()
                    T.sync()
                    res[f"{'g' if b == bits else 'g128'} {name} {sn} {N}x{K} M={M}"] = (time.perf_counter() - t0) / REP * 1e6
                for buf in (td, sd, xd, yd):
                    buf.free()
        if "p" in args.part or "d" in args.part:
            if args.g32:
                e = q8_0_engine(T, np, m)
            else:
                e = T.Engine(m["V"], m["H"], m["layers"], m["nh"], m["nkv"], m["hd"], m["I"], bits=8, max_seq=640,
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
    ap.add_argument("--g32", action="store_true", help="Q8_0 blocks (8 | BITS_G32) instead of group-128 INT8")
    args = ap.parse_args()
    if args.child:
        return child(args)
    routes = {"pieces": "0", "w8": "1"}
    got = {r: {} for r in routes}
    for rnd in range(args.rounds):
        for r, knob in routes.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--layers-7b", str(args.layers_7b),
                                "--new", str(args.new), "--part", args.part] + (["--g32"] if args.g32 else []),
                               env=dict(os.environ, TI_GEMM_W8_ROWS=knob), capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-2000:])
                return 1
            for k, v in json.loads(line[-1][7:]).items():
                got[r].setdefault(k, []).append(v)
            print(f"# round {rnd} {r} done", flush=True)
    print(f"{'Q8_0 (8 | BITS_G32)' if args.g32 else 'INT8'} rows above 16: pieces (TI_GEMM_W8_ROWS=0, 16-row gemv_wq_kernel launches) against w8 (gemm_w8_kernel); "
          f"median [min .. max] of {args.rounds} interleaved rounds, one process per route and round; g: us per call, "
          f"x = pieces / w8" + ("; g128 w8: the group-128 INT8 weight of the shape on gemm_w8_kernel, x = w8 / g128 w8"
                                if args.g32 else ""))

    def spread(v):
        return f"{statistics.median(v):10.1f} [{min(v):9.1f} .. {max(v):9.1f}]"
    for k in got["w8"]:
        if k.startswith("g128"):
            continue
        a, b = got["pieces"][k], got["w8"][k]
        ratio = statistics.median(a) / statistics.median(b)
        g128 = got["w8"].get("g128" + k[1:])   # (--g32: the group-128 weight on gemm_w8_kernel; x = g32 / g128)
        beside = f"   g128 w8 {spread(g128)}   x{statistics.median(b) / statistics.median(g128):5.2f}" if g128 else ""
        print(f"{k:72s} pieces {spread(a)}   w8 {spread(b)}   x{ratio if k[0] != 'd' else 1 / ratio:6.2f}{beside}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
