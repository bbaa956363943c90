#!/usr/bin/env python3
"""Measurements behind gemv_mx_kernel; the output is kept as profiles/mx_gemv_ab.txt.

    python tools/ab_mx_gemv.py [--rounds 3] [--layers-7b 8] [--steps 256]

MXFP4 weights (4 | BITS_G32 | BITS_MX, gemv_mx_kernel) against Q4_0 weights (4 | BITS_G32, the group-32 instance of
gemv_wq_kernel) on engines of the TinyLlama-1.1B and the Llama-2-7B shape whose every layer holds the same random
blocks (timing only).  Every (format, round) is a child process of its own and the rounds interleave q4_0, mx, q4_0,
mx ..; every figure is the median [min .. max] over the rounds.
(g) The one-row launch of each projection (QKV, O, gate/up, down, lm_head): Engine.time_kernel, REPS launches
    cycling through the layers in one captured graph between two device events, us per launch.
(t) One-stream decode, tok/s: STEPS replayed step graphs at KV length 512 after 16 untimed ones (the engine's own
    launches: both formats run without the folded rms_norm hand-off and without the fused QKV + attention launch).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ab_w8_rows import models  # noqa: E402

REPS, KV = 400, 512
KINDS = ("qkv", "o", "gate/up", "down", "lm_head")


def engine(T, np, m, fmt):
    mx = fmt == "mx"
    e = T.Engine(m["V"], m["H"], m["layers"], m["nh"], m["nkv"], m["hd"], m["I"], max_seq=KV + 512, max_batch=1,
                 bits=4 | T.BITS_G32 | (T.BITS_MX if mx else 0), rope_theta=m["theta"])
    H, I, qd, kvd = m["H"], m["I"], m["nh"] * m["hd"], m["nkv"] * m["hd"]

    def blocks(K, N):   # weights of a trained model's size in either format
        rng = np.random.default_rng(K + N)
        if mx:
            e8 = 127 + int(np.round(np.log2(0.1 / np.sqrt(K)))) + rng.integers(-1, 2, (K // 32, N))
            return rng.integers(0, 16, (K, N), dtype=np.uint8), e8.astype(np.uint8)
        d = (rng.uniform(0.5, 1.5, (K // 32, N)) * (0.3 / np.sqrt(K) / 4.0)).astype(np.float16)
        return rng.integers(-8, 8, (K, N), dtype=np.int8), d
    put = e.set_tensor_mx if mx else e.set_tensor_q
    e.set_tensor(T.E_EMBED, 0, (np.random.default_rng(1).standard_normal((m["V"], H)) * 0.02).astype(np.float32))
    e.set_tensor(T.V_OUT_NORM, 0, np.ones(H, np.float32))
    put(T.W_LM_HEAD, 0, *blocks(H, m["V"]))
    slots = [(T.W_Q, H, qd), (T.W_K, H, kvd), (T.W_V, H, kvd), (T.W_O, qd, H), (T.W_GATE, H, I), (T.W_UP, H, I),
             (T.W_DOWN, I, H)]
    made = [blocks(K, N) for _, K, N in slots]
    for l in range(m["layers"]):
        e.set_tensor(T.V_ATTN_NORM, l, np.ones(H, np.float32))
        e.set_tensor(T.V_FFN_NORM, l, np.ones(H, np.float32))
        for (slot, _, _), b in zip(slots, made):
            put(slot, l, *b)
    return e


def child(args) -> int:
    import numpy as np
    import turboinfer_amd as T
    T.init(0)
    res = {}
    for name, m in models(args.layers_7b).items():
        e = engine(T, np, m, args.child)
        e.fill_kv(0, KV, 5)
        for which, kind in enumerate(KINDS):
            e.time_kernel(which, 1, KV, REPS)
            us, by = e.time_kernel(which, 1, KV, REPS)
            res[f"g {name} {kind}, us per launch"] = us
            res[f"b {name} {kind}, weight + scale MB per launch"] = by / 1e6
        e.replay_prepare(1, KV, 5)
        e.replay_run(16)
        e.sync()
        t0 = time.perf_counter()
        e.replay_run(args.steps)
        e.sync()
        res[f"t {name} ({m['layers']} layers) one-stream decode at KV {KV}, tok/s"] = args.steps / (time.perf_counter() - t0)
        e.close()
    print("RESULT " + json.dumps(res))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers-7b", type=int, default=8)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    got = {"q4_0": {}, "mx": {}}
    for rnd in range(args.rounds):
        for fmt in got:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", fmt, "--layers-7b",
                                str(args.layers_7b), "--steps", str(args.steps)], capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-2000:])
                return 1
            for k, v in json.loads(line[-1][7:]).items():
                got[fmt].setdefault(k, []).append(v)
            print(f"# round {rnd} {fmt} done", flush=True)
    print(f"MXFP4 (gemv_mx_kernel) against Q4_0 (gemv_wq_kernel<4, .., G32>), one row; median [min .. max] of {args.rounds} "
          f"interleaved rounds, one process per format and round; x = q4_0 / mx for us and MB, mx / q4_0 for tok/s")

    def spread(v):
        return f"{statistics.median(v):9.2f} [{min(v):9.2f} .. {max(v):9.2f}]"
    for k in got["mx"]:
        a, b = got["q4_0"][k], got["mx"][k]
        r = statistics.median(a) / statistics.median(b)
        print(f"{k:66s} q4_0 {spread(a)}   mx {spread(b)}   x{1 / r if k[0] == 't' else r:5.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
