#!/usr/bin/env python3
"""Measurements behind gemv_kq_kernel; the output is kept as profiles/kq_gemv_ab.txt.

    python tools/ab_kq_gemv.py [--rounds 3] [--layers-7b 8] [--steps 256]

Q4_K weights (4 | BITS_G32 | BITS_KQ, gemv_kq_kernel) against Q4_0 (4 | BITS_G32, the same 4.5 bits per weight) and
Q4_1 (4 | BITS_G32 | BITS_AFF, 5 bits; both the group-32 instances of gemv_wq_kernel) on engines of the
TinyLlama-1.1B and the Llama-2-7B shape whose every layer holds the same random blocks (timing only).  Every
(format, round) is a child process of its own and the rounds interleave q4_0, q4_1, kq, q4_0, ..; every figure is the
median [min .. max] over the rounds.
(g) The one-row launch of each projection (QKV, O, gate/up, down, lm_head): Engine.time_kernel, REPS launches
    cycling through the layers in one captured graph between two device events, us per launch.
(r) The same at 16 rows: one launch for Q4_0 / Q4_1 where the LDS image holds 16 rows, 15 + 1 for Q4_K at K = 4096.
(t) One-stream decode, tok/s: STEPS replayed step graphs at KV length 512 after 16 untimed ones (the engine's own
    launches: no format here runs the folded rms_norm hand-off or the fused QKV + attention launch).
(c) MB the graph of (g) cycles through (the launch's weights and scales times the layers; the lm_head is one tensor):
    at or under IC_MB the weights can stay in the Infinity Cache from one cycle to the next, and (g) is then no HBM
    figure.
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

REPS, KV, IC_MB = 400, 512, 256
KINDS = ("qkv", "o", "gate/up", "down", "lm_head")
FORMATS = ("q4_0", "q4_1", "kq")


def engine(T, np, m, fmt):
    bits = 4 | T.BITS_G32 | {"q4_0": 0, "q4_1": T.BITS_AFF, "kq": T.BITS_KQ}[fmt]
    e = T.Engine(m["V"], m["H"], m["layers"], m["nh"], m["nkv"], m["hd"], m["I"], max_seq=KV + 512, max_batch=16,
                 bits=bits, rope_theta=m["theta"])
    H, I, qd, kvd = m["H"], m["I"], m["nh"] * m["hd"], m["nkv"] * m["hd"]

    def blocks(K, N):   # zero-centred weights of a trained model's size (about 0.3 / sqrt(K)) in each format
        rng = np.random.default_rng(K + N)
        a = 0.3 / np.sqrt(K)
        if fmt == "q4_0":
            return rng.integers(-8, 8, (K, N), dtype=np.int8), (rng.uniform(0.5, 1.5, (K // 32, N)) * a / 4).astype(np.float16)
        q = rng.integers(0, 16, (K, N), dtype=np.uint8)
        if fmt == "q4_1":
            d = (rng.uniform(0.5, 1.5, (K // 32, N)) * a / 4).astype(np.float16)
            return q, d, (-7.5 * d.astype(np.float32)).astype(np.float16)
        sc = rng.integers(0, 64, (K // 32, N), dtype=np.uint8)   # dmin m near 7.5 d sc, as a quantizer leaves it
        mn = np.clip(sc.astype(np.int32) + rng.integers(-2, 3, sc.shape), 0, 63).astype(np.uint8)
        d = (rng.uniform(0.5, 1.5, (K // 256, N)) * a / 128).astype(np.float16)
        return q, sc, mn, d, (7.5 * d.astype(np.float32)).astype(np.float16)
    put = {"q4_0": e.set_tensor_q, "q4_1": e.set_tensor_q1, "kq": e.set_tensor_kq}[fmt]
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
        for s in range(16):
            e.fill_kv(s, KV, 5)
        for which, kind in enumerate(KINDS):
            for rows, tag in ((1, "g"), (16, "r")):
                e.time_kernel(which, rows, KV, REPS)
                us, by = e.time_kernel(which, rows, KV, REPS)
                res[f"{tag} {name} {kind}, {rows} row(s), us per launch"] = us
                if rows == 1:
                    res[f"c {name} {kind}, MB cycled by (g)"] = by / 1e6 * (1 if kind == "lm_head" else m["layers"])
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
    got = {f: {} for f in FORMATS}
    for rnd in range(args.rounds):
        for fmt in FORMATS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", fmt, "--layers-7b",
                                str(args.layers_7b), "--steps", str(args.steps)], capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-2000:])
                return 1
            for k, v in json.loads(line[-1][7:]).items():
                got[fmt].setdefault(k, []).append(v)
            print(f"# round {rnd} {fmt} done", flush=True)
    print(f"Q4_K (gemv_kq_kernel) against Q4_0 and Q4_1 (gemv_wq_kernel<4, .., G32[, AFF]>); median [min .. max] of "
          f"{args.rounds} interleaved rounds, one process per format and round; x0 = q4_0 / kq and x1 = q4_1 / kq for us and "
          f"MB, kq / q4_0 and kq / q4_1 for tok/s; * = the cycle fits the {IC_MB} MB Infinity Cache in every format")

    def spread(v):
        return f"{statistics.median(v):8.2f} [{min(v):8.2f} .. {max(v):8.2f}]"
    for k in got["kq"]:
        a, b, c = (got[f][k] for f in FORMATS)
        x0, x1 = (statistics.median(v) / statistics.median(c) for v in (a, b))
        if k[0] == "t":
            x0, x1 = 1 / x0, 1 / x1
        star = "*" if k[0] == "c" and max(a + b + c) <= IC_MB else " "
        print(f"{k:62s} q4_0 {spread(a)}  q4_1 {spread(b)}  kq {spread(c)}  x0{x0:5.2f} x1{x1:5.2f} {star}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
