#!/usr/bin/env python3
"""Decode step throughput of the replay step (the bench's timed region) with whatever library TI_LIB
names -- old builds included (only the round-1 engine API is used): A/B runs interleave builds.

    TI_LIB=... python tools/ab_step.py [--model llama2-7b] [--batch 1] [--steps 256] [--kv-bits 16|8]
    TI_LIB=... python tools/ab_step.py --prompt 512 [--model llama2-7b] [--kv-bits 16|8] [--rounds 2]

--prompt N: the time from an N-token prompt to the first token instead (Engine.generate(.., 1), best of 3);
with --rounds R > 1 and no --kv-bits the fp16 and e4m3 caches alternate A B A B in this one process.

--kv-bits 8 runs the engine with the e4m3 KV cache (BITS_KV8); --attn adds the attention launch
alone (ti_engine_time_kernel which = 5) with its bytes and its fraction of the same run's HBM read rate."""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import MODELS  # noqa: E402


def run(model: str, batch: int = 1, kv: int = 0, steps: int = 256, kv_bits: int = 16, attn: bool = False,
        tag: str = "") -> str:
    """One replay measurement -> its result line (callers may interleave formats in one process: A B A B)."""
    import turboinfer_amd as T
    T.init(0)
    V, H, layers, nh, nkv, hd, I, bits, theta = MODELS[model]
    B = batch
    L = kv or (8192 if model == "llama3-8b" else 2048)
    if kv_bits == 8:
        bits |= T.BITS_KV8
    e = T.Engine(V, H, layers, nh, nkv, hd, I, bits=bits, max_seq=L, max_batch=B, rope_theta=theta)
    e.synth(0x7157, 0.0)
    for s in range(B):
        e.fill_kv(s, L - 1, 0x7157 + s)
    e.replay_prepare(B, L, 0x7157 % V)
    e.replay_run(16)
    e.sync()
    t0 = time.perf_counter()
    e.replay_run(steps)
    e.sync()
    dt = time.perf_counter() - t0
    line = f"{tag} {model} B={B} L={L} kv{kv_bits}: {B * steps / dt:.1f} tok/s, {dt / steps * 1e6:.1f} us/step"
    if attn:
        us, by = e.time_kernel(5, B, L, 8)
        read_gbps, _ = T.hbm_calibrate()
        line += (f"; attention {us:.1f} us, {by / 1e6:.1f} MB, {by / us / 1e3:.0f} GB/s = "
                 f"{by / us / 1e3 / read_gbps:.2f} of the HBM read rate ({read_gbps:.0f} GB/s)")
    e.close()
    return line


def prompt(model: str, n: int, kv_bits: int = 16, tag: str = "") -> str:
    """The time from an n-token prompt to the first token (generate(.., 1): prefill chunks, then the lm_head on
    the last row), best of 3 after one untimed run -> its result line."""
    import numpy as np
    import turboinfer_amd as T
    T.init(0)
    V, H, layers, nh, nkv, hd, I, bits, theta = MODELS[model]
    if kv_bits == 8:
        bits |= T.BITS_KV8
    e = T.Engine(V, H, layers, nh, nkv, hd, I, bits=bits, max_seq=max(2048, n + 16), max_batch=1, rope_theta=theta)
    e.synth(0x7157, 0.0)
    toks = np.random.RandomState(1).randint(0, V, size=n).tolist()
    e.generate([toks], 1)
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        e.generate([toks], 1)
        best = min(best, time.perf_counter() - t0)
    route = e.prefill_attn_name(n) if hasattr(e, "prefill_attn_name") and hasattr(T.lib(), "ti_engine_prefill_attn_name") else "?"
    e.close()
    return f"{tag} {model} {n}-token prompt to first token kv{kv_bits}: {best * 1e3:.2f} ms (best of 3; a chunk of {n} rows: {route})"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama2-7b", choices=sorted(MODELS))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--kv", type=int, default=0)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--tag", default="")
    ap.add_argument("--kv-bits", type=int, default=None, choices=(16, 8))
    ap.add_argument("--prompt", type=int, default=0, help="time an N-token prompt to the first token instead")
    ap.add_argument("--rounds", type=int, default=1, help="--prompt: repeats (kv16 kv8 kv16 kv8 .. without --kv-bits)")
    ap.add_argument("--attn", action="store_true", help="also time the attention launch alone")
    args = ap.parse_args()
    if args.prompt:
        for r in range(args.rounds):
            for kvb in ([args.kv_bits] if args.kv_bits else [16, 8]):
                print(prompt(args.model, args.prompt, kvb, f"{args.tag}run{r}"), flush=True)
        return 0
    args.kv_bits = args.kv_bits or 16
    print(run(args.model, args.batch, args.kv, args.steps, args.kv_bits, args.attn, args.tag))
    return 0


if __name__ == "__main__":
    sys.exit(main())
