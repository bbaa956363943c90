#!/usr/bin/env python3
"""Decode step throughput of the replay step (the bench's timed region) with whatever library TI_LIB
names -- old builds included (only the round-1 engine API is used): A/B runs interleave builds.

    TI_LIB=... python tools/ab_step.py [--model llama2-7b] [--batch 1] [--steps 256] [--kv-bits 16|8]

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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama2-7b", choices=sorted(MODELS))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--kv", type=int, default=0)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--tag", default="")
    ap.add_argument("--kv-bits", type=int, default=16, choices=(16, 8))
    ap.add_argument("--attn", action="store_true", help="also time the attention launch alone")
    args = ap.parse_args()
    print(run(args.model, args.batch, args.kv, args.steps, args.kv_bits, args.attn, args.tag))
    return 0


if __name__ == "__main__":
    sys.exit(main())
