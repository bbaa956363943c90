#!/usr/bin/env python3
"""Measurements behind the shared prompt prefix; the output is kept as profiles/shared_prefix_ab.txt.

    python tools/ab_shared_prefix.py [--part a|b|ab] [--rounds 5] [--new 128] [--streams 64] [--prefix 1920]

(a) The attention launch of a batched decode step alone: M streams, each with a prefix of P keys that all streams
    share and 128 keys of its own, ti_attn_decode (the engine's split count for M) against ti_attn_decode_shared
    at several split counts.  Each route is a captured graph of REP calls (torch.cuda.graph on a side stream whose
    handle the launches take); the routes alternate A B C .. A B C .. in this one process, device events around
    REPLAYS replays; per call (both launches of the shared route): median [min .. max] over the rounds.
(b) A whole batch on the synthetic INT4 Llama-2-7B: --streams requests of --prefix common tokens plus one own
    token, --new new tokens each.  Unregistered: Engine.generate of the full prompts (every request prefills the
    prefix).  Registered: Engine.share_prefix, then Engine.generate of the continuations at start_pos = prefix --
    cold (the registration made inside the timed window) and warm (already live).  Wall clock around the calls
    (they synchronise), the routes alternate, one untimed pass first (graph capture); the time to the first
    token is the same call with one new token.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import MODELS  # noqa: E402

REP, REPLAYS, OWN = 20, 4, 128


def spread(v):
    return f"{statistics.median(v):8.2f} [{min(v):7.2f} .. {max(v):7.2f}]"


def part_a(rounds: int) -> None:
    import torch
    import turboinfer_amd as T
    T.init(0)
    L = T.lib()
    dev = torch.device("cuda:0")
    print(f"(a) attention of one batched step alone: us per call, median [min .. max] of {rounds} rounds x {REPLAYS} "
          f"replays of a {REP}-call graph, routes alternating; P shared keys + {OWN} own keys per stream")
    shapes = [("llama2-7b shape (32 / 32 heads, hd 128)", 32, 32, 128),
              ("llama3-8b shape (32 / 8 heads, hd 128)", 32, 8, 128)]
    prefixes = (64, 256, 1024, 1920)
    max_seq = max(prefixes) + OWN
    for name, heads, kvh, hd in shapes:
        G = heads // kvh
        for M in (8, 64):
            torch.manual_seed(M)
            kc = torch.randn(M, kvh, max_seq, hd, device=dev, dtype=torch.float16) * 0.5
            vc = torch.randn(M, kvh, max_seq, hd, device=dev, dtype=torch.float16)
            q = torch.randn(M, heads * hd, device=dev)
            out = torch.zeros(M, heads * hd, device=dev, dtype=torch.float16)
            stride = kvh * max_seq * hd
            for P in prefixes:
                kc[1:, :, :P] = kc[0, :, :P]           # every stream's copy of the prefix, as fork_slot leaves it
                vc[1:, :, :P] = vc[0, :, :P]
                pos = torch.full((M,), P + OWN - 1, device=dev, dtype=torch.int32)
                dsp = max(1, min((256 + kvh * M - 1) // (kvh * M), max_seq // 64, 64))      # the engine's splits_for(M)
                ws_d = torch.zeros(max(L.ti_attn_workspace_bytes(M, heads, hd, dsp) // 4, 4), device=dev)
                ws_s = torch.empty(L.ti_attn_shared_workspace_bytes(M, heads, hd, 32) // 4, device=dev)
                a = (q.data_ptr(), kc.data_ptr(), vc.data_ptr(), stride, max_seq, pos.data_ptr(), M, heads, kvh, hd)
                blocks = (M * G + 15) // 16 * kvh

                def shared(S):
                    return lambda s: L.ti_attn_decode_shared(*a, P, S, 0, ws_s.data_ptr(), out.data_ptr(), s)
                routes = {f"ti_attn_decode, {dsp} splits": lambda s: L.ti_attn_decode(*a, dsp, ws_d.data_ptr(),
                                                                                      out.data_ptr(), s)}
                for S in (1, 2, 4, 8, 16, 32):
                    if S <= (P + 15) // 16:
                        routes[f"ti_attn_decode_shared S={S} ({blocks * S} waves)"] = shared(S)
                graphs, outs = {}, {}
                for rn, fn in routes.items():
                    T.check(fn(None))                  # once outside a graph: errors surface here
                    torch.cuda.synchronize()
                    outs[rn] = out.float().clone()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                        for _ in range(REP):
                            T.check(fn(s))
                    graphs[rn] = g
                ref = outs[next(iter(routes))]
                times = {rn: [] for rn in routes}
                for rnd in range(rounds + 1):          # round 0 untimed
                    for rn, g in graphs.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(REPLAYS):
                            g.replay()
                        e1.record()
                        e1.synchronize()
                        if rnd:
                            times[rn].append(e0.elapsed_time(e1) * 1e3 / (REP * REPLAYS))
                # K + V bytes the byte model gives each route, per kv-head row of hd fp16
                plain_b = M * (P + OWN) * kvh * hd * 4
                shared_b = ((M * G + 15) // 16 * P + M * OWN) * kvh * hd * 4
                print(f"  {name}, M = {M}, P = {P}: K/V bytes plain {plain_b / 1e6:.1f} MB, shared {shared_b / 1e6:.1f} MB")
                base = statistics.median(times[next(iter(routes))])
                for rn in routes:
                    dmax = float((outs[rn] - ref).abs().max())
                    print(f"    {rn:46s} {spread(times[rn])} us   x{base / statistics.median(times[rn]):5.2f}   "
                          f"max |out - ti_attn_decode's| {dmax:.2e}")
                sys.stdout.flush()
                del graphs
            del kc, vc


def part_b(rounds: int, n_new: int, streams: int, prefix_len: int) -> None:
    import numpy as np
    import turboinfer_amd as T
    T.init(0)
    V, H, layers, nh, nkv, hd, I, bits, theta = MODELS["llama2-7b"]
    e = T.Engine(V, H, layers, nh, nkv, hd, I, bits=bits, max_seq=prefix_len + 1 + n_new, max_batch=streams, rope_theta=theta)
    e.synth(0x7157, 0.0)
    rng = np.random.default_rng(7)
    prefix = rng.integers(3, V, prefix_len).tolist()
    own = [[int(t)] for t in rng.integers(3, V, streams)]
    full = [prefix + o for o in own]
    print(f"(b) whole batch: synthetic INT4 llama2-7b, {streams} streams, {prefix_len} common prompt tokens + 1 own, {n_new} "
          f"new tokens each; wall clock of the calls, median [min .. max] of {rounds} alternating rounds "
          f"(TI_SHARE_MIN {os.environ.get('TI_SHARE_MIN', 'default')}, TI_SHARE_SPLITS {os.environ.get('TI_SHARE_SPLITS', 'default')})")

    def unregistered(new):
        e.share_prefix([], streams)
        return e.generate(full, new)

    def cold(new):
        e.share_prefix([], streams)
        e.share_prefix(prefix, streams)
        return e.generate(own, new, start_pos=[prefix_len] * streams)

    def warm(new):
        e.share_prefix(prefix, streams)                 # live after the first call: returns at once
        return e.generate(own, new, start_pos=[prefix_len] * streams)
    routes = {"unregistered (full prompts)": unregistered, "registered, cold": cold, "registered, warm": warm}
    res = {(rn, k): [] for rn in routes for k in ("all", "first")}
    toks = {}
    for rnd in range(rounds + 1):                      # round 0 untimed (graph capture)
        for rn, fn in routes.items():
            for k, new in (("first", 1), ("all", n_new)):
                t0 = time.perf_counter()
                got = fn(new)
                dt = time.perf_counter() - t0
                if k == "all":
                    toks[rn] = got
                if rnd:
                    res[(rn, k)].append(dt)
    base = toks["unregistered (full prompts)"]
    for rn in routes:
        same = int((toks[rn] == base).all(axis=1).sum())
        tps = [streams * n_new / t for t in res[(rn, "all")]]
        print(f"  {rn:30s} total {spread([t * 1e3 for t in res[(rn, 'all')]])} ms   tok/s {spread(tps)}   "
              f"first token after {spread([t * 1e3 for t in res[(rn, 'first')]])} ms   "
              f"streams whose {n_new} tokens equal the unregistered run's: {same} / {streams}")
    # the decode steps alone: the two totals minus their first-token calls
    for rn in routes:
        d = statistics.median(res[(rn, "all")]) - statistics.median(res[(rn, "first")])
        print(f"  {rn:30s} after the first token: {d * 1e3 / max(n_new - 1, 1):8.3f} ms per step of {streams} streams")
    e.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=("a", "b", "ab"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--prefix", type=int, default=1920)
    args = ap.parse_args()
    if "a" in args.part:
        part_a(args.rounds)
    if "b" in args.part:
        part_b(args.rounds, args.new, args.streams, args.prefix)
    return 0


if __name__ == "__main__":
    sys.exit(main())
