#!/usr/bin/env python3
"""Measurements behind the repetition / presence / frequency penalties; the output is kept as
profiles/penalties_ab.txt.

    python tools/ab_penalties.py [--part a|b|ab] [--rounds 3] [--new 32] [--context 1984] [--streams 1,8,64]
                                 [--routes off,on,host]

(a) The ti_penalty_step launch alone: M streams of V = 32000 logits, each with --context distinct tokens in its
    state.  A captured graph of REP launches (torch.cuda.graph on a side stream whose handle the launches take),
    device events around REPLAYS replays; per launch: median [min .. max] over the rounds.  The launch notes no
    token (null step counter and carry), so every launch rewrites the same entries.
(b) Sampled decoding (T 0.8, top_k 40, top_p 0.9) on the synthetic INT4 Llama-2-7B at max_seq 2048: every stream
    has a prompt of --context distinct tokens and takes --new new tokens.  Routes, alternating within a round:
      off   Engine.generate_sampled, penalties at (1, 0, 0): what the parent commit runs
      on    Engine.generate_sampled under Engine.set_penalties(1.1, 0.4, 0.2)
      host  the route users had: per step Engine.step (logits to the host), penalize_logits over the context so
            far and sample_token, stream by stream; the prompt is prefilled with Engine.score, outside the clock
    Wall clock around the calls (they synchronise), one untimed round first (graph capture).  The device routes
    are timed twice per round, with one new token and with --new, and the decode rate is (new - 1) tokens per
    stream over the difference, so the prompt's prefill is not in it; the host route's clock starts after its
    prefill and stops after --new - 1 steps.  A library without the penalties (TI_LIB, the parent commit's build)
    runs the route `off` alone.
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

REP, REPLAYS = 50, 4
T_, K_, P_ = 0.8, 40, 0.9
PEN = (1.1, 0.4, 0.2)


def spread(v):
    return f"{statistics.median(v):9.2f} [{min(v):8.2f} .. {max(v):8.2f}]"


def part_a(rounds: int, context: int) -> None:
    import numpy as np
    import torch
    import turboinfer_amd as T
    T.init(0)
    L = T.lib()
    dev = torch.device("cuda:0")
    V = MODELS["llama2-7b"][0]
    print(f"(a) ti_penalty_step alone: us per launch, median [min .. max] of {rounds} rounds x {REPLAYS} replays of a "
          f"{REP}-launch graph; V = {V}, {context} distinct tokens per stream")
    for M in (1, 8, 64):
        rng = np.random.default_rng(M)
        logits = torch.randn(M, V, device=dev)
        counts = torch.zeros(M, V, device=dev, dtype=torch.int32)
        seen = torch.zeros(M, V, device=dev, dtype=torch.int32)
        n_seen = torch.zeros(M, device=dev, dtype=torch.int32)
        st = T.PenaltyState(counts.data_ptr(), seen.data_ptr(), n_seen.data_ptr())
        for m in range(M):
            ctx = torch.from_numpy(rng.permutation(V)[:context].astype(np.int32)).to(dev)
            T.check(L.ti_penalty_reset(C.byref(st), V, m, ctx.data_ptr(), context, None))
        torch.cuda.synchronize()
        a = T.PenaltyArgs(logits.data_ptr(), V, M, V, st, PEN[0], PEN[1], PEN[2], 1, 1, None, None, None, 0, None)
        T.check(L.ti_penalty_step(C.byref(a), None))       # once outside a graph: errors surface here
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for _ in range(REP):
                T.check(L.ti_penalty_step(C.byref(a), s))
        times = []
        for rnd in range(rounds + 1):                      # round 0 untimed
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPLAYS):
                g.replay()
            e1.record()
            e1.synchronize()
            if rnd:
                times.append(e0.elapsed_time(e1) * 1e3 / (REP * REPLAYS))
        print(f"  M = {M:2d}: {spread(times)} us per launch ({int(n_seen.max())} entries walked per stream)")
        sys.stdout.flush()
        del g


def part_b(rounds: int, n_new: int, context: int, streams_list, routes_want) -> None:
    import numpy as np
    import turboinfer_amd as T
    T.init(0)
    has = hasattr(T.lib(), "ti_engine_set_penalties")
    V, H, layers, nh, nkv, hd, I, bits, theta = MODELS["llama2-7b"]
    print(f"(b) sampled decoding (T {T_}, top_k {K_}, top_p {P_}): synthetic INT4 llama2-7b, max_seq 2048, prompts of {context} "
          f"distinct tokens, {n_new} new tokens per stream; decode tok/s over all streams, median [min .. max] of {rounds} "
          f"alternating rounds; library {'with' if has else 'WITHOUT'} the penalties ({os.path.basename(T.LIB_PATH)})")
    for streams in streams_list:
        e = T.Engine(V, H, layers, nh, nkv, hd, I, bits=bits, max_seq=2048, max_batch=streams, rope_theta=theta)
        e.synth(0x7157, 0.0)
        rng = np.random.default_rng(7 + streams)
        prompts = [(3 + rng.permutation(V - 3)[:context]).tolist() for _ in range(streams)]
        draws = rng.uniform(0, 1, (streams, n_new)).astype(np.float32)

        def device(pen):
            def run():
                if has:
                    e.set_penalties(*pen)
                # (a change of penalties drops the step graphs: one step outside the clock captures this route's)
                e.generate_sampled([[5]] * streams, 1, T_, K_, P_, draws[:, :1])
                t0 = time.perf_counter()
                e.generate_sampled(prompts, 1, T_, K_, P_, draws[:, :1])
                t1 = time.perf_counter()
                toks, _ = e.generate_sampled(prompts, n_new, T_, K_, P_, draws)
                t2 = time.perf_counter()
                return (t2 - t1) - (t1 - t0), toks
            return run

        def host():
            if has:
                e.set_penalties()
            for m, p in enumerate(prompts):                # the prompt's KV rows, outside the clock
                e.score(p[:-1], stream=m)
            ctx = [list(p) for p in prompts]
            tok = [p[-1] for p in prompts]
            out = np.zeros((streams, n_new), np.int32)
            t0 = 0.0
            for s in range(n_new):
                if s == 1:                                 # (as the device routes: the first token is not in the rate)
                    t0 = time.perf_counter()
                lg = e.step(tok, [context - 1 + s] * streams)
                for m in range(streams):
                    pl = T.penalize_logits(lg[m], ctx[m], *PEN)
                    tok[m], _ = T.sample_token(pl, T_, K_, P_, float(draws[m, s]))
                    ctx[m].append(tok[m])
                    out[m, s] = tok[m]
            return time.perf_counter() - t0, out
        routes = {"off": device((1.0, 0.0, 0.0)), "on": device(PEN), "host": host}
        routes = {k: v for k, v in routes.items() if k in routes_want and (has or k == "off")}
        res = {rn: [] for rn in routes}
        toks = {}
        for rnd in range(rounds + 1):                      # round 0 untimed (graph capture)
            for rn, fn in routes.items():
                dt, toks[rn] = fn()
                if rnd:
                    res[rn].append(streams * (n_new - 1) / dt)
        for rn in routes:
            note = ""
            if rn == "host" and "on" in toks:
                same = int((toks["host"] == toks["on"]).all(axis=1).sum())
                note = f"   streams whose tokens equal the route on's: {same} / {streams}"
            if rn == "on" and "off" in toks:
                note = f"   x{statistics.median(res['on']) / statistics.median(res['off']):.3f} of off"
            print(f"  {streams:2d} streams  {rn:5s} {spread(res[rn])} tok/s{note}")
        sys.stdout.flush()
        e.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=("a", "b", "ab"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--context", type=int, default=1984)
    ap.add_argument("--streams", default="1,8,64")
    ap.add_argument("--routes", default="off,on,host")
    args = ap.parse_args()
    if "a" in args.part:
        part_a(args.rounds, args.context)
    if "b" in args.part:
        part_b(args.rounds, args.new, args.context, [int(s) for s in args.streams.split(",")], args.routes.split(","))
    return 0


if __name__ == "__main__":
    sys.exit(main())
