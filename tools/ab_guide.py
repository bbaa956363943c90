#!/usr/bin/env python3
"""Measurements behind token-automaton guided decoding; the output is kept as profiles/guide_ab.txt.

    python tools/ab_guide.py [--part a|b|c|abc] [--rounds 3] [--new 32] [--context 1984] [--streams 1,8,64]
                             [--routes off,on,host]

The guide is a 64-state cycle over V = 32000: state i allows the ids = i (mod 64), 500 of them, and moves to
state i + 1 (mod 64).
(a) The ti_guide_step launch alone: M streams of V logits, stream m in state m (mod 64).  A captured graph of REP
    launches (torch.cuda.graph on a side stream whose handle the launches take), device events around REPLAYS
    replays; per launch: median [min .. max] over the rounds.  The launch consumes no token (null step counter
    and carry), so every launch masks with the same state; after the first the row already holds the -inf it
    writes, which changes no access.
(b) Sampled decoding (T 0.8, top_k 40, top_p 0.9) on the synthetic INT4 Llama-2-7B at max_seq 2048: every stream
    has a prompt of --context tokens and takes --new new tokens.  Routes, alternating within a round:
      off   Engine.generate_sampled, no guide: what the parent commit runs
      on    Engine.generate_sampled under Engine.set_guide(the cycle)
      host  the route users had: per step Engine.step (logits to the host), guide_apply and sample_token, stream
            by stream; the prompt is prefilled with Engine.score, outside the clock
    Wall clock around the calls (they synchronise), one untimed round first (graph capture).  The device routes
    are timed twice per round, with one new token and with --new, and the decode rate is (new - 1) tokens per
    stream over the difference, so the prompt's prefill is not in it; the host route's clock starts after its
    prefill and stops after --new - 1 steps.  A library without the guides (TI_LIB, the parent commit's build)
    runs the route `off` alone.
(c) Where the one-stream step's time goes: Engine.stamp_steps with and without the guide is not comparable (the
    stamped graph is the unsampled step), so this part prints the launch count of the unsampled step graph with
    no guide set -- it must equal the parent's -- and leaves the sampled step's split to a profiler run.
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
STATES = 64


def spread(v):
    return f"{statistics.median(v):9.2f} [{min(v):8.2f} .. {max(v):8.2f}]"


def cycle(V, n=STATES):
    """-> (row_ptr, tokens, next): state i allows the ids = i (mod n) and moves to i + 1 (mod n)."""
    import numpy as np
    rows = [np.arange(i, V, n, dtype=np.int32) for i in range(n)]
    row_ptr = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int64)
    nxt = np.concatenate([np.full(r.size, (i + 1) % n, np.int32) for i, r in enumerate(rows)])
    return row_ptr, np.concatenate(rows), nxt


def part_a(rounds: int) -> None:
    import numpy as np
    import torch
    import turboinfer_amd as T
    T.init(0)
    L = T.lib()
    dev = torch.device("cuda:0")
    V = MODELS["llama2-7b"][0]
    W = (V + 31) // 32
    row_ptr, tokens, nxt = cycle(V)
    mask = np.zeros((STATES, W), np.uint32)
    for s in range(STATES):
        a = tokens[row_ptr[s]: row_ptr[s + 1]].astype(np.int64)
        np.bitwise_or.at(mask[s], a >> 5, np.uint32(1) << (a & 31).astype(np.uint32))
    d = [torch.from_numpy(x).to(dev) for x in (row_ptr, tokens, nxt, mask.view(np.int32))]
    gd = T.GuideDev(STATES, W, *(x.data_ptr() for x in d))
    print(f"(a) ti_guide_step alone: us per launch, median [min .. max] of {rounds} rounds x {REPLAYS} replays of a "
          f"{REP}-launch graph; V = {V}, {STATES}-state cycle ({V // STATES} allowed ids per state)")
    for M in (1, 8, 64):
        logits = torch.randn(M, V, device=dev)
        state = (torch.arange(M, device=dev, dtype=torch.int32) % STATES).contiguous()
        a = T.GuideArgs(logits.data_ptr(), V, M, V, gd, state.data_ptr(), 1, 1, None, None, None, 0, None)
        T.check(L.ti_guide_step(C.byref(a), None))         # once outside a graph: errors surface here
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for _ in range(REP):
                T.check(L.ti_guide_step(C.byref(a), s))
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
        print(f"  M = {M:2d}: {spread(times)} us per launch ({int(torch.isinf(logits).sum()) // M} of {V} columns at -inf per row)")
        sys.stdout.flush()
        del g


def part_b(rounds: int, n_new: int, context: int, streams_list, routes_want) -> None:
    import numpy as np
    import turboinfer_amd as T
    T.init(0)
    has = hasattr(T.lib(), "ti_engine_set_guide")
    V, H, layers, nh, nkv, hd, I, bits, theta = MODELS["llama2-7b"]
    guide = cycle(V)
    print(f"(b) sampled decoding (T {T_}, top_k {K_}, top_p {P_}): synthetic INT4 llama2-7b, max_seq 2048, prompts of {context} "
          f"tokens, {n_new} new tokens per stream; decode tok/s over all streams, median [min .. max] of {rounds} "
          f"alternating rounds; library {'with' if has else 'WITHOUT'} the guides ({os.path.basename(T.LIB_PATH)})")
    for streams in streams_list:
        e = T.Engine(V, H, layers, nh, nkv, hd, I, bits=bits, max_seq=2048, max_batch=streams, rope_theta=theta)
        e.synth(0x7157, 0.0)
        rng = np.random.default_rng(7 + streams)
        prompts = [(3 + rng.permutation(V - 3)[:context]).tolist() for _ in range(streams)]
        draws = rng.uniform(1e-6, 1, (streams, n_new)).astype(np.float32)

        def device(on):
            def run():
                if has:
                    e.set_guide(*guide) if on else e.set_guide(None)
                # (a change of guide drops the step graphs: one step outside the clock captures this route's)
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
                e.set_guide(None)
            for m, p in enumerate(prompts):                # the prompt's KV rows, outside the clock
                e.score(p[:-1], stream=m)
            tok = [p[-1] for p in prompts]
            state = [0] * streams
            out = np.zeros((streams, n_new), np.int32)
            t0 = 0.0
            for s in range(n_new):
                if s == 1:                                 # (as the device routes: the first token is not in the rate)
                    t0 = time.perf_counter()
                lg = e.step(tok, [context - 1 + s] * streams)
                for m in range(streams):
                    state[m], pl = T.guide_apply(guide, state[m], tok[m] if s else -1, lg[m])
                    tok[m], _ = T.sample_token(pl, T_, K_, P_, float(draws[m, s]))
                    out[m, s] = tok[m]
            return time.perf_counter() - t0, out
        routes = {"off": device(False), "on": device(True), "host": host}
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
            if rn == "on":
                ok = bool(((toks["on"] % STATES) == (np.arange(n_new) % STATES)).all())
                note = f"   every token accepted: {ok}"
                if "off" in toks:
                    note = f"   x{statistics.median(res['on']) / statistics.median(res['off']):.3f} of off" + note
            print(f"  {streams:2d} streams  {rn:5s} {spread(res[rn])} tok/s{note}")
        sys.stdout.flush()
        e.close()


def part_c() -> None:
    import turboinfer_amd as T
    T.init(0)
    V, H, layers, nh, nkv, hd, I, bits, theta = MODELS["llama2-7b"]
    for streams in (1, 64):
        e = T.Engine(V, H, layers, nh, nkv, hd, I, bits=bits, max_seq=2048, max_batch=streams, rope_theta=theta)
        e.synth(0x7157, 0.0)
        e.replay_prepare(streams, 2048, 1)
        print(f"(c) no guide set, {streams} streams: {len(e.stamp_steps(steps=4))} launches in the stamped step graph")
        e.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="abc")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--context", type=int, default=1984)
    ap.add_argument("--streams", default="1,8,64")
    ap.add_argument("--routes", default="off,on,host")
    args = ap.parse_args()
    if "a" in args.part:
        part_a(args.rounds)
    if "b" in args.part:
        part_b(args.rounds, args.new, args.context, [int(s) for s in args.streams.split(",")], args.routes.split(","))
    if "c" in args.part:
        part_c()
    return 0


if __name__ == "__main__":
    sys.exit(main())
