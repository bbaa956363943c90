#!/usr/bin/env python3
"""Measurements behind lookahead greedy decoding; the output is kept as profiles/lookahead_ab.txt.

    python tools/ab_lookahead.py [--part a|b|ab] [--rounds 5] [--new 128]

(a) The attention launch of a verify step alone: a chunk of M rows at the end of a prefix of `keys` keys,
    ti_attn_prefill_split at several split counts against the two routes a prompt chunk had before,
    ti_attn_prefill and ti_attn_decode at stream stride 0.  Each route is a captured graph of REP launches
    (torch.cuda.graph on a side stream whose handle the launches take); the routes alternate A B C .. A B C ..
    in this one process, device events around REPLAYS replays; per launch: median [min .. max] over the rounds.
(b) A whole request on the synthetic INT4 Llama-2-7B: context 2048 (fill_kv), --new tokens; Engine.generate
    against Engine.generate_lookahead at k = 3, 7, 15, once with corpus = the plain run's own tokens (every
    draft right: the ceiling) and once with a corpus of tokens the text never contains (no draft ever proposed
    or accepted: what a verify step costs).  Wall clock around the call (it synchronises), the runs alternate,
    one untimed call of each first (graph capture); ms per step, tokens per step, tok/s.
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


def spread(v):
    return f"{statistics.median(v):8.2f} [{min(v):7.2f} .. {max(v):7.2f}]"


def part_a(rounds: int) -> None:
    import torch
    import turboinfer_amd as T
    T.init(0)
    L = T.lib()
    dev = torch.device("cuda:0")
    print(f"(a) attention launch alone: us per launch, median [min .. max] of {rounds} rounds x {REPLAYS} replays of a "
          f"{REP}-launch graph, routes alternating")
    shapes = [("llama2-7b shape (32 / 32 heads, hd 128)", 32, 32, 128, 2048),
              ("llama3-8b shape (32 / 8 heads, hd 128)", 32, 8, 128, 8192)]
    for name, heads, kvh, hd, keys in shapes:
        torch.manual_seed(keys)
        kc = (0.5 * torch.randn(kvh, keys, hd, device=dev)).half()
        vc = torch.randn(kvh, keys, hd, device=dev).half()
        for M in (8, 16):
            q = torch.randn(M, heads * hd, device=dev)
            pos = torch.arange(keys - M, keys, device=dev, dtype=torch.int32)
            out = torch.zeros(M, heads * hd, device=dev, dtype=torch.float16)
            ws_s = torch.zeros(L.ti_attn_prefill_split_workspace_bytes(16, heads, hd, 32) // 4, device=dev)
            dsp = max(1, min((256 + kvh * M - 1) // (kvh * M), keys // 64, 64))      # the engine's splits_for(M)
            ws_d = torch.zeros(max(L.ti_attn_workspace_bytes(M, heads, hd, dsp) // 4, 4), device=dev)
            a = (q.data_ptr(), kc.data_ptr(), vc.data_ptr())

            def split(S):
                return lambda s: L.ti_attn_prefill_split(*a, keys, pos.data_ptr(), M, heads, kvh, hd, S, ws_s.data_ptr(),
                                                         out.data_ptr(), s)
            routes = {f"ti_attn_prefill_split S={S}": split(S) for S in (4, 8, 16, 32)}
            routes["ti_attn_prefill"] = lambda s: L.ti_attn_prefill(*a, keys, pos.data_ptr(), M, heads, kvh, hd,
                                                                    out.data_ptr(), s)
            routes[f"ti_attn_decode stride 0, {dsp} splits"] = lambda s: L.ti_attn_decode(
                *a, 0, keys, pos.data_ptr(), M, heads, kvh, hd, dsp, ws_d.data_ptr(), out.data_ptr(), s)
            graphs, outs = {}, {}
            for rn, fn in routes.items():
                T.check(fn(None))                      # once outside a graph: errors surface here
                torch.cuda.synchronize()
                outs[rn] = out.float().clone()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                    for _ in range(REP):
                        T.check(fn(s))
                graphs[rn] = g
            ref = outs["ti_attn_prefill"]
            times = {rn: [] for rn in routes}
            for rnd in range(rounds + 1):              # round 0 untimed
                for rn, g in graphs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(REPLAYS):
                        g.replay()
                    e1.record()
                    e1.synchronize()
                    if rnd:
                        times[rn].append(e0.elapsed_time(e1) * 1e3 / (REP * REPLAYS))
            print(f"  {name}, M = {M}, {keys} keys")
            for rn in routes:
                dmax = float((outs[rn] - ref).abs().max())
                print(f"    {rn:40s} {spread(times[rn])} us   max |out - ti_attn_prefill's| {dmax:.2e}")
            sys.stdout.flush()


def part_b(rounds: int, n_new: int) -> None:
    import numpy as np
    import turboinfer_amd as T
    T.init(0)
    V, H, layers, nh, nkv, hd, I, bits, theta = MODELS["llama2-7b"]
    ctx = 2048
    e = T.Engine(V, H, layers, nh, nkv, hd, I, bits=bits, max_seq=ctx + n_new + 32, max_batch=1, rope_theta=theta)
    e.synth(0x7157, 0.0)
    e.fill_kv(0, ctx, 0x7157)
    print(f"(b) whole request: synthetic INT4 llama2-7b, context {ctx}, {n_new} new tokens; wall clock of the call, "
          f"median [min .. max] of {rounds} alternating rounds")
    prompt = [0x7157 % V]
    plain = e.generate([prompt], n_new, start_pos=[ctx])[0].tolist()
    runs = {"generate": None}
    for k in (3, 7, 15):
        # the request's own greedy tokens through the verify step's kernels (no corpus).  The synthetic model's
        # logits are those of random weights: where its top two are closer than the rounding difference between
        # the one-row and the k + 1-row kernels the two routes part ways, so the ceiling's corpus is this text
        own = e.generate_lookahead(prompt, n_new, k=k, ngram=3, start_pos=ctx)[0].tolist()
        used = set(own) | set(plain) | set(prompt)
        unrelated = [t for t in range(1000, 1000 + 8 * n_new) if t not in used][:2 * n_new]
        runs[f"lookahead k={k:2d} true corpus"] = (k, own)
        runs[f"lookahead k={k:2d} unrelated corpus"] = (k, unrelated)
        same = next((i for i, (a, b) in enumerate(zip(own, plain)) if a != b), n_new)
        note = f"  k={k:2d} without corpus: first {same} of {n_new} tokens equal generate's"
        if same < n_new:
            lg = e.generate([prompt], same + 1, start_pos=[ctx], want_logits=True)[1][0]
            top = np.sort(lg)[-2:]
            note += (f"; at token {same} generate's top-2 logits differ by {top[1] - top[0]:.3g} = "
                     f"{(top[1] - top[0]) / np.max(np.abs(lg)):.2g} of max|logit| (the project's logits bar: 2e-3), "
                     f"second choice {int(np.argsort(lg)[-2])}, the verify step chose {own[same]}")
        print(note, flush=True)
    res = {rn: [] for rn in runs}
    stats = {}
    for rnd in range(rounds + 1):                      # round 0 untimed (graph capture)
        for rn, spec in runs.items():
            t0 = time.perf_counter()
            if spec is None:
                toks = e.generate([prompt], n_new, start_pos=[ctx])[0].tolist()
                st = dict(steps=n_new, drafted=0, accepted=0, produced=n_new)
            else:
                toks, st = e.generate_lookahead(prompt, n_new, k=spec[0], ngram=3, corpus=spec[1], start_pos=ctx)
                toks = toks.tolist()
            dt = time.perf_counter() - t0
            want = plain if spec is None else runs[f"lookahead k={spec[0]:2d} true corpus"][1]
            stats[rn] = (st, sum(a == b for a, b in zip(toks, want)))
            if rnd:
                res[rn].append(dt)
    base =statistics.median(res["generate"]) / n_new
    for rn in runs:
        st, same = stats[rn]
        ms = [t * 1e3 / st["steps"] for t in res[rn]]
        tps = [st["produced"] / t for t in res[rn]]
        print(f"  {rn:34s} steps {st['steps']:4d} drafted {st['drafted']:5d} accepted {st['accepted']:4d} "
              f"tokens/step {st['produced'] / st['steps']:5.2f}  ms/step {spread(ms)}  tok/s {spread(tps)}  "
              f"tokens equal to the route's own greedy text: {same} / {n_new}")
    for k in (3, 7, 15):
        st, _ = stats[f"lookahead k={k:2d} unrelated corpus"]
        step = statistics.median(res[f"lookahead k={k:2d} unrelated corpus"]) / st["steps"]
        ceil = stats[f"lookahead k={k:2d} true corpus"][0]
        print(f"  k={k:2d}: a verify step of the unrelated-corpus run ({st['accepted']} drafts accepted in {st['steps']} "
              f"steps) costs {step / base:.2f} plain steps ({step * 1e3:.3f} ms against {base * 1e3:.3f} ms, the "
              f"request's prompt and read-backs included): break-even at {step / base:.2f} tokens per step; the true "
              f"corpus gave {ceil['produced'] / ceil['steps']:.2f}")
    e.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=("a", "b", "ab"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--new", type=int, default=128)
    args = ap.parse_args()
    if "a" in args.part:
        part_a(args.rounds)
    if "b" in args.part:
        part_b(args.rounds, args.new)
    return 0


if __name__ == "__main__":
    sys.exit(main())
