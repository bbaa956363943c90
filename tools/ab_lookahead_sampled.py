#!/usr/bin/env python3
"""Measurements behind sampled lookahead decoding; the output is kept in profiles/sampled_loops_ab.txt.

    python tools/ab_lookahead_sampled.py [--rounds 5] [--new 128]

A whole request on the synthetic INT4 Llama-2-7B: context 2048 (fill_kv), --new tokens, top_k 50, top_p 0.9,
temperature 1.0, one set of seeded draws for every route.  Engine.generate_sampled against
Engine.generate_lookahead_sampled at k = 3, 7, 15, once with corpus = that route's own output (every draft right:
the ceiling) and once with a corpus of tokens the text never contains (no draft proposed: what a verify step
costs).  The greedy Engine.generate_lookahead with the unrelated corpus runs in the same rounds: its verify step
is the sampled one without the ti_lookahead_sample launch, so the difference of the two ms/step is that launch's
share.  Wall clock around the call (it synchronises), the runs alternate A B C .. A B C .. in this one process,
one untimed call of each first (graph capture); median [min .. max] over the rounds.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import MODELS  # noqa: E402

T_, TOP_K, TOP_P = 1.0, 50, 0.9


def spread(v):
    return f"{statistics.median(v):8.3f} [{min(v):7.3f} .. {max(v):7.3f}]"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--new", type=int, default=128)
    args = ap.parse_args()
    import numpy as np
    import turboinfer_amd as T
    T.init(0)
    n_new, rounds = args.new, args.rounds
    V, H, layers, nh, nkv, hd, I, bits, theta = MODELS["llama2-7b"]
    ctx = 2048
    e = T.Engine(V, H, layers, nh, nkv, hd, I, bits=bits, max_seq=ctx + n_new + 32, max_batch=1, rope_theta=theta)
    e.synth(0x7157, 0.0)
    e.fill_kv(0, ctx, 0x7157)
    draws = np.random.RandomState(0x7157).uniform(0, 1, n_new).astype(np.float32)
    prompt = [0x7157 % V]
    print(f"sampled lookahead: synthetic INT4 llama2-7b, context {ctx}, {n_new} new tokens, T {T_} top_k {TOP_K} "
          f"top_p {TOP_P}; wall clock of the call, median [min .. max] of {rounds} alternating rounds")
    plain = e.generate_sampled([prompt], n_new, T_, TOP_K, TOP_P, draws, start_pos=[ctx])[0][0].tolist()
    runs = {"generate_sampled": None}
    for k in (3, 7, 15):
        # the route's own output as corpus.  With a corpus a token is computed by another row of another step than
        # without one; the two differ at most by rounding, but the 50 survivors of a random-weight model are nearly
        # equal, so now and then that swaps the 50th survivor or moves a draw across a boundary, and the output
        # with a corpus leaves the corpus (measured: at token 39).  So the corpus is fed back until the output
        # repeats it (a fixed point: every draft right), at most 8 passes.
        own = e.generate_lookahead_sampled(prompt, n_new, T_, TOP_K, TOP_P, draws, k=k, ngram=3, start_pos=ctx)[0].tolist()
        for n_pass in range(1, 9):
            nxt = e.generate_lookahead_sampled(prompt, n_new, T_, TOP_K, TOP_P, draws, k=k, ngram=3, corpus=own,
                                               start_pos=ctx)[0].tolist()
            eq = next((i for i, (x, y) in enumerate(zip(nxt, own)) if x != y), n_new)
            print(f"  k={k:2d} corpus pass {n_pass}: first {eq} of {n_new} tokens equal the corpus", flush=True)
            own = nxt
            if eq == n_new:
                break
        used = set(own) | set(plain) | set(prompt)
        unrelated = [t for t in range(1000, 1000 + 8 * n_new) if t not in used][:2 * n_new]
        runs[f"sampled lookahead k={k:2d} own text as corpus"] = ("s", k, own)
        runs[f"sampled lookahead k={k:2d} unrelated corpus"] = ("s", k, unrelated)
        runs[f"greedy  lookahead k={k:2d} unrelated corpus"] = ("g", k, unrelated)
        same = next((i for i, (a, b) in enumerate(zip(own, plain)) if a != b), n_new)
        print(f"  k={k:2d} without corpus: first {same} of {n_new} tokens equal generate_sampled's", flush=True)
    res = {rn: [] for rn in runs}
    stats = {}
    for rnd in range(rounds + 1):                      # round 0 untimed (graph capture)
        for rn, spec in runs.items():
            t0 = time.perf_counter()
            if spec is None:
                e.generate_sampled([prompt], n_new, T_, TOP_K, TOP_P, draws, start_pos=[ctx])
                st = dict(steps=n_new, drafted=0, accepted=0, produced=n_new)
            elif spec[0] == "s":
                toks, _, st = e.generate_lookahead_sampled(prompt, n_new, T_, TOP_K, TOP_P, draws, k=spec[1], ngram=3,
                                                           corpus=spec[2], start_pos=ctx)
                st = dict(st, same=sum(x == y for x, y in zip(toks.tolist(), spec[2])))
            else:
                _, st = e.generate_lookahead(prompt, n_new, k=spec[1], ngram=3, corpus=spec[2], start_pos=ctx)
            dt = time.perf_counter() - t0
            stats[rn] = st
            if rnd:
                res[rn].append(dt)
    base = statistics.median(res["generate_sampled"]) / n_new
    for rn in runs:
        st = stats[rn]
        ms = [t * 1e3 / st["steps"] for t in res[rn]]
        tps = [st["produced"] / t for t in res[rn]]
        print(f"  {rn:46s} steps {st['steps']:4d} drafted {st['drafted']:5d} accepted {st['accepted']:4d} "
              f"tokens/step {st['produced'] / st['steps']:5.2f}  ms/step {spread(ms)}  tok/s {spread(tps)}"
              + (f"  tokens equal to the corpus: {st['same']} / {n_new}" if "own text" in rn else ""))
    for k in (3, 7, 15):
        s = statistics.median(res[f"sampled lookahead k={k:2d} unrelated corpus"]) / stats[f"sampled lookahead k={k:2d} unrelated corpus"]["steps"]
        g = statistics.median(res[f"greedy  lookahead k={k:2d} unrelated corpus"]) / stats[f"greedy  lookahead k={k:2d} unrelated corpus"]["steps"]
        print(f"  k={k:2d}: a sampled verify step costs {s / base:.2f} sampled plain steps ({s * 1e3:.3f} ms against "
              f"{base * 1e3:.3f} ms); the greedy verify step {g * 1e3:.3f} ms: the sampler launch over {k + 1} rows is "
              f"{(s - g) * 1e6:.0f} us = {100 * (s - g) / s:.1f} % of the sampled verify step")
    e.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
