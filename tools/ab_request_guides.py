#!/usr/bin/env python3
"""Measurements behind per-request guides in continuous batching; the output is kept as
profiles/request_guides_ab.txt.

    TI_LIB_PARENT=<the parent commit's libturboinfer_amd.so> python tools/ab_request_guides.py [--part a|b|ab]
                  [--rounds 3] [--new 32] [--context 1984] [--requests 64]

Both libraries live in one process: this build through the package, the parent commit's through a second copy of
the package bound to TI_LIB_PARENT, so their routes alternate within a round.  Without TI_LIB_PARENT the parent's
routes run on this build's unchanged entry points (and the output says so).  The guide is tools/ab_guide.py's:
a 64-state cycle over V = 32000, state i allowing the 500 ids = i (mod 64) and moving to state i + 1 (mod 64).
(a) The guide launch alone, V = 32000, M = 1 / 8 / 64 rows, row m in state m (mod 64): the parent's scalar
    ti_guide_step, this build's scalar ti_guide_step, and ti_guide_step_rows over a library table whose rows all name
    that guide.  REP * REPLAYS back-to-back launches on one stream between two device events (the host enqueues
    faster than a launch runs, so the device never waits); the launch consumes no token (null step counter and
    carry), so every launch masks with the same state.  us per launch, median [min .. max] over the rounds, and the
    table form's difference to the parent beside the parent's own run-to-run spread.
(b) A mixed batch on the synthetic INT4 Llama-2-7B at max_seq 2048: --requests requests with prompts of --context
    tokens through max_batch = --requests slots, (T 0.8, top_k 40, top_p 0.9), the even requests under the cycle
    guide and the odd ones unguided.  As one ti_engine_serve_requests_guided call, and as the only route the parent
    has: ti_engine_set_guide + ti_engine_serve_requests with the guided half, then ti_engine_set_guide(NULL) + the
    unguided half, each call with half of its slots idle and each change of guide dropping the step graphs.  The
    clock is around the whole route, recaptures and prefill included; tok/s = all new tokens over it.  The tokens of
    both routes are compared first.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ab_guide import STATES, cycle  # noqa: E402
from ab_requests import engine, packages, spread, workload  # noqa: E402
from bench import MODELS  # noqa: E402

REP, REPLAYS = 50, 4
T_, K_, P_ = 0.8, 40, 0.9
CAP = 64


def part_a(T, P, rounds: int) -> None:
    import numpy as np
    L = T.lib()
    V = MODELS["llama2-7b"][0]
    W = (V + 31) // 32
    n = REP * REPLAYS
    row_ptr, tokens, nxt = cycle(V)
    mask = np.zeros((STATES, W), np.uint32)
    for s in range(STATES):
        a = tokens[row_ptr[s]: row_ptr[s + 1]].astype(np.int64)
        np.bitwise_or.at(mask[s], a >> 5, np.uint32(1) << (a & 31).astype(np.uint32))
    d = [T.DeviceBuffer.from_array(x) for x in (row_ptr, tokens, nxt, mask)]
    gd = T.GuideDev(STATES, W, *(x.ptr for x in d))
    table = (T.GuideDev * CAP)()
    table[2] = gd                                          # handle 3
    table_d = T.DeviceBuffer.from_array(np.frombuffer(bytes(table), np.uint8))
    print(f"(a) the guide launch alone, V = {V}, {STATES}-state cycle ({V // STATES} allowed ids per state): us per launch, "
          f"median [min .. max] of {rounds} rounds of {n} back-to-back launches on one stream between two device events, "
          f"routes alternating within a round; parent = {'TI_LIB_PARENT' if P else 'this build (no TI_LIB_PARENT)'}")
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    T.check(L.ti_stream_create(C.byref(stream)))
    T.check(L.ti_event_create(C.byref(ev0)))
    T.check(L.ti_event_create(C.byref(ev1)))
    for M in (1, 8, 64):
        rng = np.random.default_rng(M)
        host = (rng.standard_normal((M, V)) * 3).astype(np.float32)
        logits = T.DeviceBuffer.from_array(host)
        state = T.DeviceBuffer.from_array((np.arange(M) % STATES).astype(np.int32))
        tab = np.zeros(M, np.dtype([("t", np.float32), ("k", np.int32), ("p", np.float32), ("pen", np.float32, 3), ("res", np.int32, 2)]))
        tab[:] = (T_, K_, P_, (1.0, 0.0, 0.0), (3, 0))
        tab_d = T.DeviceBuffer.from_array(tab)
        rows_args = T.GuideArgs(logits.ptr, V, M, V, T.GuideDev(), state.ptr, 1, 1, None, None, None, 0, None)

        def scalar(pkg):                                       # (each copy of the package has its own ctypes classes)
            g = pkg.GuideDev(STATES, W, *(x.ptr for x in d))
            args = pkg.GuideArgs(logits.ptr, V, M, V, g, state.ptr, 1, 1, None, None, None, 0, None)
            return lambda s: pkg.lib().ti_guide_step(C.byref(args), s)

        def rows(s):
            return L.ti_guide_step_rows(C.byref(rows_args), table_d.ptr, CAP, tab_d.ptr, s)
        routes = {"parent scalar": scalar(P or T), "scalar": scalar(T), "table": rows}
        out = {}
        for rn, fn in routes.items():
            logits.upload(host)
            T.check(fn(stream))
            T.check(L.ti_stream_sync(stream))
            out[rn] = logits.download(np.uint32, (M, V)).copy()
        same = all(np.array_equal(out[rn], out["table"]) for rn in routes)
        ninf = int((out["table"] == 0xFF800000).sum()) // M
        times = {rn: [] for rn in routes}
        for rnd in range(rounds + 1):                          # round 0 untimed
            for rn, fn in routes.items():
                T.check(L.ti_event_record(ev0, stream))
                for _ in range(n):
                    fn(stream)
                T.check(L.ti_event_record(ev1, stream))
                ms = C.c_float()
                T.check(L.ti_event_elapsed_ms(ev0, ev1, C.byref(ms)))
                if rnd:
                    times[rn].append(ms.value * 1e3 / n)
        for rn in routes:
            print(f"  M = {M:2d}  {rn:14s} {spread(times[rn])} us per launch")
        par = times["parent scalar"]
        print(f"  M = {M:2d}  table - parent: {statistics.median(times['table']) - statistics.median(par):+.2f} us; the parent's "
              f"own spread (max - min): {max(par) - min(par):.2f} us; rows of the three routes bit-equal: {same} "
              f"({ninf} of {V} columns at -inf per row)")
        sys.stdout.flush()


def part_b(T, P, rounds: int, n_new: int, context: int, n_req: int) -> None:
    import numpy as np
    V = MODELS["llama2-7b"][0]
    prompts, draws = workload(np, V, n_req, context, n_new)
    guide = cycle(V)
    guided = list(range(0, n_req, 2))
    free = list(range(1, n_req, 2))
    q = dict(max_new=n_new, temperature=T_, top_k=K_, top_p=P_)
    print(f"(b) a mixed batch: {n_req} requests of {context} prompt tokens, {n_new} new tokens each (T {T_}, top_k {K_}, top_p "
          f"{P_}), {n_req} slots, chunk 16, synthetic INT4 llama2-7b at max_seq 2048; the even requests under the "
          f"{STATES}-state cycle guide, the odd ones unguided; tok/s = all new tokens over the whole route (prefill and "
          f"graph captures included), median [min .. max] of {rounds} alternating rounds; split route on "
          f"{'TI_LIB_PARENT' if P else 'this build (no TI_LIB_PARENT)'}")
    ep, et = engine(P or T, n_req), engine(T, n_req)
    handle = et.add_guide(*guide)

    def mixed():
        gh = [handle if r % 2 == 0 else 0 for r in range(n_req)]
        return et.serve_requests(prompts, [q] * n_req, draws, chunk=16, guides=gh)[0]

    def split():
        out = [None] * n_req
        for idx, g in ((guided, guide), (free, None)):
            ep.set_guide(*g) if g else ep.set_guide(None)
            toks, _ = ep.serve_requests([prompts[r] for r in idx], [q] * len(idx), draws[idx], chunk=16)
            for r, tk in zip(idx, toks):
                out[r] = tk
        return out
    routes = {"set_guide + 2 serve_requests calls": split, "1 serve_requests_guided call": mixed}
    res, toks = {rn: [] for rn in routes}, {}
    for rnd in range(rounds + 1):                              # round 0 untimed; its tokens are compared
        for rn, fn in routes.items():
            t0 = time.perf_counter()
            toks[rn] = fn()
            dt = time.perf_counter() - t0
            if rnd:
                res[rn].append(n_req * n_new / dt)
        if rnd == 0:
            a, b = toks.values()
            eq = sum(x == y for x, y in zip(a, b))
            ok = all(all(t % STATES == i % STATES for i, t in enumerate(b[r])) for r in guided)
            print(f"  requests whose tokens are equal in both routes: {eq} / {n_req}; every guided request accepted by the "
                  f"cycle: {ok}")
    for rn in routes:
        print(f"    {rn:36s} {spread(res[rn])} tok/s")
    a, b = (statistics.median(res[rn]) for rn in ("1 serve_requests_guided call", "set_guide + 2 serve_requests calls"))
    print(f"    one call / split: x{a / b:.2f}")
    sys.stdout.flush()
    ep.close()
    et.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--context", type=int, default=1984)
    ap.add_argument("--requests", type=int, default=64)
    args = ap.parse_args()
    T, P = packages()
    T.init(0)
    if P:
        P.init(0)
    if "a" in args.part:
        part_a(T, P, args.rounds)
    if "b" in args.part:
        part_b(T, P, args.rounds, args.new, args.context, args.requests)
    return 0


if __name__ == "__main__":
    sys.exit(main())
