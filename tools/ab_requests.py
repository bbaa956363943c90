#!/usr/bin/env python3
"""Measurements behind per-request parameters in continuous batching; the output is kept as
profiles/requests_ab.txt.

    TI_LIB_PARENT=<the parent commit's libturboinfer_amd.so> python tools/ab_requests.py [--part a|b|c|abc]
                  [--rounds 3] [--new 32] [--context 1984] [--requests 64]

Both libraries live in one process: this build through the package, the parent commit's through a second copy of
the package bound to TI_LIB_PARENT, so their routes alternate within a round.  Without TI_LIB_PARENT the parent's
routes run on this build's unchanged entry points (and the output says so).
(a) The sampler launch alone, (T 0.8, top_k 40, top_p 0.9), V = 32000, M = 1 / 8 / 64 rows: the parent's scalar
    ti_sample_device, this build's scalar ti_sample_device, and ti_sample_device_rows with a uniform table.
    REP * REPLAYS back-to-back launches on one stream between two device events (a launch runs ~30 us, the host
    enqueues faster, so the device never waits); us per launch, median [min .. max] over the rounds, and the table
    form's difference to the parent beside the parent's own run-to-run spread.
(b) The full loop with uniform parameters on the synthetic INT4 Llama-2-7B at max_seq 2048: --requests requests with
    prompts of --context tokens through max_batch = --requests slots, all on one parameter set: the parent's
    ti_engine_serve_sampled against ti_engine_serve_requests.  Wall clock around the calls (they synchronise), one
    untimed round first (graph capture); each route is timed with one new token and with --new, and the decode rate
    is (new - 1) tokens per request over the difference, so the prompts' prefill is not in it.
(c) A mixed batch: the requests cycle over 4 parameter sets, with and without penalties in one of them.  As one
    ti_engine_serve_requests call, and as what a user has today: one ti_engine_serve_sampled call per set with that
    set's requests (and ti_engine_set_penalties before it), each call with most of its slots idle and every change of
    parameters dropping the step graphs.  The clock is around the whole route, recaptures and prefill included;
    tok/s = all new tokens over it.  The tokens of both routes are compared first.
"""
from __future__ import annotations

import argparse
import ctypes as C
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import MODELS  # noqa: E402

REP, REPLAYS = 50, 4
T_, K_, P_ = 0.8, 40, 0.9
SETS = [((1.0, 1, 1.0), (1.0, 0.0, 0.0)), ((0.8, 40, 0.9), (1.0, 0.0, 0.0)), ((1.2, 200, 1.0), (1.3, 0.2, 0.1)),
        ((0.7, 1024, 0.5), (1.0, 0.0, 0.0))]


def spread(v):
    return f"{statistics.median(v):9.2f} [{min(v):8.2f} .. {max(v):8.2f}]"


def packages():
    """-> (this build's package, the parent's or None)."""
    import turboinfer_amd as T
    path = os.environ.get("TI_LIB_PARENT")
    if not path:
        return T, None
    os.environ["TI_LIB"] = path                      # read when the package is executed
    spec = importlib.util.spec_from_file_location("turboinfer_amd_parent", os.path.join(ROOT, "turboinfer_amd", "__init__.py"))
    P = importlib.util.module_from_spec(spec)
    sys.modules["turboinfer_amd_parent"] = P
    spec.loader.exec_module(P)
    del os.environ["TI_LIB"]
    assert P.LIB_PATH == path and T.LIB_PATH != path
    return T, P


def part_a(T, P, rounds: int) -> None:
    import numpy as np
    L = T.lib()
    V = MODELS["llama2-7b"][0]
    n = REP * REPLAYS
    print(f"(a) the sampler launch alone (T {T_}, top_k {K_}, top_p {P_}), V = {V}: us per launch, median [min .. max] of "
          f"{rounds} rounds of {n} back-to-back launches on one stream between two device events (the queue stays ahead "
          f"of the device), routes alternating within a round; parent = {'TI_LIB_PARENT' if P else 'this build (no TI_LIB_PARENT)'}")
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    T.check(L.ti_stream_create(C.byref(stream)))
    T.check(L.ti_event_create(C.byref(ev0)))
    T.check(L.ti_event_create(C.byref(ev1)))
    for M in (1, 8, 64):
        rng = np.random.default_rng(M)
        logits = T.DeviceBuffer.from_array((rng.standard_normal((M, V)) * 3).astype(np.float32))
        draws = T.DeviceBuffer.from_array(rng.uniform(0.01, 0.99, M).astype(np.float32))
        tok, lp = T.DeviceBuffer(M * 4), T.DeviceBuffer(M * 4)
        tab = np.zeros(M, np.dtype([("t", np.float32), ("k", np.int32), ("p", np.float32), ("pen", np.float32, 3), ("res", np.int32, 2)]))
        tab[:] = (T_, K_, P_, (1.0, 0.0, 0.0), (0, 0))
        tab_d = T.DeviceBuffer.from_array(tab)

        def scalar(lib):
            return lambda s: lib.ti_sample_device(logits.ptr, V, M, V, T_, K_, P_, draws.ptr, tok.ptr, lp.ptr, s)

        def rows(s):
            return L.ti_sample_device_rows(logits.ptr, V, M, V, tab_d.ptr, K_, draws.ptr, tok.ptr, lp.ptr, None, s)
        routes = {"parent scalar": scalar((P or T).lib()), "scalar": scalar(L), "table": rows}
        out = {}
        for rn, fn in routes.items():
            T.check(fn(stream))
            T.check(L.ti_stream_sync(stream))
            out[rn] = (tok.download(np.int32, M).copy(), lp.download(np.uint32, M).copy())
        same = all(np.array_equal(out[rn][0], out["table"][0]) and np.array_equal(out[rn][1], out["table"][1]) for rn in routes)
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
              f"own spread (max - min): {max(par) - min(par):.2f} us; tokens and log p of the three routes equal: {same}")
        sys.stdout.flush()


def workload(np, V, n_req, context, n_new):
    rng = np.random.default_rng(7 + n_req)
    prompts = [(3 + rng.permutation(V - 3)[:context]).tolist() for _ in range(n_req)]
    draws = rng.uniform(1e-6, 1, (n_req, n_new)).astype(np.float32)
    return prompts, draws


def engine(M, n_req):
    V, H, layers, nh, nkv, hd, I, bits, theta = MODELS["llama2-7b"]
    e = M.Engine(V, H, layers, nh, nkv, hd, I, bits=bits, max_seq=2048, max_batch=n_req, rope_theta=theta)
    e.synth(0x7157, 0.0)
    return e


def part_b(T, P, rounds: int, n_new: int, context: int, n_req: int) -> None:
    import numpy as np
    V = MODELS["llama2-7b"][0]
    prompts, draws = workload(np, V, n_req, context, n_new)
    print(f"(b) uniform parameters (T {T_}, top_k {K_}, top_p {P_}): synthetic INT4 llama2-7b, max_seq 2048, {n_req} requests "
          f"of {context} prompt tokens through {n_req} slots, {n_new} new tokens each, chunk 16; decode tok/s over all "
          f"requests, median [min .. max] of {rounds} alternating rounds; parent = "
          f"{'TI_LIB_PARENT' if P else 'this build (no TI_LIB_PARENT)'}")
    ep, et = engine(P or T, n_req), engine(T, n_req)

    def sampled(new):
        return ep.serve_sampled(prompts, new, T_, K_, P_, draws[:, :new], eos=-1, chunk=16)

    def requests(new):
        q = [dict(max_new=new, temperature=T_, top_k=K_, top_p=P_)] * n_req
        return et.serve_requests(prompts, q, draws[:, :new], chunk=16)
    routes = {"parent serve_sampled": sampled, "serve_requests": requests}
    res, toks = {rn: [] for rn in routes}, {}
    for rnd in range(rounds + 1):                              # round 0 untimed (graph capture)
        for rn, fn in routes.items():
            t0 = time.perf_counter()
            fn(1)
            t1 = time.perf_counter()
            toks[rn], _ = fn(n_new)
            t2 = time.perf_counter()
            if rnd:
                res[rn].append(n_req * (n_new - 1) / ((t2 - t1) - (t1 - t0)))
    for rn in routes:
        print(f"  {rn:22s} {spread(res[rn])} tok/s")
    a, b = statistics.median(res["serve_requests"]), statistics.median(res["parent serve_sampled"])
    par = res["parent serve_sampled"]
    print(f"  serve_requests / parent: x{a / b:.3f}; the parent's own spread: x{min(par) / b:.3f} .. x{max(par) / b:.3f}; "
          f"tokens equal: {toks['serve_requests'] == toks['parent serve_sampled']}")
    sys.stdout.flush()
    ep.close()
    et.close()


def part_c(T, P, rounds: int, n_new: int, context: int, n_req: int) -> None:
    import numpy as np
    V = MODELS["llama2-7b"][0]
    prompts, draws = workload(np, V, n_req, context, n_new)
    ns = len(SETS)
    print(f"(c) a mixed batch: {n_req} requests of {context} prompt tokens over {ns} parameter sets (request r: set r mod {ns}), "
          f"{n_new} new tokens each, {n_req} slots, chunk 16; tok/s = all new tokens over the whole route (prefill and "
          f"graph captures included), median [min .. max] of {rounds} alternating rounds; split route on "
          f"{'TI_LIB_PARENT' if P else 'this build (no TI_LIB_PARENT)'}")
    ep, et = engine(P or T, n_req), engine(T, n_req)
    for with_pen in (False, True):
        sets = [(s, pen if with_pen else (1.0, 0.0, 0.0)) for s, pen in SETS]

        def mixed():
            q = [dict(max_new=n_new, temperature=sets[r % ns][0][0], top_k=sets[r % ns][0][1], top_p=sets[r % ns][0][2],
                      repetition=sets[r % ns][1][0], presence=sets[r % ns][1][1], frequency=sets[r % ns][1][2])
                 for r in range(n_req)]
            return et.serve_requests(prompts, q, draws, chunk=16)[0]

        def split():
            out = [None] * n_req
            for s, ((t, k, p), pen) in enumerate(sets):
                idx = list(range(s, n_req, ns))
                ep.set_penalties(*pen)
                toks, _ = ep.serve_sampled([prompts[r] for r in idx], n_new, t, k, p, draws[idx], eos=-1, chunk=16)
                for r, tk in zip(idx, toks):
                    out[r] = tk
            ep.set_penalties()
            return out
        routes = {f"{ns} serve_sampled calls": split, "1 serve_requests call": mixed}
        res, toks = {rn: [] for rn in routes}, {}
        for rnd in range(rounds + 1):                          # round 0 untimed; its tokens are compared
            for rn, fn in routes.items():
                t0 = time.perf_counter()
                toks[rn] = fn()
                dt = time.perf_counter() - t0
                if rnd:
                    res[rn].append(n_req * n_new / dt)
            if rnd == 0:
                eq = sum(a == b for a, b in zip(*toks.values()))
                print(f"  penalties in set 2: {'(1.3, 0.2, 0.1)' if with_pen else 'none'}; requests whose tokens are equal "
                      f"in both routes: {eq} / {n_req}")
        for rn in routes:
            print(f"    {rn:24s} {spread(res[rn])} tok/s")
        a, b = (statistics.median(res[rn]) for rn in ("1 serve_requests call", f"{ns} serve_sampled calls"))
        print(f"    one call / split: x{a / b:.2f}")
        sys.stdout.flush()
    ep.close()
    et.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="abc")
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
    if "c" in args.part:
        part_c(T, P, args.rounds, args.new, args.context, args.requests)
    return 0


if __name__ == "__main__":
    sys.exit(main())
