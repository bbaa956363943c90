"""Scoring throughput (Engine.score / ti_engine_score) next to the prefill it is built on (GPU box):
    python tools/score_bench.py [reps]
Llama-2-7B shape, INT4, synthetic weights.  For 512 and 2048 tokens: the time of score(tokens)
(every position's log-probability, one read-back) and of generate(tokens, max_new=1) over the same
tokens (the prefill of every token + one lm_head row + the read-back), alternating, host clock around
calls that end in a device synchronise; medians and the spread of `reps` repetitions after a warm-up
of both.  The expected extra of score over generate is ceil(n / 128) lm_head passes plus the logits
traffic ("Scoring").  No threshold: this prints what it measures."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import turboinfer_amd as T  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
V = 32000
T.init(0)
e = T.Engine(V, 4096, 32, 32, 32, 128, 11008, bits=4, max_seq=2048, max_batch=1)
e.synth(0x7157, 0.0)


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


for n in (512, 2048):
    tokens = np.random.RandomState(n).randint(0, V, size=n).astype(np.int32)
    prompt = tokens.tolist()
    targets = np.concatenate([tokens[1:], [-1]]).astype(np.int32)
    c0 = e.counters()
    lp = e.score(tokens, targets)          # warm-up of both paths (module loads, buffers)
    c1 = e.counters()
    e.generate([prompt], 1)
    ts, tg = [], []
    for _ in range(reps):                  # alternating: both see the same machine state
        tg.append(timed(lambda: e.generate([prompt], 1)))
        ts.append(timed(lambda: e.score(tokens, targets)))
    ms, mg = float(np.median(ts)), float(np.median(tg))
    ppl = float(np.exp(-np.mean(lp[:-1].astype(np.float64))))
    print(f"n {n:4d}: score {ms:8.2f} ms (min {min(ts):.2f} max {max(ts):.2f}) = {n / ms * 1e3:8.0f} scored tok/s | "
          f"generate(max_new=1) {mg:8.2f} ms (min {min(tg):.2f} max {max(tg):.2f}) | score / generate {ms / mg:.3f} | "
          f"{c1[1] - c0[1]} prefill chunk(s), {-(-n // 128)} lm_head blocks, perplexity {ppl:.1f} (synthetic weights)",
          flush=True)
e.close()
