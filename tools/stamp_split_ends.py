#!/usr/bin/env python3
"""Per-split workgroup ends of the fused QKV + attention launch from a raw stamp dump.

    TI_STAMP_RAW=raw.bin python tools/stamp_probe.py --model llama2-7b
    python tools/stamp_split_ends.py raw.bin [--splits 8]

ti_engine_stamp_steps writes the stamp words as read when TI_STAMP_RAW names a file.  For the launches tagged qkv
(workgroup = split + splits * head) this prints, per split, the mean over launches of the split's median and last
workgroup end (us from the launch's first entry) next to the launch's median and last end: a split that became
the launch's tail shows here (split S - 1 waits for the v rows the other splits publish)."""
from __future__ import annotations

import argparse
import sys

import numpy as np

TAG_QKV = 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("raw")
    ap.add_argument("--splits", type=int, default=8)
    args = ap.parse_args()
    b = np.fromfile(args.raw, np.uint8)
    n, steps, words = (int(x) for x in b[:24].view(np.uint64))
    o = 24
    info = b[o:o + 12 * n].view(np.int32).reshape(n, 3)
    o += 12 * n
    offs = b[o:o + 8 * n * steps].view(np.uint64).astype(np.int64)
    o += 8 * n * steps
    w = b[o:].view(np.uint64)
    S = args.splits
    med, last, all_med, all_last, cnt = np.zeros(S), np.zeros(S), 0.0, 0.0, 0
    for i in range(n * steps):
        kind, tag, wgs = info[i % n]
        if tag != TAG_QKV or wgs == 0 or wgs % S:
            continue
        p = w[offs[i]:offs[i] + wgs * words].reshape(wgs, words).astype(np.int64)
        if not p[:, 0].all():
            continue
        first = p[:, 0].min()
        ends = (p[:, 1:9].max(axis=1) - first) * 0.01   # s_memrealtime: 100 MHz
        for s in range(S):
            e = ends[s::S]
            med[s] += np.median(e)
            last[s] += e.max()
        all_med += np.median(ends)
        all_last += ends.max()
        cnt += 1
    if not cnt:
        print("no qkv launch in the dump")
        return 1
    print(f"{cnt} qkv launches; workgroup ends, us from the launch's first entry (mean over launches)")
    print(f"launch: median {all_med / cnt:.3f}  last {all_last / cnt:.3f}")
    for s in range(S):
        print(f"split {s}: median {med[s] / cnt:.3f}  last {last[s] / cnt:.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
