"""Time the prompt-chunk attention launches alone (HIP events, 50 launches each): a 7B prompt chunk (32
heads, hd 128) of M rows at positions 0..M-1 through ti_attn_prefill (fp16 cache), ti_attn_prefill_f8 (e4m3
cache: the e4m3 of the same random fp16 arrays) and the decode route of both (ti_attn_decode /
ti_attn_decode_f8 at stride 0).  Each shape runs the launches A B C D A B C D (--rounds) in this one process.

    [TI_LIB=...] python tools/prefill_attn_time.py [--rounds 2] [--mode 0..3]

--mode: ti_attn_prefill_set_kernel for both prefill entry points (0 automatic)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import turboinfer_amd as T  # noqa: E402

SHAPES = [(32, 128), (32, 256), (32, 512), (32, 1024), (8, 512)]   # (kv_heads, M): 7B MHA; Llama-3-8B GQA 4


def e4m3(x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).clamp(-448.0, 448.0)
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()


def main(rounds=2, mode=0, tag=""):
    T.init(0)
    L = T.lib()
    L.ti_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    a, b = C.c_void_p(), C.c_void_p()
    T.check(L.ti_event_create(C.byref(a)))
    T.check(L.ti_event_create(C.byref(b)))
    heads, hd, max_seq = 32, 128, 2048
    rng = np.random.RandomState(0)
    has_f8 = hasattr(L, "ti_attn_prefill_f8")           # (older TI_LIB builds lack it)
    prev = L.ti_attn_prefill_set_kernel(mode)
    for kvh, M in SHAPES:
        k16 = rng.standard_normal((kvh, max_seq, hd)).astype(np.float16)
        v16 = rng.standard_normal((kvh, max_seq, hd)).astype(np.float16)
        kc, vc = T.DeviceBuffer.from_array(k16), T.DeviceBuffer.from_array(v16)
        k8, v8 = T.DeviceBuffer.from_array(e4m3(k16)), T.DeviceBuffer.from_array(e4m3(v16))
        q = T.DeviceBuffer.from_array(rng.standard_normal((M, heads * hd)).astype(np.float32))
        pos = T.DeviceBuffer.from_array(np.arange(M, dtype=np.int32))
        out = T.DeviceBuffer(M * heads * hd * 2)
        ws = T.DeviceBuffer(L.ti_attn_workspace_bytes(M, heads, hd, 4))
        ws.zero()
        runs = {"prefill fp16": lambda: L.ti_attn_prefill(q.ptr, kc.ptr, vc.ptr, max_seq, pos.ptr, M, heads, kvh, hd, out.ptr, None)}
        if has_f8:
            runs["prefill e4m3"] = lambda: L.ti_attn_prefill_f8(q.ptr, k8.ptr, v8.ptr, max_seq, pos.ptr, M, heads, kvh, hd,
                                                               out.ptr, None)
        runs["decode fp16"] = lambda: L.ti_attn_decode(q.ptr, kc.ptr, vc.ptr, 0, max_seq, pos.ptr, M, heads, kvh, hd, 4,
                                                       ws.ptr, out.ptr, None)
        if hasattr(L, "ti_attn_decode_f8"):
            runs["decode e4m3"] = lambda: L.ti_attn_decode_f8(q.ptr, k8.ptr, v8.ptr, 0, max_seq, pos.ptr, M, heads, kvh, hd, 4,
                                                             ws.ptr, out.ptr, None)
        for rnd in range(rounds):
            for name, f in runs.items():
                T.check(f())
                T.check(L.ti_event_record(a, None))
                for _ in range(50):
                    f()
                T.check(L.ti_event_record(b, None))
                ms = C.c_float()
                T.check(L.ti_event_elapsed_ms(a, b, C.byref(ms)))
                print(f"{tag}M {M:5d} kv_heads {kvh:2d} mode {mode} round {rnd} {name:13s}: {ms.value * 1e3 / 50:8.1f} us per launch",
                      flush=True)
    L.ti_attn_prefill_set_kernel(prev)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--mode", type=int, default=0, choices=(0, 1, 2, 3))
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    main(args.rounds, args.mode, args.tag)
