"""A Llama GGUF with Q4_K linear weights (ggml type 12, written here from NumPy bytes) through ModelLoader::load (fp32
values fl(fl(d sc) q) - fl(dmin m) bit for bit, the raw blocks as <name>.ggml_q4_k) and InferenceEngine (weight_bits 0
picks Q4_K super-blocks; greedy tokens equal those of the dequantized values at weight_bits 16), and what is refused."""
import json
import subprocess

import numpy as np
import pytest

from test_cpp_api import BIN, _gguf_oracle, api_check, read, write  # noqa: F401  (api_check: a fixture)
from test_gpu_cpp_api_mx import NAMES, gguf_write_raw

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
TOP = {"token_embeddings.weight": "token_embd.weight", "norm.weight": "output_norm.weight", "lm_head.weight": "output.weight"}


def q4k_tensor(rng, shape):
    """(block_q4_K bytes, the loader's fp32 values) of a random [out][in] tensor: every byte pattern is a block."""
    nb = shape[0] * shape[1] // 256
    raw = rng.randint(0, 256, (nb, 144)).astype(np.uint8)
    raw[:, 0:4] = np.stack([rng.uniform(0.5, 1.5, nb) * s for s in (3e-4, 2.2e-3)], 1).astype(f16).view(np.uint8)
    s, qs = raw[:, 4:16].astype(np.int32), raw[:, 16:].reshape(nb, 4, 1, 32)
    sc = np.concatenate([s[:, 0:4] & 63, (s[:, 8:12] & 15) | (s[:, 0:4] >> 6) << 4], axis=1).astype(f32)   # get_scale_min_k4
    m = np.concatenate([s[:, 4:8] & 63, (s[:, 8:12] >> 4) | (s[:, 4:8] >> 6) << 4], axis=1).astype(f32)
    q = np.concatenate([qs & 15, qs >> 4], axis=2).reshape(nb, 8, 32).astype(f32)   # chunk c: low nibbles 2c, high 2c + 1
    d, dmin = (raw[:, o:o + 2].copy().view(f16).astype(f32) for o in (0, 2))
    return raw.tobytes(), (((d * sc)[:, :, None] * q).astype(f32) - (dmin * m)[:, :, None]).astype(f32).reshape(shape)


def fails(*args):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    return r.stdout + r.stderr if r.returncode else ""


def test_q4k_gguf_through_loader_and_engine(api_check, golden, oracle, tmp_path):
    from pyoracle import OracleModel
    G, d, tmp = _gguf_oracle(), golden("decode_mini_gqa_w4"), tmp_path
    cfg = json.loads(str(d["cfg"]))
    m = OracleModel(oracle, cfg, int(d["seed"][0]), float(d["jitter"][0]))
    deq, rng, kq = m.weights(), np.random.RandomState(5), {}
    m.close()
    (tmp / "ref").mkdir()
    lines = [f"meta {cfg['vocab']} {cfg['hidden']} {cfg['layers']} {cfg['heads']} {cfg['inter']} {cfg['rope_theta']!r}"]
    for j, (ref, a) in enumerate(deq.items()):   # [K][N] under the reference's names, [out][in] in the file
        p = ref.split(".", 2)
        gg = f"blk.{p[1]}.{NAMES[p[2]]}.weight" if p[0] == "layers" else TOP[ref]
        kq[gg] = ref, tuple(a.shape), G.T_F32, a.tobytes()
        if a.ndim == 2 and gg != "token_embd.weight":
            raw, v = q4k_tensor(rng, a.T.shape)
            deq[ref], kq[gg] = np.ascontiguousarray(v.T), (ref, v.shape, 12, raw)
        write(tmp / "ref" / f"t{j}.bin", deq[ref])
        lines.append(f"{ref} t{j}.bin")
    (tmp / "ref" / "manifest.txt").write_text("\n".join(lines) + "\n")
    kvs = [("llama." + k, G.U32, cfg[c]) for k, c in [("vocab_size", "vocab"), ("embedding_length", "hidden"), ("block_count", "layers"),
           ("attention.head_count", "heads"), ("attention.head_count_kv", "kv_heads"), ("feed_forward_length", "inter")]]
    kvs += [("general.architecture", G.STR, "llama"), ("llama.rope.theta", G.F32, float(cfg["rope_theta"]))]
    q40 = bytes(G.quant_q4_0(deq["layers.0.attention.q_proj.weight"].T))   # one linear as Q4_0 blocks of the same values
    for name, retype in [("kq", lambda n, t, r: (t, r)), ("q5k", lambda n, t, r: (13 if t == 12 else t, r)),
                         ("mixed", lambda n, t, r: (G.T_Q4_0, q40) if n == "blk.0.attn_q.weight" else (t, r))]:
        gguf_write_raw(G, tmp / f"{name}.gguf", kvs, [(n, s) + retype(n, t, r) for n, (_, s, t, r) in kq.items()])
    # the loader: values and companions by name out of <dump>.meta / .data (the raw blocks: one byte an element)
    api_check("gguf_load", tmp / "kq.gguf", tmp / "dump")
    lines = open(str(tmp / "dump.meta")).read().split("\n")
    ne = int(lines[4])
    data, off, got = open(str(tmp / "dump.data"), "rb").read(), 0, {}
    for p in (ln.split() for ln in lines[6 + ne:6 + ne + int(lines[5 + ne])]):   # name, dtype code, ndim, dims
        n = int(np.prod([int(v) for v in p[3:]])) * (1 if p[0].endswith(".ggml_q4_k") else 4)
        got[p[0]], off = data[off:off + n], off + n
    for name, (ref, _, t, raw) in kq.items():   # a companion for every type-12 tensor and for no other
        assert got.get(name + ".ggml_q4_k") == (raw if t == 12 else None), name
        assert got[name] == np.ascontiguousarray(deq[ref].T if t == 12 else deq[ref], f32).tobytes(), name
    assert "unsupported ggml type 13" in fails("gguf_load", tmp / "q5k.gguf", tmp / "x")   # the other k-quants still raise
    prompts = write(tmp / "p.bin", np.array([d["prompt"].tolist()] * 2, np.int32))
    out_a = api_check("generate", tmp / "ref", prompts, 12, 1, 16, tmp / "a.bin")
    out_b = api_check("generate_gguf", tmp / "kq.gguf", prompts, 12, 1, 0, tmp / "b.bin")
    assert "Q4_K super-blocks" in out_b and "Q4_K" not in out_a, out_b
    a, b = read(tmp / "a.bin"), read(tmp / "b.bin")
    assert a.shape == b.shape and np.array_equal(a, b)
    assert "Q4_K" not in api_check("generate_gguf", tmp / "mixed.gguf", prompts, 2, 1, 0, tmp / "m.bin")
    assert "Q4_K" in fails("generate", tmp / "ref", prompts, 2, 1, 4 | 32 | 512, tmp / "x.bin")   # fp32 model: refused by name
