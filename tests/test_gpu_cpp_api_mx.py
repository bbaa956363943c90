"""A Llama GGUF whose linear weights are MXFP4 blocks (ggml type 39, written here from NumPy codes and e8m0 bytes) through
ModelLoader::load and InferenceEngine, driven like test_cpp_api.py::test_inference_engine_keeps_gguf_q_blocks: with
weight_bits 0 the dequantized values are recognised as MX blocks (recover_mx) and the engine reports them; the greedy
tokens equal those of the same values under the reference's names with weight_bits 4 | 32 | 256.  The same model
written as Q4_0 still reports Q4_0 blocks."""
import json
import struct

import numpy as np
import pytest

from test_cpp_api import _gguf_oracle, api_check, read, write  # noqa: F401  (api_check: a fixture)
from test_gpu_gemm_mx import E2M1

pytestmark = pytest.mark.gpu
NAMES = {"attention.q_proj.weight": "attn_q", "attention.k_proj.weight": "attn_k", "attention.v_proj.weight": "attn_v",
         "attention.o_proj.weight": "attn_output", "feed_forward.w3.weight": "ffn_gate", "feed_forward.w1.weight": "ffn_up",
         "feed_forward.w2.weight": "ffn_down", "attention_norm.weight": "attn_norm", "ffn_norm.weight": "ffn_norm"}


def mx_tensor(rng, shape):
    """(block_mxfp4 bytes, dequantized values) of a random [out][in] tensor: byte 0 e, qs[j] = element j | j + 16 << 4."""
    out, k = shape
    codes = rng.randint(0, 16, (out, k // 32, 32)).astype(np.uint8)
    e = (127 + int(np.round(np.log2(0.1 / np.sqrt(k)))) + rng.randint(-1, 2, (out, k // 32, 1))).astype(np.uint8)
    raw = np.concatenate([e, codes[..., :16] | (codes[..., 16:] << 4)], axis=2)
    return raw.tobytes(), (E2M1[codes] * np.exp2(e.astype(np.float64) - 127)).astype(np.float32).reshape(out, k)


def gguf_write_raw(G, path, kvs, tensors):   # tensors: (name, row-major shape, ggml type, stored bytes)
    head = struct.pack("<IIQQ", G.MAGIC, G.VERSION, len(tensors), len(kvs))
    head += b"".join(G._str(k) + struct.pack("<I", t) + G._value(t, v) for k, t, v in kvs)
    data = b""
    for name, shape, tt, raw in tensors:
        head += G._str(name) + struct.pack("<I", len(shape)) + b"".join(struct.pack("<Q", d) for d in reversed(shape))
        head += struct.pack("<IQ", tt, len(data))
        data += raw + b"\0" * (-len(raw) % 32)
    open(path, "wb").write(head + b"\0" * (-len(head) % 32) + data)


def test_inference_engine_keeps_gguf_mxfp4_blocks(api_check, golden, oracle, tmp_path):
    from pyoracle import OracleModel
    G, d = _gguf_oracle(), golden("decode_mini_gqa_w4")
    cfg = json.loads(str(d["cfg"]))
    m = OracleModel(oracle, cfg, int(d["seed"][0]), float(d["jitter"][0]))
    w = m.weights()
    m.close()
    rng, deq = np.random.RandomState(5), dict(w)
    f32 = lambda a: (tuple(a.shape), G.T_F32, np.asarray(a, np.float32).tobytes())   # noqa: E731
    mx, q4 = [("token_embd.weight",) + f32(w["token_embeddings.weight"]), ("output_norm.weight",) + f32(w["norm.weight"])], []
    for ref, gg in [("lm_head.weight", "output.weight")] + [(f"layers.{l}.{r}", f"blk.{l}.{g}.weight")
                                                          for l in range(cfg["layers"]) for r, g in NAMES.items()]:
        if w[ref].ndim == 2:   # [K][N] under the reference's names, [out][in] in the file
            raw, v = mx_tensor(rng, w[ref].T.shape)
            deq[ref] = np.ascontiguousarray(v.T)
            mx.append((gg, v.shape, 39, raw))
            q4.append((gg, np.ascontiguousarray(w[ref].T), G.T_Q4_0))
        else:
            mx.append((gg,) + f32(w[ref]))
            q4.append((gg, w[ref], G.T_F32))
    kvs = [("general.architecture", G.STR, "llama"), ("llama.vocab_size", G.U32, cfg["vocab"]),
           ("llama.embedding_length", G.U32, cfg["hidden"]), ("llama.block_count", G.U32, cfg["layers"]),
           ("llama.attention.head_count", G.U32, cfg["heads"]), ("llama.attention.head_count_kv", G.U32, cfg["kv_heads"]),
           ("llama.feed_forward_length", G.U32, cfg["inter"]), ("llama.rope.theta", G.F32, float(cfg["rope_theta"]))]
    gguf_write_raw(G, tmp_path / "mx.gguf", kvs, mx)
    G.gguf_write(tmp_path / "q4.gguf", kvs, [("token_embd.weight", w["token_embeddings.weight"], G.T_F32),
                                             ("output_norm.weight", w["norm.weight"], G.T_F32)] + q4)
    mdir = tmp_path / "ref"
    mdir.mkdir()
    lines = [f"meta {cfg['vocab']} {cfg['hidden']} {cfg['layers']} {cfg['heads']} {cfg['inter']} {cfg['rope_theta']!r}"]
    for j, (k, v) in enumerate(deq.items()):
        write(mdir / f"t{j}.bin", v.astype(np.float32))
        lines.append(f"{k} t{j}.bin")
    (mdir / "manifest.txt").write_text("\n".join(lines) + "\n")
    prompts = write(tmp_path / "p.bin", np.array([d["prompt"].tolist()] * 2, np.int32))
    out_a = api_check("generate", mdir, prompts, 12, 1, 4 | 32 | 256, tmp_path / "a.bin")
    out_b = api_check("generate_gguf", tmp_path / "mx.gguf", prompts, 12, 1, 0, tmp_path / "b.bin")
    assert "MXFP4 blocks" in out_a and "MXFP4 blocks" in out_b, out_b
    a, b = read(tmp_path / "a.bin"), read(tmp_path / "b.bin")
    assert a.shape == b.shape and np.array_equal(a, b)
    out_q = api_check("generate_gguf", tmp_path / "q4.gguf", prompts, 2, 1, 0, tmp_path / "q.bin")
    assert "group-32 blocks" in out_q and "MXFP4" not in out_q and "affine" not in out_q, out_q
