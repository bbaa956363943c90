// engine.cpp -- the device-resident decode engine (ti_engine.h).
//
// State per engine (one device, one HIP stream):
//   * packed weights: per layer one fused [q|k|v] linear, o, one gate/up linear with rows
//     interleaved by 8 (so the SiLU*up epilogue sees both halves in one 16-row tile), down;
//     lm_head; fp16 embedding table; fp32 norm weights; RoPE (cos, sin) table computed on
//     the host with the reference formula (tensor_engine.cpp:1561-1566, 1595-1597).
//   * per stream fp16 K/V caches [layer][stream][kv_head][max_seq][head_dim].
//   * a device-side decode loop: step counter, positions, argmax feedback -- one decode
//     step is a fixed launch sequence captured once into a hipGraph and replayed, so the
//     host never waits inside generate().
// Reference counterparts: InferenceEngineImpl (src/model/inference_engine.cpp:446-693),
// KVCache (:25-172), forward_pass_incremental (:1493-1552), generate (:734-802).
//
// This file: creation, weights, the KV cache's fill / read, the settings.  The step and its graph cache are in
// engine_step.cpp, the entry points that run it in engine_generate / _serve / _beam / _lookahead.cpp, the timing
// and stamp diagnostics in engine_diag.cpp; engine_impl.hpp declares what they share.
#include "engine_impl.hpp"

using namespace ti_eng;

namespace {

// tensor ids of the synthetic model: identical to oracle/ti_oracle.c
constexpr uint32_t kTidEmb = 1, kTidOutNorm = 2, kTidLmHead = 3, kTidLayer0 = 16;
enum { TL_ATTN_NORM = 0, TL_FFN_NORM, TL_Q, TL_K, TL_V, TL_O, TL_G, TL_U, TL_D };
inline uint32_t tid_layer(int l, int t) { return kTidLayer0 + 16u * (uint32_t)l + (uint32_t)t; }
inline uint32_t tid_kv(int l, int v) { return 0x100000u + 2u * (uint32_t)l + (uint32_t)v; }

uint16_t host_half(float f) {
  const _Float16 h = (_Float16)f;
  uint16_t u;
  std::memcpy(&u, &h, 2);
  return u;
}

int validate(const ti_engine_config& c) {
  if (c.vocab < 1 || c.hidden < 1 || c.layers < 0 || c.inter < 1 || c.max_seq < 1 || c.max_batch < 1)
    return ti_set_error(TI_ERR_ARG, "ti_engine_create: non-positive size in config");
  if (c.compat) {
    if (c.bits & TI_BITS_KV8) return ti_set_error(TI_ERR_ARG, "ti_engine_create: TI_BITS_KV8 on a compat engine (no KV cache)");
    return TI_OK;
  }
  if (c.heads < 1 || c.kv_heads < 1 || c.heads % c.kv_heads)
    return ti_set_error(TI_ERR_ARG, "ti_engine_create: heads %d / kv_heads %d", c.heads, c.kv_heads);
  const int G = c.heads / c.kv_heads;
  if (G != 1 && G != 2 && G != 4 && G != 8) return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_create: GQA group %d", G);
  if (c.head_dim != 64 && c.head_dim != 128) return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_create: head_dim %d", c.head_dim);
  const int wbits = c.bits & ~TI_BITS_KV8;   // the weight format; TI_BITS_KV8 goes with every one
  if (wbits != 4 && wbits != 8 && wbits != 16 && wbits != (4 | TI_BITS_G32) && wbits != (8 | TI_BITS_G32) &&
      wbits != (4 | TI_BITS_G32 | TI_BITS_AFF))
    return ti_set_error(TI_ERR_ARG, "ti_engine_create: bits %d (4, 8, 16; 4 or 8 | TI_BITS_G32; 4 | TI_BITS_G32 | "
                        "TI_BITS_AFF; each | TI_BITS_KV8)", c.bits);
  const int qd = c.heads * c.head_dim, kvd = c.kv_heads * c.head_dim;
  if (c.hidden % 128 || qd % 128 || c.inter % 128)
    return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_create: hidden, heads*head_dim and inter must be multiples of 128");
  if (kvd % 16 || c.vocab % 16)
    return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_create: kv_heads*head_dim and vocab must be multiples of 16");
  return TI_OK;
}

// Decode-attention workspace: the largest need over the row counts that run the split kernel --
// decode batches up to max_batch and prompt chunks of up to 64 rows (ti_gemm_packed_rows; longer
// chunks run ti_attn_prefill / ti_attn_prefill_f8, no workspace), all chunk sizes when TI_ATTN_PREFILL=0.
size_t ws_bytes(const ti_engine* e) {
  const ti_engine_config& c = e->c;
  const int R = prefill_attn_on() ? std::min(e->rows_cap, std::max(c.max_batch, 64)) : e->rows_cap;
  size_t b = 0;
  for (int M = 1; M <= R; ++M) b = std::max(b, ti_attn_workspace_bytes(M, c.heads, c.head_dim, e->splits_for(M)));
  return b;
}

// Shared-prefix registration (ti_engine_share_prefix).  TI_SHARE_MIN: the shortest registered prefix whose
// batched steps take ti_attn_decode_shared; shorter ones keep the plain kernel.  1024: the smallest measured
// prefix at which 8 streams of the 7B shape win (22.6 -> 13.7 us; 256 keys 8.0 -> 10.4, 64 keys 4.4 -> 7.9); 64
// streams win from 64 keys on, the Llama-3-8B shape at 8 streams only from 1920 (profiles/shared_prefix_ab.txt).
#ifndef TI_SHARE_MIN_DEFAULT
#define TI_SHARE_MIN_DEFAULT 1024
#endif
int share_min_env() {
  const char* v = getenv("TI_SHARE_MIN");
  return v && atoi(v) > 0 ? atoi(v) : TI_SHARE_MIN_DEFAULT;
}
}  // namespace

namespace ti_eng {

// Forget the registration (an entry point is about to write a prefix row, or the caller asked): the graphs
// that bake the prefix length go with it.  Nothing happens -- nothing is enqueued -- without a registration.
int share_clear(ti_engine* e) {
  if (e->share_len == 0) return TI_OK;
  TI_TRY(drop_graphs(e));
  e->share_len = e->share_n = 0;
  e->share_tokens.clear();
  return TI_OK;
}
// May M streams starting at base[0 .. M) attend the registered prefix once for all?  Clears the registration
// first when one of them would write a prefix row of a registered slot.
int share_begin(ti_engine* e, int M, const int32_t* base, bool* use) {
  *use = false;
  if (e->share_len == 0) return TI_OK;
  bool below = false, all = true;
  for (int m = 0; m < M; ++m) {
    below = below || (m < e->share_n && base[m] < e->share_len);
    all = all && base[m] >= e->share_len;
  }
  if (below) return share_clear(e);
  *use = all && M >= 2 && M <= e->share_n && e->share_len >= e->share_min;
  return TI_OK;
}

// Penalties (ti_engine_set_penalties).  Slot m's state becomes the histogram of head[0 .. n_head) ++
// tail[0 .. n_tail): the registered prefix, when the stream continues it, and the prompt.
int pen_reset_slot(ti_engine* e, int m, const int32_t* head, int n_head, const int32_t* tail, int n_tail) {
  const int n = n_head + n_tail;
  if (n > e->c.max_seq) return ti_set_error(TI_ERR_ARG, "engine: a penalty context of %d tokens exceeds max_seq %d", n, e->c.max_seq);
  std::vector<int32_t> ctx((size_t)n);
  if (n_head) std::memcpy(ctx.data(), head, (size_t)n_head * 4);
  if (n_tail) std::memcpy(ctx.data() + n_head, tail, (size_t)n_tail * 4);
  TI_TRY(ti_memcpy_h2d(e->pen_ctx, ctx.data(), (size_t)n * 4, e->s));
  return ti_penalty_reset(&e->pen, e->c.vocab, m, e->pen_ctx, n, e->s);
}

// The penalty state, made by whoever penalises first (ti_engine_set_penalties, ti_engine_serve_requests); the
// buffers never move afterwards, so no graph has to go.
int pen_state_alloc(ti_engine* e) {
  if (e->pen.counts) return TI_OK;
  const ti_engine_config& c = e->c;
  TI_TRY(e->alloc_t(&e->pen.counts, (size_t)c.max_batch * c.vocab));
  TI_TRY(e->alloc_t(&e->pen.seen, (size_t)c.max_batch * c.vocab));
  TI_TRY(e->alloc_t(&e->pen.n_seen, (size_t)c.max_batch));
  TI_TRY(e->alloc_t(&e->pen_ctx, (size_t)c.max_seq));
  if (!e->pen_carry) TI_TRY(e->alloc_t(&e->pen_carry, (size_t)c.max_batch));   // (a guide may have made it)
  return TI_OK;
}

// The entry points that produce tokens without the sampled step graph cannot penalise.
int pen_refuse(const ti_engine* e, const char* fn) {
  if (!e->pen_active()) return TI_OK;
  return ti_set_error(TI_ERR_UNSUPPORTED, "%s: penalties are active (ti_engine_set_penalties); only ti_engine_generate_sampled "
                      "and ti_engine_serve_sampled apply them", fn);
}

}  // namespace ti_eng

extern "C" {

int ti_engine_create(const ti_engine_config* cfg, ti_engine** out) {
  if (!cfg || !out) return ti_set_error(TI_ERR_ARG, "ti_engine_create: null");
  *out = nullptr;
  TI_TRY(validate(*cfg));
  DeviceScope bind_(cfg->device);   // restores the caller's device after ti_init's hipSetDevice
  TI_TRY(ti_init(cfg->device));
  ti_engine* e = new ti_engine();
  e->c = *cfg;
  e->kv8 = !cfg->compat && (cfg->bits & TI_BITS_KV8) != 0;
  e->c.bits &= ~TI_BITS_KV8;   // from here on: the weight format
  const ti_engine_config& c = e->c;
  auto fail = [&](int rc) { delete e; return rc; };
  if (hipStreamCreateWithFlags(&e->s, hipStreamNonBlocking) != hipSuccess)
    return fail(ti_check_hip(hipErrorUnknown, "hipStreamCreate"));
  const int B = c.max_batch, H = c.hidden, I = c.inter, V = c.vocab;
  int rc = TI_OK;
  e->layer.resize((size_t)c.layers);
  if (c.compat) {
    for (auto& L : e->layer) {
      if ((rc = e->alloc_linear(L.gu, H, I)) || (rc = e->alloc_linear(L.down, I, H))) return fail(rc);
    }
    if ((rc = e->alloc_linear(e->lm, H, V))) return fail(rc);
    if ((rc = e->alloc_t(&e->tmp, (size_t)B * I))) return fail(rc);
  } else {
    const int qd = e->qd(), kvd = e->kvd(), hd = c.head_dim;
    e->kv_stride = (int64_t)c.kv_heads * c.max_seq * hd;
    for (auto& L : e->layer) {
      if ((rc = e->alloc_linear(L.qkv, H, qd + 2 * kvd)) || (rc = e->alloc_linear(L.o, qd, H)) ||
          (rc = e->alloc_linear(L.gu, H, 2 * I)) || (rc = e->alloc_linear(L.down, I, H)) ||
          (rc = e->alloc_t(&L.attn_norm, (size_t)H)) || (rc = e->alloc_t(&L.ffn_norm, (size_t)H)) ||
          (rc = e->alloc(reinterpret_cast<void**>(&L.kc), (size_t)B * e->kv_stride * e->kv_esz())) ||
          (rc = e->alloc(reinterpret_cast<void**>(&L.vc), (size_t)B * e->kv_stride * e->kv_esz())))
        return fail(rc);
      e->kv_bytes += (size_t)2 * B * e->kv_stride * e->kv_esz();
    }
    if ((rc = e->alloc_linear(e->lm, H, V)) || (rc = e->alloc_t(&e->emb, (size_t)V * H)) ||
        (rc = e->alloc_t(&e->out_norm, (size_t)H)) || (rc = e->alloc_t(&e->rope_cs, (size_t)c.max_seq * hd)))
      return fail(rc);
    e->weight_bytes += (size_t)V * H * 2 + (size_t)H * 4 * (2 * c.layers + 1);
    // RoPE table with the reference formula: freq_i = 1 / theta^(2i/d), angle = pos * freq_i.
    std::vector<float> cs((size_t)c.max_seq * hd), pv((size_t)c.max_seq);
    for (int p = 0; p < c.max_seq; ++p) pv[p] = (float)p;
    if ((rc = ti_rope_table(pv.data(), c.max_seq, hd, c.rope_theta, cs.data()))) return fail(rc);
    if ((rc = ti_memcpy_h2d(e->rope_cs, cs.data(), cs.size() * 4, e->s))) return fail(rc);
    if (const char* env = getenv("TI_ATTN_PART")) e->part_on = atoi(env) != 0;
    e->splits_max = e->splits_for(1);
    e->pf_rows = (c.bits & ~TI_BITS_G32) == 4 ? TI_GEMM_MAX_ROWS : 16;   // int4 (also group-32): the tile GEMM
    // (affine group-32 runs the fused kernel only: prompt chunks of its 16 rows)
    e->rows_cap = std::max(B, e->pf_rows);
    const int R = e->rows_cap;
    const int Rp = (R + 15) / 16 * 16;   // packed operands hold whole 16-row blocks
    if ((rc = e->alloc_t(&e->q, (size_t)R * qd)) || (rc = e->alloc_t(&e->attn, (size_t)Rp * qd)) ||
        (rc = e->alloc_t(&e->act, (size_t)Rp * I)) || (rc = e->alloc_t(&e->xn, (size_t)Rp * std::max(H, I))) ||
        (rc = e->alloc(reinterpret_cast<void**>(&e->ws), ws_bytes(e))) ||
        (rc = e->alloc_t(&e->pf_ones, (size_t)e->pf_rows)) || (rc = e->alloc_t(&e->pf_zero, (size_t)1)) ||
        (rc = e->alloc_t(&e->pf_base, (size_t)e->pf_rows)) || (rc = e->alloc_t(&e->fx, (size_t)H)) ||
        (rc = e->alloc_t(&e->ss, (size_t)256)) || (rc = e->alloc_t(&e->ss_rows, (size_t)4096 * TI_FOLD_SS_ROWS)) ||
        (rc = e->alloc_t(&e->part_o, ti_qkv_attn_part_o_elems(c.heads, hd, TI_ATTN_MAX_PART_SPLITS))) ||
        (rc = e->alloc_t(&e->part_ml, ti_qkv_attn_part_ml_elems(c.heads, hd, TI_ATTN_MAX_PART_SPLITS))) ||
        (rc = e->alloc(&e->qa_xchg, ti_qkv_attn_xchg_bytes(c.heads, TI_ATTN_MAX_PART_SPLITS))))
      return fail(rc);
    if (const char* env = getenv("TI_FOLD")) e->fold_on = atoi(env) != 0;
    if (const char* env = getenv("TI_QKV_ATTN")) e->qa_on = atoi(env) != 0;
    e->share_min = share_min_env();
    if ((c.bits & ~TI_BITS_G32) == 4) {   // batched rows and prompt chunks: split-K tile GEMM (TI_SPLITK_MB, 0 = off)
      const char* env = getenv("TI_SPLITK_MB");
      const size_t mb = env ? (size_t)std::max(0, atoi(env)) : 64;
      if (mb && (rc = e->alloc(&e->splitk_ws, mb << 20))) return fail(rc);
      e->splitk_bytes = mb << 20;
    }
    std::vector<int32_t> ones(e->pf_rows, 1);
    if ((rc = ti_memcpy_h2d(e->pf_ones, ones.data(), ones.size() * 4, e->s)) || (rc = ti_memset(e->pf_zero, 0, 4, e->s)))
      return fail(rc);
    std::vector<uint16_t*> tab;
    for (auto& L : e->layer) tab.push_back(L.kc);
    for (auto& L : e->layer) tab.push_back(L.vc);
    if ((rc = e->alloc_t(&e->kv_tab, tab.size())) || (rc = ti_memcpy_h2d(e->kv_tab, tab.data(), tab.size() * sizeof(void*), e->s)))
      return fail(rc);
  }
  const int R = std::max(B, e->rows_cap);
  if ((rc = e->alloc_t(&e->h, (size_t)R * H)) || (rc = e->alloc_t(&e->h_last, (size_t)B * H)) ||
      (rc = e->alloc_t(&e->logits, (size_t)B * V)) ||
      (rc = e->alloc_t(&e->argmax, (size_t)R * TI_ARGMAX_SLOTS)) || (rc = e->alloc_t(&e->pos, (size_t)R)) ||
      (rc = e->alloc_t(&e->base_pos, (size_t)B)) || (rc = e->alloc_t(&e->step_ctr, (size_t)1)) ||
      (rc = e->alloc_t(&e->n_in, (size_t)B)) || (rc = ensure_io(e, 8, 8)))
    return fail(rc);
  if (hipStreamSynchronize(e->s) != hipSuccess) return fail(ti_check_hip(hipErrorUnknown, "hipStreamSynchronize"));
  *out = e;
  return TI_OK;
}

int ti_engine_destroy(ti_engine* e) {
  if (e) {
    DeviceScope bind_(e);
    hipStreamSynchronize(e->s);
    delete e;
  }
  return TI_OK;
}

int ti_engine_get_stream(ti_engine* e, void** stream) {
  if (!e || !stream) return ti_set_error(TI_ERR_ARG, "ti_engine_get_stream: null");
  DeviceScope bind_(e);
  *stream = (void*)e->s;
  return TI_OK;
}

int ti_engine_memory(ti_engine* e, size_t* wb, size_t* kb) {
  if (!e) return ti_set_error(TI_ERR_ARG, "ti_engine_memory: null");
  DeviceScope bind_(e);
  if (wb) *wb = e->weight_bytes;
  if (kb) *kb = e->kv_bytes;
  return TI_OK;
}

int ti_engine_set_tensor(ti_engine* e, int slot, int layer, const float* data, int scale_mode) {
  if (!e || !data) return ti_set_error(TI_ERR_ARG, "ti_engine_set_tensor: null");
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  const int H = c.hidden, I = c.inter, V = c.vocab;
  const bool per_layer = slot <= TI_W_DOWN || slot == TI_V_ATTN_NORM || slot == TI_V_FFN_NORM;
  if (per_layer && (layer < 0 || layer >= c.layers))
    return ti_set_error(TI_ERR_ARG, "ti_engine_set_tensor: layer %d of %d", layer, c.layers);

  if (c.compat) {
    DevLinear* L = nullptr;
    size_t n = 0;
    switch (slot) {
      case TI_W_UP: L = &e->layer[layer].gu; n = (size_t)H * I; break;
      case TI_W_DOWN: L = &e->layer[layer].down; n = (size_t)I * H; break;
      case TI_W_LM_HEAD: L = &e->lm; n = (size_t)H * V; break;
      case TI_W_Q: case TI_W_K: case TI_W_V: case TI_E_EMBED: return TI_OK;  // unused by the compat path
      default: return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_set_tensor: slot %d not part of the compat model", slot);
    }
    return ti_memcpy_h2d(L->f32, data, n * 4, e->s);
  }

  if (slot == TI_V_ATTN_NORM || slot == TI_V_FFN_NORM || slot == TI_V_OUT_NORM) {
    float* dst = slot == TI_V_OUT_NORM ? e->out_norm
                                       : (slot == TI_V_ATTN_NORM ? e->layer[layer].attn_norm : e->layer[layer].ffn_norm);
    return ti_memcpy_h2d(dst, data, (size_t)H * 4, e->s);
  }
  if (slot == TI_E_EMBED) {
    std::vector<uint16_t> hb((size_t)V * H);
    for (size_t i = 0; i < hb.size(); ++i) hb[i] = host_half(data[i]);
    return ti_memcpy_h2d(e->emb, hb.data(), hb.size() * 2, e->s);
  }
  const int qd = e->qd(), kvd = e->kvd();
  DevLinear* L = nullptr;
  int K = 0, Nsrc = 0, map = TI_ROWS_CONCAT, off = 0;
  switch (slot) {
    case TI_W_Q: L = &e->layer[layer].qkv; K = H; Nsrc = qd; off = 0; break;
    case TI_W_K: L = &e->layer[layer].qkv; K = H; Nsrc = kvd; off = qd; break;
    case TI_W_V: L = &e->layer[layer].qkv; K = H; Nsrc = kvd; off = qd + kvd; break;
    case TI_W_O: L = &e->layer[layer].o; K = qd; Nsrc = H; break;
    case TI_W_GATE: L = &e->layer[layer].gu; K = H; Nsrc = I; map = TI_ROWS_INTERLEAVE8; off = 0; break;
    case TI_W_UP: L = &e->layer[layer].gu; K = H; Nsrc = I; map = TI_ROWS_INTERLEAVE8; off = 8; break;
    case TI_W_DOWN: L = &e->layer[layer].down; K = I; Nsrc = H; break;
    case TI_W_LM_HEAD: L = &e->lm; K = H; Nsrc = V; break;
    default: return ti_set_error(TI_ERR_ARG, "ti_engine_set_tensor: slot %d", slot);
  }
  // read-modify-write of the fused buffer: the packer only touches this part's rows
  const size_t tb = ti_wpack_tile_bytes(c.bits, L->K, L->N), sb = ti_wpack_scale_bytes(c.bits, L->K, L->N);
  std::vector<uint8_t> th(tb);
  std::vector<uint16_t> sh(sb / 2 + 1);
  TI_TRY(ti_memcpy_d2h(th.data(), L->tiles, tb, e->s));
  if (sb) TI_TRY(ti_memcpy_d2h(sh.data(), L->scales, sb, e->s));
  TI_TRY(ti_wpack_host(data, K, Nsrc, L->N, c.bits, scale_mode, map, off, th.data(), sb ? sh.data() : nullptr));
  TI_TRY(ti_memcpy_h2d(L->tiles, th.data(), tb, e->s));
  if (sb) TI_TRY(ti_memcpy_h2d(L->scales, sh.data(), sb, e->s));
  return TI_OK;
}

// Exact group-32 weights: Q4_0 / Q8_0 blocks (q int8, d) or, with m, Q4_1 blocks (q 0..15, d, m;
// TI_BITS_AFF engines), packed without re-quantization (ti_wpack_q_host / ti_wpack_q1_host).
static int set_tensor_blocks(ti_engine* e, int slot, int layer, const void* q, const uint16_t* d, const uint16_t* m) {
  const char* fn = m ? "ti_engine_set_tensor_q1" : "ti_engine_set_tensor_q";
  if (!e || !q || !d) return ti_set_error(TI_ERR_ARG, "%s: null", fn);
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  if (!(c.bits & TI_BITS_G32)) return ti_set_error(TI_ERR_ARG, "%s: engine bits %d lack TI_BITS_G32", fn, c.bits);
  if (((c.bits & TI_BITS_AFF) != 0) != (m != nullptr))
    return ti_set_error(TI_ERR_ARG, "%s: engine bits %d (%s blocks expected)", fn, c.bits,
                        (c.bits & TI_BITS_AFF) ? "affine Q4_1" : "Q4_0 / Q8_0");
  if (layer < 0 || (slot <= TI_W_DOWN && layer >= c.layers)) return ti_set_error(TI_ERR_ARG, "%s: layer %d", fn, layer);
  const int H = c.hidden, I = c.inter, V = c.vocab, qd = e->qd(), kvd = e->kvd();
  DevLinear* L = nullptr;
  int K = 0, Nsrc = 0, map = TI_ROWS_CONCAT, off = 0;
  switch (slot) {
    case TI_W_Q: L = &e->layer[layer].qkv; K = H; Nsrc = qd; off = 0; break;
    case TI_W_K: L = &e->layer[layer].qkv; K = H; Nsrc = kvd; off = qd; break;
    case TI_W_V: L = &e->layer[layer].qkv; K = H; Nsrc = kvd; off = qd + kvd; break;
    case TI_W_O: L = &e->layer[layer].o; K = qd; Nsrc = H; break;
    case TI_W_GATE: L = &e->layer[layer].gu; K = H; Nsrc = I; map = TI_ROWS_INTERLEAVE8; off = 0; break;
    case TI_W_UP: L = &e->layer[layer].gu; K = H; Nsrc = I; map = TI_ROWS_INTERLEAVE8; off = 8; break;
    case TI_W_DOWN: L = &e->layer[layer].down; K = I; Nsrc = H; break;
    case TI_W_LM_HEAD: L = &e->lm; K = H; Nsrc = V; break;
    default: return ti_set_error(TI_ERR_ARG, "%s: slot %d is not a linear weight", fn, slot);
  }
  const size_t tb = ti_wpack_tile_bytes(c.bits, L->K, L->N), sb = ti_wpack_scale_bytes(c.bits, L->K, L->N);
  std::vector<uint8_t> th(tb);
  std::vector<uint16_t> sh(sb / 2 + 1);
  TI_TRY(ti_memcpy_d2h(th.data(), L->tiles, tb, e->s));
  TI_TRY(ti_memcpy_d2h(sh.data(), L->scales, sb, e->s));
  if (m)
    TI_TRY(ti_wpack_q1_host(static_cast<const uint8_t*>(q), d, m, K, Nsrc, L->N, map, off, th.data(), sh.data()));
  else
    TI_TRY(ti_wpack_q_host(static_cast<const int8_t*>(q), d, K, Nsrc, L->N, c.bits, map, off, th.data(), sh.data()));
  TI_TRY(ti_memcpy_h2d(L->tiles, th.data(), tb, e->s));
  TI_TRY(ti_memcpy_h2d(L->scales, sh.data(), sb, e->s));
  return ti_stream_sync(e->s);
}

int ti_engine_set_tensor_q(ti_engine* e, int slot, int layer, const int8_t* q, const uint16_t* d) {
  return set_tensor_blocks(e, slot, layer, q, d, nullptr);
}

int ti_engine_set_tensor_q1(ti_engine* e, int slot, int layer, const uint8_t* q, const uint16_t* d, const uint16_t* m) {
  if (!m) return ti_set_error(TI_ERR_ARG, "ti_engine_set_tensor_q1: null");
  return set_tensor_blocks(e, slot, layer, q, d, m);
}

int ti_engine_synth(ti_engine* e, uint64_t seed, float norm_jitter) {
  if (!e) return ti_set_error(TI_ERR_ARG, "ti_engine_synth: null");
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  if (c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_synth: compat engines take the reference model");
  if (c.bits & TI_BITS_G32)
    return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_synth: group-32 engines take their weights from ti_engine_set_tensor[_q]");
  const int H = c.hidden, I = c.inter, V = c.vocab, qd = e->qd(), kvd = e->kvd(), b = c.bits;
  for (int l = 0; l < c.layers; ++l) {
    DevLayer& L = e->layer[l];
    const int nq = qd + 2 * kvd;
    TI_TRY(ti_wsynth_device(seed, tid_layer(l, TL_Q), H, qd, nq, b, TI_ROWS_CONCAT, 0, L.qkv.tiles, L.qkv.scales, e->s));
    TI_TRY(ti_wsynth_device(seed, tid_layer(l, TL_K), H, kvd, nq, b, TI_ROWS_CONCAT, qd, L.qkv.tiles, L.qkv.scales, e->s));
    TI_TRY(ti_wsynth_device(seed, tid_layer(l, TL_V), H, kvd, nq, b, TI_ROWS_CONCAT, qd + kvd, L.qkv.tiles, L.qkv.scales, e->s));
    TI_TRY(ti_wsynth_device(seed, tid_layer(l, TL_O), qd, H, H, b, TI_ROWS_CONCAT, 0, L.o.tiles, L.o.scales, e->s));
    TI_TRY(ti_wsynth_device(seed, tid_layer(l, TL_G), H, I, 2 * I, b, TI_ROWS_INTERLEAVE8, 0, L.gu.tiles, L.gu.scales, e->s));
    TI_TRY(ti_wsynth_device(seed, tid_layer(l, TL_U), H, I, 2 * I, b, TI_ROWS_INTERLEAVE8, 8, L.gu.tiles, L.gu.scales, e->s));
    TI_TRY(ti_wsynth_device(seed, tid_layer(l, TL_D), I, H, H, b, TI_ROWS_CONCAT, 0, L.down.tiles, L.down.scales, e->s));
    TI_TRY(ti_fill_uniform_f32(seed, tid_layer(l, TL_ATTN_NORM), (uint64_t)H, norm_jitter, 1.0f, L.attn_norm, e->s));
    TI_TRY(ti_fill_uniform_f32(seed, tid_layer(l, TL_FFN_NORM), (uint64_t)H, norm_jitter, 1.0f, L.ffn_norm, e->s));
  }
  TI_TRY(ti_wsynth_device(seed, kTidLmHead, H, V, V, b, TI_ROWS_CONCAT, 0, e->lm.tiles, e->lm.scales, e->s));
  TI_TRY(ti_fill_uniform_f32(seed, kTidOutNorm, (uint64_t)H, norm_jitter, 1.0f, e->out_norm, e->s));
  TI_TRY(ti_fill_uniform_f16(seed, kTidEmb, (uint64_t)V * H, 0.02f, e->emb, e->s));
  return ti_stream_sync(e->s);
}

int ti_engine_fill_kv(ti_engine* e, int stream, int n, uint64_t seed) {
  if (!e || e->c.compat) return ti_set_error(TI_ERR_ARG, "ti_engine_fill_kv: no KV cache");
  DeviceScope bind_(e);
  if (stream < 0 || stream >= e->c.max_batch || n < 0 || n > e->c.max_seq)
    return ti_set_error(TI_ERR_ARG, "ti_engine_fill_kv: stream %d n %d", stream, n);
  if (stream < e->share_n && n > 0) TI_TRY(share_clear(e));   // (writes the slot's rows from 0)
  for (int l = 0; l < e->c.layers; ++l) {
    DevLayer& L = e->layer[l];
    uint16_t* caches[2] = {e->kv_at(L.kc, (size_t)stream * e->kv_stride), e->kv_at(L.vc, (size_t)stream * e->kv_stride)};
    for (int v = 0; v < 2; ++v) {
      if (e->kv8)
        TI_TRY(ti_fill_kv_uniform_f8(seed, tid_kv(l, v), n, e->c.kv_heads, e->c.head_dim, e->c.max_seq,
                                     reinterpret_cast<uint8_t*>(caches[v]), e->s));
      else
        TI_TRY(ti_fill_kv_uniform(seed, tid_kv(l, v), n, e->c.kv_heads, e->c.head_dim, e->c.max_seq, caches[v], e->s));
    }
  }
  return ti_stream_sync(e->s);
}

int ti_engine_read_kv(ti_engine* e, int layer, int stream, int which, int pos0, int n, void* out) {
  if (!e || e->c.compat) return ti_set_error(TI_ERR_ARG, "ti_engine_read_kv: no KV cache");
  const ti_engine_config& c = e->c;
  if (!out || layer < 0 || layer >= c.layers || stream < 0 || stream >= c.max_batch || (which != 0 && which != 1) ||
      pos0 < 0 || n < 1 || pos0 > c.max_seq - n)
    return ti_set_error(TI_ERR_ARG, "ti_engine_read_kv: layer %d stream %d which %d pos0 %d n %d", layer, stream, which,
                        pos0, n);
  DeviceScope bind_(e);
  const DevLayer& L = e->layer[(size_t)layer];
  const size_t esz = e->kv_esz(), row = (size_t)n * c.head_dim * esz;
  const char* base = reinterpret_cast<const char*>(which ? L.vc : L.kc) + (size_t)stream * e->kv_stride * esz;
  E_CHECK(hipMemcpy2DAsync(out, row, base + (size_t)pos0 * c.head_dim * esz, (size_t)c.max_seq * c.head_dim * esz, row,
                           (size_t)c.kv_heads, hipMemcpyDeviceToHost, e->s),
          "hipMemcpy2DAsync(read_kv)");
  return ti_stream_sync(e->s);
}

int ti_engine_share_prefix(ti_engine* e, const int32_t* tokens, int n, int n_streams) {
  const char* fn = "ti_engine_share_prefix";
  if (!e || (!tokens && n > 0)) return ti_set_error(TI_ERR_ARG, "%s: null", fn);
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  if (c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "%s: compat engine", fn);
  if (e->kv8) return ti_set_error(TI_ERR_UNSUPPORTED, "%s: TI_BITS_KV8 engine (no e4m3 shared-prefix attention)", fn);
  if (n < 0 || n >= c.max_seq) return ti_set_error(TI_ERR_ARG, "%s: n %d outside [0, max_seq %d)", fn, n, c.max_seq);
  if (n == 0) return share_clear(e);
  if (n_streams < 2 || n_streams > c.max_batch)
    return ti_set_error(TI_ERR_ARG, "%s: n_streams %d outside [2, max_batch %d]", fn, n_streams, c.max_batch);
  for (int i = 0; i < n; ++i)
    if (tokens[i] < 0 || tokens[i] >= c.vocab)
      return ti_set_error(TI_ERR_ARG, "%s: token %d at %d outside [0, vocab %d)", fn, tokens[i], i, c.vocab);
  // the live registration again (the system-prompt cache across calls): nothing to do
  if (n == e->share_len && n_streams == e->share_n && std::equal(tokens, tokens + n, e->share_tokens.begin())) return TI_OK;
  TI_TRY(share_clear(e));
  if (!e->share_ws) {
    void* w = nullptr;
    TI_TRY(e->alloc(&w, ti_attn_shared_workspace_bytes(c.max_batch, c.heads, c.head_dim, 32)));
    e->share_ws = static_cast<float*>(w);
  }
  TI_TRY(ensure_io(e, n, 1));
  TI_TRY(ti_memcpy_h2d(e->in_tokens, tokens, (size_t)n * 4, e->s));   // slot 0's token row
  TI_TRY(prefill_tokens(e, 0, n, 0));
  for (int d = 1; d < n_streams; ++d) TI_TRY(fork_slot(e, 0, d, n));
  TI_TRY(ti_stream_sync(e->s));
  e->share_tokens.assign(tokens, tokens + n);
  e->share_len = n;
  e->share_n = n_streams;
  return TI_OK;
}

int ti_engine_shared_prefix(ti_engine* e, int* len, int* n_streams) {
  if (!e) return ti_set_error(TI_ERR_ARG, "ti_engine_shared_prefix: null");
  if (len) *len = e->share_len;
  if (n_streams) *n_streams = e->share_n;
  return TI_OK;
}

int ti_engine_set_stop(ti_engine* e, int32_t token) {
  if (!e || token < -1 || token >= e->c.vocab) return ti_set_error(TI_ERR_ARG, "ti_engine_set_stop: token %d", token);
  e->stop_token = token;
  return TI_OK;
}

int ti_engine_set_penalties(ti_engine* e, float repetition, float presence, float frequency) {
  const char* fn = "ti_engine_set_penalties";
  if (!e) return ti_set_error(TI_ERR_ARG, "%s: null", fn);
  if (!(std::isfinite(repetition) && repetition > 0.0f) || !std::isfinite(presence) || !std::isfinite(frequency))
    return ti_set_error(TI_ERR_ARG, "%s: repetition %g (finite, > 0), presence %g, frequency %g (finite)", fn,
                        (double)repetition, (double)presence, (double)frequency);
  if (e->c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "%s: compat engine", fn);
  if (repetition == e->pen_rep && presence == e->pen_pres && frequency == e->pen_freq) return TI_OK;
  DeviceScope bind_(e);
  TI_TRY(drop_graphs(e));   // the step graphs bake the values in
  const bool on = repetition != 1.0f || presence != 0.0f || frequency != 0.0f;
  if (on) TI_TRY(pen_state_alloc(e));
  e->pen_rep = repetition;
  e->pen_pres = presence;
  e->pen_freq = frequency;
  return TI_OK;
}

int ti_engine_get_penalties(ti_engine* e, float* repetition, float* presence, float* frequency) {
  if (!e) return ti_set_error(TI_ERR_ARG, "ti_engine_get_penalties: null");
  if (repetition) *repetition = e->pen_rep;
  if (presence) *presence = e->pen_pres;
  if (frequency) *frequency = e->pen_freq;
  return TI_OK;
}

int ti_engine_counters(ti_engine* e, uint64_t* decode_steps, uint64_t* prefill_chunks) {
  if (!e) return ti_set_error(TI_ERR_ARG, "ti_engine_counters: null");
  if (decode_steps) *decode_steps = e->n_decode_steps;
  if (prefill_chunks) *prefill_chunks = e->n_prefill_chunks;
  return TI_OK;
}

int ti_engine_graph_counters(ti_engine* e, uint64_t* captured, uint64_t* dropped) {
  if (!e) return ti_set_error(TI_ERR_ARG, "ti_engine_graph_counters: null");
  if (captured) *captured = e->n_graphs_captured;
  if (dropped) *dropped = e->n_graphs_dropped;
  return TI_OK;
}

int ti_engine_prefill_attn_name(ti_engine* e, int rows, char* buf, int len) {
  if (!e || !buf || rows < 1 || len < 1) return ti_set_error(TI_ERR_ARG, "ti_engine_prefill_attn_name: null engine / buffer, rows or len < 1");
  if (e->c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_prefill_attn_name: compat engine");
  static const char* const names[3][2] = {{"ti_attn_prefill", "ti_attn_prefill_f8"},
                                          {"ti_attn_decode", "ti_attn_decode_f8"},
                                          {"ti_attn_decode_packed", "ti_attn_decode_packed_f8"}};
  snprintf(buf, (size_t)len, "%s", names[prefill_attn_route(e, rows)][e->kv8 ? 1 : 0]);
  return TI_OK;
}

int ti_engine_set_prefill(ti_engine* e, int rows) {
  if (!e || e->c.compat || rows < 0 || rows > e->rows_cap || (rows > 0 && rows > ((e->c.bits & ~TI_BITS_G32) == 4 ? TI_GEMM_MAX_ROWS : 16)))
    return ti_set_error(TI_ERR_ARG, "ti_engine_set_prefill: rows %d", rows);
  DeviceScope bind_(e);
  e->pf_rows = rows;
  return TI_OK;
}

int ti_engine_set_fold(ti_engine* e, int on, int* active) {
  if (!e) return ti_set_error(TI_ERR_ARG, "ti_engine_set_fold: null");
  DeviceScope bind_(e);
  if (on >= 0 && ((on != 0) != e->fold_on || (on != 0) != e->part_on)) {
    TI_TRY(drop_graphs(e));   // captured step graphs bake the setting in
    e->fold_on = e->part_on = on != 0;
  }
  if (active) *active = fold_usable(e, 1) ? 1 : 0;
  return TI_OK;
}

int ti_engine_set_qkv_attn(ti_engine* e, int on, int* active) {
  if (!e) return ti_set_error(TI_ERR_ARG, "ti_engine_set_qkv_attn: null");
  DeviceScope bind_(e);
  if (on >= 0 && (on != 0) != e->qa_on) {
    TI_TRY(drop_graphs(e));   // captured step graphs bake the setting in
    e->qa_on = on != 0;
  }
  if (active) *active = qa_usable(e, 1) ? 1 : 0;
  return TI_OK;
}

}  // extern "C"
