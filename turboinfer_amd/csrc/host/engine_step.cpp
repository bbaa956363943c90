// engine_step.cpp -- what a decode step and a prompt chunk launch (enqueue_step, enqueue_prefill), the epilogues
// and the step plan they are built from, and the cache of their captured graphs.
#include "engine_impl.hpp"

namespace ti_eng {

// Rows of the batched-rows kernel (int4, M > 16) take their fp16 operands in fragment order
// (TI_X_F16_PACKED): the rms_norm prep, the attention output and the SiLU*up output are written
// that way, so every operand load of the kernel is one contiguous KiB per wave.
bool packed_rows(const ti_engine* e, int M) { return ti_gemm_packed_rows(e->c.bits, M) != 0; }

// One projection for rows [0, M): the fused kernel in chunks of the rows its LDS image
// holds, or -- int4, when the rows do not fit -- rms_norm into fp16 rows once (e->xn) and
// the batched-rows kernel in chunks of TI_GEMM_MAX_ROWS.  Graph-capturable.
int gemm_rows(ti_engine* e, const DevLinear& W, int M, const void* x, int x_kind, int ldx, const float* nw,
              const ti_epilogue& epi, size_t out_elem, bool last_gets_ctr) {
  const ti_engine_config& c = e->c;
  int rows = ti_gemm_max_rows(c.bits, x_kind, W.N, W.K);
  if (x_kind == TI_X_F32_RMSNORM && ti_gemm_packed_rows_for(c.bits, M, W.N, W.K) && e->xn) {
    TI_TRY(ti_rmsnorm_f16_packed(static_cast<const float*>(x), ldx, nw, c.eps, e->xn, M, W.K, e->s));
    x = e->xn;
    x_kind = TI_X_F16_PACKED;
    ldx = W.K;
    rows = ti_gemm_max_rows(c.bits, x_kind, W.N, W.K);
  } else if (x_kind == TI_X_F32_RMSNORM && rows < M && (c.bits & ~TI_BITS_G32) == 4 && e->xn) {
    TI_TRY(ti_rmsnorm_f16(static_cast<const float*>(x), ldx, nw, c.eps, e->xn, W.K, M, W.K, e->s));
    x = e->xn;
    x_kind = TI_X_F16;
    ldx = W.K;
    rows = ti_gemm_max_rows(c.bits, x_kind, W.N, W.K);
  }
  if (rows < 1) return ti_set_error(TI_ERR_UNSUPPORTED, "engine: no GEMM kernel for N=%d K=%d", W.N, W.K);
  const size_t x_elem = x_kind == TI_X_F16 || x_kind == TI_X_F16_FOLDED || x_kind == TI_X_F16_PACKED ? 2 : 4;
  for (int m0 = 0; m0 < M; m0 += rows) {
    const int mm = std::min(rows, M - m0);
    ti_epilogue ep = epi;
    ep.out = static_cast<char*>(epi.out) + (size_t)m0 * epi.ldo * out_elem;
    if (ep.pos) ep.pos += m0;
    if (ep.k_cache) ep.k_cache = e->kv_at(ep.k_cache, (size_t)m0 * ep.kv_stream_stride);
    if (ep.v_cache) ep.v_cache = e->kv_at(ep.v_cache, (size_t)m0 * ep.kv_stream_stride);
    if (ep.k_cache) ep.kv_fp8 = e->kv8 ? 1 : 0;   // every QKV launch of a TI_BITS_KV8 engine
    if (ep.argmax) ep.argmax += (size_t)m0 * TI_ARGMAX_SLOTS;
    if (!(last_gets_ctr && m0 + mm >= M)) ep.step_ctr = nullptr;
    ep.splitk_ws = e->splitk_ws;
    ep.splitk_bytes = (int64_t)e->splitk_bytes;
    const void* xm = static_cast<const char*>(x) + (size_t)m0 * ldx * x_elem;
    TI_TRY(ti_gemm_wq_a16(W.tiles, W.scales, c.bits, xm, x_kind, ldx, nw, c.eps, mm, W.N, W.K, &ep, e->s));
  }
  return TI_OK;
}

// The decode attention over the engine's caches, in their element type.
int attn_merged(ti_engine* e, bool packed, const uint16_t* kc, const uint16_t* vc, int64_t stride, int M, int splits) {
  const ti_engine_config& c = e->c;
  if (e->kv8)
    return (packed ? ti_attn_decode_packed_f8 : ti_attn_decode_f8)(
        e->q, reinterpret_cast<const uint8_t*>(kc), reinterpret_cast<const uint8_t*>(vc), stride, c.max_seq, e->pos, M,
        c.heads, c.kv_heads, c.head_dim, splits, e->ws, e->attn, e->s);
  return (packed ? ti_attn_decode_packed : ti_attn_decode)(e->q, kc, vc, stride, c.max_seq, e->pos, M, c.heads,
                                                            c.kv_heads, c.head_dim, splits, e->ws, e->attn, e->s);
}
int attn_partials(ti_engine* e, const uint16_t* kc, const uint16_t* vc, int M, int splits) {
  const ti_engine_config& c = e->c;
  if (e->kv8)
    return ti_attn_decode_partials_f8(e->q, reinterpret_cast<const uint8_t*>(kc), reinterpret_cast<const uint8_t*>(vc),
                                      e->kv_stride, c.max_seq, e->pos, M, c.heads, c.kv_heads, c.head_dim, splits,
                                      e->part_o, e->part_ml, e->s);
  return ti_attn_decode_partials(e->q, kc, vc, e->kv_stride, c.max_seq, e->pos, M, c.heads, c.kv_heads, c.head_dim,
                                 splits, e->part_o, e->part_ml, e->s);
}

// Splits of the prefix per (16 columns, kv-head), TI_SHARE_SPLITS sets them: about 512 waves (two per CU), at most
// 8 splits, at least 4 key blocks per split -- the fastest of 1 .. 32 splits at 8 and 64 streams of the 7B and
// the Llama-3-8B shape with 1024 and 1920 prefix keys (8, 4, 8, 4), the fastest at 64 keys and within 8 % of it at 256
// (profiles/shared_prefix_ab.txt; more, shorter splits lose to the partials they write and the merge reads)
static int share_splits(const ti_engine* e, int M) {
  const ti_engine_config& c = e->c;
  const char* v = getenv("TI_SHARE_SPLITS");
  const int nkb = (e->share_len + 15) / 16, blocks = (M * (c.heads / c.kv_heads) + 15) / 16 * c.kv_heads;
  if (v && atoi(v) > 0) return std::min(atoi(v), std::min(32, nkb));
  return std::max(1, std::min((512 + blocks - 1) / blocks, std::min(8, nkb / 4)));
}

// n steps of M streams from the current device state: the replayed step graph.
int run_steps(ti_engine* e, int M, StepMode mode, int n) {
  if (n <= 0) return TI_OK;
  hipGraphExec_t g = nullptr;
  TI_TRY(get_graph(e, M, mode, &g));
  for (int s = 0; s < n; ++s) E_CHECK(hipGraphLaunch(g, e->s), "hipGraphLaunch");
  e->n_decode_steps += (uint64_t)n;
  return TI_OK;
}

// The folded rms_norm hand-off applies to single-stream steps whose producers (O, down) run on
// the fused kernel with at most 256 workgroups.
bool fold_usable(ti_engine* e, int M) {
  const ti_engine_config& c = e->c;
  // (group-32 weights: their launch grid is not ti_gemm_grid's, so no fold hand-off)
  if (!e->fold_on || M != 1 || c.compat || !e->fx || (c.bits & TI_BITS_G32)) return false;
  const int H = c.hidden, I = c.inter, qd = e->qd();
  const int g_o = ti_gemm_grid(1, H, qd), g_d = ti_gemm_grid(1, H, I);
  return g_o > 0 && g_o <= 256 && g_d > 0 && g_d <= 256 && ti_gemm_max_rows(c.bits, TI_X_F16, H, qd) >= 1;
}

// The batched fold: 17..64 int4 rows on the batched-rows kernels (packed operands), the O / down
// producers' column groups within the partial buffer.
static bool bfold_usable(ti_engine* e, int M) {
  const ti_engine_config& c = e->c;
  if (!e->fold_on || c.compat || c.bits != 4 || M <= 16 || M > TI_FOLD_SS_ROWS || !packed_rows(e, M) || !e->ss_rows)
    return false;
  const int po = ti_gemm_fold_partials(c.bits, M, c.hidden, e->qd()), pd = ti_gemm_fold_partials(c.bits, M, c.hidden, c.inter);
  return po >= 1 && po <= 4096 && pd >= 1 && pd <= 4096;
}

// Split partials merged by the O projection: one stream, 2..8 splits, heads*head_dim <= 4096.
static bool part_usable(ti_engine* e, int M) {
  const ti_engine_config& c = e->c;
  const int sp = e->splits_for(M);
  return e->part_on && e->part_o && M == 1 && !c.compat && sp >= 2 && sp <= TI_ATTN_MAX_PART_SPLITS &&
         e->qd() <= 4096;
}

// The fused launch's bounded waits: after the stream's work, a set error word means a workgroup's q part or
// new key never came (wrong results for that step) -- reported, and the exchange zeroed so the generations
// agree again.  One 4-byte read on the engine's stream (synchronous).
int qa_fault_check(ti_engine* e) {
  if (!e->qa_xchg || !qa_usable(e, 1)) return TI_OK;   // (only engines whose 1-stream steps take the launch)
  const ti_engine_config& c = e->c;
  const size_t off = ti_qkv_attn_error_offset(c.heads, e->splits_for(1));
  if (off + 8 > ti_qkv_attn_xchg_bytes(c.heads, TI_ATTN_MAX_PART_SPLITS))
    return ti_set_error(TI_ERR_ARG, "engine: exchange error word outside the buffer");
  uint32_t err[2] = {0u, 0u};
  TI_TRY(ti_memcpy_d2h(err, static_cast<char*>(e->qa_xchg) + off, sizeof(err), e->s));
  if (!err[0] && !err[1]) return TI_OK;
  TI_TRY(ti_memset(e->qa_xchg, 0, ti_qkv_attn_xchg_bytes(c.heads, TI_ATTN_MAX_PART_SPLITS), e->s));
  TI_TRY(ti_stream_sync(e->s));
  return ti_set_error(TI_ERR_HIP, "engine: the fused QKV + attention launch's exchange timed out (a workgroup's q "
                      "part or the new key never arrived); results of the last call are wrong, exchange reset");
}

// QKV + attention in one launch (ti_qkv_attn_partials): one stream with the fold and split partials,
// int8 / int4 group-128 weights, head_dim 64 GQA (TinyLlama-1.1B) or head_dim 128 MHA (Llama-2-7B).
bool qa_usable(ti_engine* e, int M) {
  const ti_engine_config& c = e->c;
  // (a TI_BITS_KV8 engine: off -- the launch attends the step's own key unquantised, a different function)
  if (!e->qa_on || e->kv8 || M != 1 || !fold_usable(e, M) || !part_usable(e, M)) return false;
  // all heads x splits workgroups resident at once for the in-launch q exchange
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return false;
  const int sp = e->splits_for(M);
  return c.heads * sp <= cus && ti_gemm_grid(1, c.hidden, c.inter) <= 256 &&
         ti_qkv_attn_supported(c.bits, c.hidden, c.heads, c.kv_heads, c.head_dim, sp);
}

StepPlan plan_step(ti_engine* e, int M) {
  StepPlan p{};
  p.M = M;
  p.fold = fold_usable(e, M);
  p.bfold = !p.fold && bfold_usable(e, M);
  p.part = part_usable(e, M);
  p.qa = qa_usable(e, M);
  p.packed = packed_rows(e, M);
  p.splits = e->splits_for(M);
  return p;
}

// The fold's producer side (a RESID epilogue): w the next norm's weight, n_next the output width of the call
// that consumes the fold.
void fold_into(const ti_engine* e, const StepPlan& p, ti_epilogue& ep, const float* w, int n_next) {
  if (!p.fold && !p.bfold) return;
  ep.fold_w = w;
  ep.fold_x = p.fold ? e->fx : e->xn;
  ep.fold_ss = p.fold ? e->ss : e->ss_rows;
  if (p.bfold) ep.fold_packed = ti_gemm_packed_rows_for(e->c.bits, p.M, n_next, e->c.hidden);
}

// The fold's consumer side, a projection of output width n behind an rms_norm.  n_ss: partials the last producer
// wrote (one stream); bn_ss: partials per row the last batched producer wrote (0: none yet, rms_norm prep).
void norm_in(const ti_engine* e, const StepPlan& p, int n_ss, int bn_ss, const void*& x, int& xk, int& ldx,
             const float*& nw, ti_epilogue& ep, int n) {
  if (!p.fold && !(p.bfold && bn_ss > 0)) return;
  x = p.fold ? e->fx : e->xn;
  if (p.fold) xk = TI_X_F16_FOLDED;
  else xk = ti_gemm_packed_rows_for(e->c.bits, p.M, n, e->c.hidden) ? TI_X_F16_PACKED : TI_X_F16;
  ldx = e->c.hidden;
  nw = nullptr;
  ep.ss_in = p.fold ? e->ss : e->ss_rows;
  ep.n_ss = p.fold ? n_ss : bn_ss;
}

// ti_step_begin's arguments for M rows fed by the device loop's buffers (enqueue_prefill: its own token feed).
ti_step_args step_args(const ti_engine* e, int M) {
  ti_step_args sa{};
  sa.emb = e->emb;
  sa.h = e->h;
  sa.hidden = e->c.hidden;
  sa.M = M;
  sa.vocab = e->c.vocab;
  sa.in_stride = e->in_cap;
  sa.out_stride = e->out_cap;
  sa.placeholder_first = -1;
  sa.in_tokens = e->in_tokens;
  sa.n_in = e->n_in;
  sa.argmax = e->argmax;
  sa.out_tokens = e->out_tokens;
  sa.pos = e->pos;
  sa.base_pos = e->base_pos;
  sa.step_ctr = e->step_ctr;
  return sa;
}

// The projections' epilogues: QKV (RoPE, K / V appended at e->pos into kc / vc, streams stream_stride elements
// apart), the residual add into h (O, down), SiLU * up into act, the logits with the greedy argmax keys.
ti_epilogue qkv_epilogue(const ti_engine* e, uint16_t* kc, uint16_t* vc, int64_t stream_stride) {
  ti_epilogue ep{};
  ep.kind = TI_EPI_QKV_ROPE_KV;
  ep.ldo = e->qd();
  ep.out = e->q;
  ep.q_dim = e->qd();
  ep.kv_dim = e->kvd();
  ep.head_dim = e->c.head_dim;
  ep.max_seq = e->c.max_seq;
  ep.pos = e->pos;
  ep.rope_cs = e->rope_cs;
  ep.k_cache = kc;
  ep.v_cache = vc;
  ep.kv_stream_stride = stream_stride;
  return ep;
}
ti_epilogue resid_epilogue(const ti_engine* e) {
  ti_epilogue ep{};
  ep.kind = TI_EPI_RESID_F32;
  ep.ldo = e->c.hidden;
  ep.out = e->h;
  return ep;
}
ti_epilogue silu_epilogue(const ti_engine* e, bool packed) {
  ti_epilogue ep{};
  ep.kind = TI_EPI_SILU_MUL_F16;
  ep.ldo = e->c.inter;
  ep.out = e->act;
  ep.out_packed = packed;
  return ep;
}
ti_epilogue logits_epilogue(const ti_engine* e, float* out, bool argmax) {
  ti_epilogue ep{};
  ep.kind = argmax ? TI_EPI_LOGITS_ARGMAX : TI_EPI_STORE_F32;
  ep.ldo = e->c.vocab;
  ep.out = out;
  if (argmax) ep.argmax = e->argmax;
  return ep;
}

// One decode step for streams [0, M) on e->s.  Graph-capturable (no host sync / alloc).  Besides its arguments it
// reads only what a change of drops the graphs: buffers, samp_t / k / p, the pen_* values, share_len, the settings.
int enqueue_step(ti_engine* e, int M, StepMode mode) {
  const ti_engine_config& c = e->c;
  ti_step_args sa = step_args(e, M);
  const int H = c.hidden, qd = e->qd(), I = c.inter, V = c.vocab;
  const StepPlan p = plan_step(e, M);
  const bool pk = p.packed;
  int bn_ss = 0;   // partials per row the last batched producer wrote (0: none yet, rms_norm prep)
  auto next_norm = [&](int l) -> const float* { return l < c.layers ? e->layer[l].attn_norm : e->out_norm; };
  auto next_n = [&](int l) -> int { return l < c.layers ? e->layer[l].qkv.N : e->lm.N; };
  if (p.fold) {
    sa.fold_w = next_norm(0);
    sa.fold_x = e->fx;
    sa.fold_ss = e->ss;
  }
  stamp_tag(TI_STAMP_TAG_BEGIN);
  TI_TRY(ti_step_begin(&sa, e->s));
  int n_ss = 1;   // partials the last producer wrote (step_begin: one)

  auto gemm = [&](const DevLinear& W, const void* x, int x_kind, int ldx, const float* nw, ti_epilogue epi,
                  size_t out_elem, bool last_gets_ctr) -> int {
    if (x_kind == TI_X_F32_RMSNORM) norm_in(e, p, n_ss, bn_ss, x, x_kind, ldx, nw, epi, W.N);
    TI_TRY(gemm_rows(e, W, M, x, x_kind, ldx, nw, epi, out_elem, last_gets_ctr));
    if (epi.fold_x && p.fold) n_ss = ti_gemm_grid(M, W.N, W.K);
    if (epi.fold_x && p.bfold) bn_ss = ti_gemm_fold_partials(c.bits, M, W.N, W.K);
    return TI_OK;
  };

  for (int l = 0; l < c.layers; ++l) {
    DevLayer& L = e->layer[l];
    const ti_epilogue ep = qkv_epilogue(e, L.kc, L.vc, e->kv_stride);
    ti_epilogue eo = resid_epilogue(e);
    fold_into(e, p, eo, L.ffn_norm, L.gu.N);
    if (p.qa || p.part) {   // the O projection merges the attention's splits while staging its input
      stamp_tag(TI_STAMP_TAG_QKV);
      if (p.qa) {   // QKV + attention in one launch
        TI_TRY(ti_qkv_attn_partials(L.qkv.tiles, L.qkv.scales, c.bits, e->fx, e->ss, n_ss, c.eps, e->rope_cs, e->pos,
                                    L.kc, L.vc, c.max_seq, H, c.heads, c.kv_heads, c.head_dim, p.splits, e->part_o,
                                    e->part_ml, e->qa_xchg, e->s));
      } else {
        TI_TRY(gemm(L.qkv, e->h, TI_X_F32_RMSNORM, H, L.attn_norm, ep, 4, false));
        stamp_tag(TI_STAMP_TAG_ATTN);
        TI_TRY(attn_partials(e, L.kc, L.vc, M, p.splits));
      }
      eo.ss_in = e->part_ml;
      eo.n_ss = p.splits;
      eo.head_dim = c.head_dim;
      stamp_tag(TI_STAMP_TAG_O);
      TI_TRY(gemm(L.o, e->part_o, TI_X_ATTN_SPLITS, qd, nullptr, eo, 4, false));
    } else {
      stamp_tag(TI_STAMP_TAG_QKV);
      TI_TRY(gemm(L.qkv, e->h, TI_X_F32_RMSNORM, H, L.attn_norm, ep, 4, false));
      stamp_tag(TI_STAMP_TAG_ATTN);
      if (mode.shared)   // the registered prefix from slot 0 once for all streams, then each stream's own keys
        TI_TRY(ti_attn_decode_shared(e->q, L.kc, L.vc, e->kv_stride, c.max_seq, e->pos, M, c.heads, c.kv_heads, c.head_dim,
                                     e->share_len, share_splits(e, M), pk ? 1 : 0, e->share_ws, e->attn, e->s));
      else
        TI_TRY(attn_merged(e, pk, L.kc, L.vc, e->kv_stride, M, p.splits));
      stamp_tag(TI_STAMP_TAG_O);
      TI_TRY(gemm(L.o, e->attn, pk ? TI_X_F16_PACKED : TI_X_F16, qd, nullptr, eo, 4, false));
    }

    stamp_tag(TI_STAMP_TAG_GATE_UP);
    TI_TRY(gemm(L.gu, e->h, TI_X_F32_RMSNORM, H, L.ffn_norm, silu_epilogue(e, pk), 2, false));

    ti_epilogue ed = resid_epilogue(e);
    fold_into(e, p, ed, next_norm(l + 1), next_n(l + 1));
    stamp_tag(TI_STAMP_TAG_DOWN);
    TI_TRY(gemm(L.down, e->act, pk ? TI_X_F16_PACKED : TI_X_F16, I, nullptr, ed, 4, false));
  }
  ti_epilogue el = logits_epilogue(e, e->logits);
  el.step_ctr = e->step_ctr;
  el.advance = mode.advance;
  stamp_tag(TI_STAMP_TAG_LM_HEAD);
  TI_TRY(gemm(e->lm, e->h, TI_X_F32_RMSNORM, H, e->out_norm, el, 4, true));
  stamp_tag(TI_STAMP_TAG_OTHER);
  // (rows mode: the values are each row's own in e->row_params, the engine-wide ones do not apply)
  if (mode.sampled && (mode.rows ? mode.rows_pen : e->pen_active())) {   // the stream's context penalises the row the sampler is about to read
    ti_penalty_args pa{};
    pa.logits = e->logits;
    pa.ldl = V;
    pa.M = M;
    pa.V = V;
    pa.state = e->pen;
    pa.repetition = e->pen_rep;
    pa.presence = e->pen_pres;
    pa.frequency = e->pen_freq;
    pa.draw_stride = e->draw_cap;
    pa.advance = mode.advance;
    pa.step_ctr = e->step_ctr;
    pa.n_in = e->n_in;
    pa.out_tokens = e->out_tokens;
    pa.out_stride = e->out_cap;
    pa.carry = mode.carry ? e->pen_carry : nullptr;
    TI_TRY(mode.rows ? ti_penalty_step_rows(&pa, e->row_params, e->s) : ti_penalty_step(&pa, e->s));
  }
  // the stream's automaton state masks the row (-inf survives the penalties); rows_guide: each row's own library guide
  if (mode.sampled && (mode.rows_guide || e->guide_active())) TI_TRY(guide_enqueue(e, M, mode));
  if (mode.sampled && mode.rows)   // each row's temperature / top_k / top_p from the table; one instance for all rows
    TI_TRY(ti_sample_step_rows(e->logits, V, M, V, e->row_params, mode.rows_big ? V : std::min(V, TI_SAMPLE_MAX_K), e->draws,
                               e->draw_cap, e->step_ctr, mode.advance, e->n_in, e->argmax, e->lps, e->samp_ws, e->s));
  else if (mode.sampled)   // sample_next_token on the device; its key feeds the token back (ti_hip.h)
    TI_TRY(ti_sample_step_ws(e->logits, V, M, V, e->samp_t, e->samp_k, e->samp_p, e->draws, e->draw_cap, e->step_ctr,
                             mode.advance, e->n_in, e->argmax, e->lps, e->samp_ws, e->s));
  return TI_OK;
}

// TI_PREFILL_LOGITS=0: the last prompt token through a decode step instead (A/B knob, ti_engine_generate)
bool prefill_logits_on() {
  static const int on = [] {
    const char* v = getenv("TI_PREFILL_LOGITS");
    return v ? atoi(v) != 0 : 1;
  }();
  return on != 0;
}

// TI_ATTN_PREFILL=0: prefill chunks through the decode attention kernel (A/B knob)
bool prefill_attn_on() {
  static const int on = [] {
    const char* v = getenv("TI_ATTN_PREFILL");
    return v ? atoi(v) != 0 : 1;
  }();
  return on != 0;
}

// The attention of a prompt chunk of `rows` rows: row-major chunks take one pass over the prefix per 16
// rows on MFMA (ti_attn_prefill, ti_attn_prefill_f8 over an e4m3 cache), packed chunks (int4, 17-64
// rows) and TI_ATTN_PREFILL=0 the decode kernel at stride 0.  enqueue_prefill launches by it and
// ti_engine_prefill_attn_name labels by it.
PfAttn prefill_attn_route(const ti_engine* e, int rows) {
  if (packed_rows(e, rows)) return PF_ATTN_DECODE_PACKED;
  return prefill_attn_on() ? PF_ATTN_MFMA : PF_ATTN_DECODE;
}

// The prompt chunk: ti_engine_set_prefill's rows, or, when that is 0 (prompts consumed by decode steps), the
// chunk of the entry points that prefill regardless (serve, score, lookahead, share_prefix).
int prefill_chunk_rows(const ti_engine* e) {
  return e->pf_rows > 0 ? e->pf_rows : std::min(e->rows_cap, (e->c.bits & ~TI_BITS_G32) == 4 ? TI_GEMM_MAX_ROWS : 16);
}

// Prefill (reference forward_pass, inference_engine.cpp:1429-1491, with the KV kept): prompt
// tokens [t0, t0 + rows) of stream m at positions base + t0 + j, as `rows` rows of the
// batched path that share stream m's KV cache (epilogue / attention stream stride 0: row j
// appends at its own position and attends to [0, base + t0 + j], causal).  No lm_head here: the
// decode loop takes over at the last prompt token, or ti_engine_generate runs the lm_head on the
// chunk's last row.  Not graph-captured (host position upload).
int enqueue_prefill(ti_engine* e, int m, int t0, int rows, int base) {
  ++e->n_prefill_chunks;
  std::vector<int32_t> bp(rows);
  for (int j = 0; j < rows; ++j) bp[j] = base + t0 + j;
  TI_TRY(ti_memcpy_h2d(e->pf_base, bp.data(), (size_t)rows * 4, e->s));
  ti_step_args sa = step_args(e, rows);
  sa.in_stride = 1;                       // row j reads in_tokens[j + step_ctr] = token t0 + j
  sa.out_stride = 0;
  sa.in_tokens = e->in_tokens + (size_t)m * e->in_cap + t0;
  sa.n_in = e->pf_ones;
  sa.out_tokens = nullptr;
  sa.base_pos = e->pf_base;
  sa.step_ctr = e->pf_zero;
  TI_TRY(ti_step_begin(&sa, e->s));
  return enqueue_prefill_layers(e, m, rows, 0);
}

// Tokens [0, n) of slot m's in_tokens row as prompt chunks at positions base + t.
int prefill_tokens(ti_engine* e, int slot, int n, int base) {
  const int pf = prefill_chunk_rows(e);
  for (int t0 = 0; t0 < n; t0 += pf) TI_TRY(enqueue_prefill(e, slot, t0, std::min(pf, n - t0), base));
  return TI_OK;
}

// Every layer of a prompt chunk: `rows` rows of e->h at the positions in e->pos, through stream slot m's KV
// cache (graph-capturable: nothing here touches the host).  split_attn > 0 (the lookahead verify step, at most
// 16 rows of an fp16 cache): the attention is ti_attn_prefill_split with that many splits.
int enqueue_prefill_layers(ti_engine* e, int m, int rows, int split_attn) {
  const ti_engine_config& c = e->c;
  const int H = c.hidden, qd = e->qd(), I = c.inter;
  for (int l = 0; l < c.layers; ++l) {
    DevLayer& L = e->layer[l];
    uint16_t* kc = e->kv_at(L.kc, (size_t)m * e->kv_stride);
    uint16_t* vc = e->kv_at(L.vc, (size_t)m * e->kv_stride);
    TI_TRY(gemm_rows(e, L.qkv, rows, e->h, TI_X_F32_RMSNORM, H, L.attn_norm, qkv_epilogue(e, kc, vc, 0), 4, false));
    const PfAttn route = prefill_attn_route(e, rows);
    const bool pk = route == PF_ATTN_DECODE_PACKED;
    // (an e4m3 cache: on either route every row reads its keys, its own included, from the quantised
    // cache, as a decode step would)
    if (split_attn > 0)
      TI_TRY(ti_attn_prefill_split(e->q, kc, vc, c.max_seq, e->pos, rows, c.heads, c.kv_heads, c.head_dim, split_attn,
                                   e->la_ws, e->attn, e->s));
    else if (route == PF_ATTN_MFMA && e->kv8)
      TI_TRY(ti_attn_prefill_f8(e->q, reinterpret_cast<const uint8_t*>(kc), reinterpret_cast<const uint8_t*>(vc), c.max_seq,
                                e->pos, rows, c.heads, c.kv_heads, c.head_dim, e->attn, e->s));
    else if (route == PF_ATTN_MFMA)
      TI_TRY(ti_attn_prefill(e->q, kc, vc, c.max_seq, e->pos, rows, c.heads, c.kv_heads, c.head_dim, e->attn, e->s));
    else
      TI_TRY(attn_merged(e, pk, kc, vc, 0, rows, e->splits_for(rows)));
    const int xk = pk ? TI_X_F16_PACKED : TI_X_F16;
    TI_TRY(gemm_rows(e, L.o, rows, e->attn, xk, qd, nullptr, resid_epilogue(e), 4, false));
    TI_TRY(gemm_rows(e, L.gu, rows, e->h, TI_X_F32_RMSNORM, H, L.ffn_norm, silu_epilogue(e, pk), 2, false));
    TI_TRY(gemm_rows(e, L.down, rows, e->act, xk, I, nullptr, resid_epilogue(e), 4, false));
  }
  return TI_OK;
}

// ---------------------------------------------------------------------------------------- the graph cache
// Whatever `enqueue` launches on e->s, captured; *out gets the instantiated graph (out null: capture, destroy).
// The callable's error goes ahead of the capture's.
int capture_graph(ti_engine* e, const std::function<int()>& enqueue, hipGraphExec_t* out) {
  TI_TRY(ti_gemm_prepare());
  E_CHECK(hipStreamBeginCapture(e->s, hipStreamCaptureModeThreadLocal), "capture_graph: begin capture");
  const int rc = enqueue();
  hipGraph_t g = nullptr;
  const hipError_t ec = hipStreamEndCapture(e->s, &g);
  hipError_t ei = hipSuccess;
  if (rc == TI_OK && ec == hipSuccess && out) ei = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  if (g) hipGraphDestroy(g);
  TI_TRY(rc);
  E_CHECK(ec, "hipStreamEndCapture");
  E_CHECK(ei, "hipGraphInstantiate");
  return TI_OK;
}

int cached_graph(ti_engine* e, const GraphKey& key, const std::function<int()>& enqueue, hipGraphExec_t* out) {
  auto it = e->graphs.find(key);
  if (it == e->graphs.end()) {
    hipGraphExec_t ex = nullptr;
    TI_TRY(capture_graph(e, enqueue, &ex));
    it = e->graphs.emplace(key, ex).first;
    ++e->n_graphs_captured;
  }
  *out = it->second;
  return TI_OK;
}

// Every cached graph goes (something they bake in is about to change), once the stream has run what it holds.
int drop_graphs(ti_engine* e) {
  TI_TRY(ti_stream_sync(e->s));
  for (auto& g : e->graphs) hipGraphExecDestroy(g.second);
  e->n_graphs_dropped += e->graphs.size();
  e->graphs.clear();
  return TI_OK;
}

// The step graph of M streams in `mode`: the key and the launches come from the one mode object.
int get_graph(ti_engine* e, int M, StepMode mode, hipGraphExec_t* out) {
  const GraphKey key{GraphKey::Step, M, 0, 0, mode.advance, mode.sampled, mode.shared, mode.carry,
                     mode.rows,      mode.rows_pen, mode.rows_big, mode.rows_guide};
  return cached_graph(e, key, [&] { return enqueue_step(e, M, mode); }, out);
}

// The [max_batch][cap] draws / log-probabilities of the sampled step graphs, for `need` draws per stream.
int grow_step_draws(ti_engine* e, int need) {
  if (need <= e->draw_cap) return TI_OK;
  TI_TRY(drop_graphs(e));   // graphs bake the buffers in
  const int cap = std::max(need, 64);
  TI_TRY(e->alloc_t(&e->draws, (size_t)e->c.max_batch * cap));
  TI_TRY(e->alloc_t(&e->lps, (size_t)e->c.max_batch * cap));
  e->draw_cap = cap;
  return TI_OK;
}

// What the sampled step and verify graphs bake in of the sampler: its parameters (kernel arguments) and, for
// top_k above TI_SAMPLE_MAX_K, the HBM workspace its survivors live in (ws_rows rows).  One drop when any changes.
int sampler_prepare(ti_engine* e, float t, int k, float p, int ws_rows) {
  const size_t wsb = ti_sample_workspace_bytes(e->c.vocab, k) * (size_t)ws_rows;
  if (wsb <= e->samp_ws_bytes && e->samp_t == t && e->samp_k == k && e->samp_p == p) return TI_OK;
  TI_TRY(drop_graphs(e));
  if (wsb > e->samp_ws_bytes) {
    void* w = nullptr;
    TI_TRY(e->alloc(&w, wsb));
    e->samp_ws = w;
    e->samp_ws_bytes = wsb;
  }
  e->samp_t = t;
  e->samp_k = k;
  e->samp_p = p;
  return TI_OK;
}

// The sampler's workspace alone, for the rows-mode graphs (their parameters live in e->row_params, so samp_t / k / p
// stay as the scalar graphs baked them): at least `bytes`, growing drops the graphs that bake the pointer in.
int sampler_ws_reserve(ti_engine* e, size_t bytes) {
  if (bytes <= e->samp_ws_bytes) return TI_OK;
  TI_TRY(drop_graphs(e));
  void* w = nullptr;
  TI_TRY(e->alloc(&w, bytes));
  e->samp_ws = w;
  e->samp_ws_bytes = bytes;
  return TI_OK;
}

int ensure_io(ti_engine* e, int in_cap, int out_cap) {
  const int B = e->c.max_batch;
  if (in_cap > e->in_cap) {
    TI_TRY(drop_graphs(e));   // graphs bake the buffers in
    void* p = nullptr;
    TI_TRY(e->alloc(&p, (size_t)B * in_cap * sizeof(int32_t)));
    e->in_tokens = static_cast<int32_t*>(p);
    e->in_cap = in_cap;
  }
  if (out_cap > e->out_cap) {
    TI_TRY(drop_graphs(e));
    void* p = nullptr;
    TI_TRY(e->alloc(&p, (size_t)B * out_cap * sizeof(int32_t)));
    e->out_tokens = static_cast<int32_t*>(p);
    e->out_cap = out_cap;
  }
  return TI_OK;
}

// Row keys of the greedy argmax: max over each row's TI_ARGMAX_SLOTS slots.
int read_argmax(ti_engine* e, int n, std::vector<unsigned long long>& keys) {
  std::vector<unsigned long long> slots((size_t)n * TI_ARGMAX_SLOTS);
  TI_TRY(ti_memcpy_d2h(slots.data(), e->argmax, slots.size() * 8, e->s));
  keys.assign((size_t)n, 0ull);
  for (int m = 0; m < n; ++m)
    for (int j = 0; j < TI_ARGMAX_SLOTS; ++j) keys[m] = std::max(keys[m], slots[(size_t)m * TI_ARGMAX_SLOTS + j]);
  return TI_OK;
}

}  // namespace ti_eng
