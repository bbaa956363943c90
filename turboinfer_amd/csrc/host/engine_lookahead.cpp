#include "engine_impl.hpp"

using namespace ti_eng;

// ------------------------------------------------------------------------------ lookahead greedy decoding
namespace {

// Splits of the verify step's attention (ti_attn_prefill_split).  A split's time is its share of the keys plus
// a merge that grows with the split count, so the best count goes with the square root of the keys and hardly
// with the rows: 8 measured fastest at 2048 keys (4 / 8 / 16 / 32: 18.3 / 14.5 / 16.3 / 25.7 us, 7B shape, 8 or
// 16 rows) and 16 at 8192 (55 / 32 / 25 / 30 us at 8 rows of the Llama-3-8B shape, 55 / 33 / 30 / 39 at 16;
// profiles/lookahead_ab.txt) -- sqrt(max_seq / 32), with at most one wave per SIMD over the (query blocks x
// kv-heads) and at most 32.  ti_engine_config.attn_splits overrides it as it does the decode attention's.
int la_splits(const ti_engine* e, int R) {
  const ti_engine_config& c = e->c;
  if (c.attn_splits > 0) return std::min(c.attn_splits, 32);
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 256;
  const int G = c.heads / c.kv_heads, qpw = std::max(1, 16 / G), blocks = (R + qpw - 1) / qpw * c.kv_heads;
  const int by_keys = (int)std::lround(std::sqrt((double)c.max_seq / 32.0));
  return std::max(1, std::min(std::min(by_keys, std::max(1, 4 * cus / blocks)), 32));
}

ti_lookahead_args la_args(ti_engine* e, int k) {
  const ti_engine_config& c = e->c;
  ti_lookahead_args a{};
  a.state = e->la_state;
  a.cfg = e->la_state + TI_LA_STATE_WORDS;
  a.hist = e->la_hist;
  a.k = k;
  a.hidden = c.hidden;
  a.vocab = c.vocab;
  a.max_pos = c.max_seq - 1;
  a.emb = e->emb;
  a.h = e->h;
  a.row_tok = e->la_row_tok;
  a.pos = e->pos;
  a.argmax = e->argmax;
  a.out_tokens = e->la_out;
  return a;
}

// One verify step of stream slot `stream`: the draft lookup, k + 1 rows through every layer as a prompt chunk
// (positions from the device, key-split attention), the lm_head's greedy keys, accept / commit.
// `sampled`: ti_lookahead_sample between the two turns each live row's greedy keys into its sampled token's.
int enqueue_verify(ti_engine* e, int stream, int k, int splits, bool sampled) {
  const ti_engine_config& c = e->c;
  const int R = k + 1;
  const ti_lookahead_args a = la_args(e, k);
  TI_TRY(ti_lookahead_begin(&a, e->s));
  TI_TRY(enqueue_prefill_layers(e, stream, R, splits));
  TI_TRY(gemm_rows(e, e->lm, R, e->h, TI_X_F32_RMSNORM, c.hidden, e->out_norm, logits_epilogue(e, e->la_logits), 4, false));
  if (sampled)
    TI_TRY(ti_lookahead_sample(e->la_logits, c.vocab, R, c.vocab, e->samp_t, e->samp_k, e->samp_p, e->la_draws,
                               e->la_samp_cap, a.state, a.cfg, e->argmax, e->la_lps, e->samp_ws, e->s));
  return ti_lookahead_accept(&a, e->s);
}

int get_verify_graph(ti_engine* e, int stream, int k, int splits, bool sampled, hipGraphExec_t* out) {
  const GraphKey key{GraphKey::Verify, k + 1, stream, splits, false, sampled, false, false};
  return cached_graph(e, key, [&] { return enqueue_verify(e, stream, k, splits, sampled); }, out);
}

// The sampler of ti_engine_generate_lookahead_sampled (null: the greedy entry point, which enqueues nothing of it)
struct LaSampler {
  float temperature;
  int top_k;
  float top_p;
  const float* draws;   // host [max_new]
  float* out_logprobs;  // host [max_new], nullable
};

int la_generate(const char* fn, ti_engine* e, int stream, const int32_t* prompt, int prompt_len, int start_pos,
                const int32_t* corpus, int corpus_len, int k, int ngram, int max_new, const LaSampler* sp,
                int32_t* out_tokens, ti_lookahead_stats* stats) {
  if (!e || !prompt || !out_tokens || (!corpus && corpus_len != 0) || (sp && !sp->draws))
    return ti_set_error(TI_ERR_ARG, "%s: null", fn);
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  if (c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "%s: compat engine", fn);
  if (e->kv8) return ti_set_error(TI_ERR_UNSUPPORTED, "%s: TI_BITS_KV8 engine (no e4m3 key-split prefill attention)", fn);
  TI_TRY(pen_refuse(e, fn));
  TI_TRY(guide_refuse(e, fn));
  if (stream < 0 || stream >= c.max_batch) return ti_set_error(TI_ERR_ARG, "%s: stream %d of %d", fn, stream, c.max_batch);
  if (prompt_len < 1 || max_new < 1 || corpus_len < 0)
    return ti_set_error(TI_ERR_ARG, "%s: prompt_len %d max_new %d corpus_len %d", fn, prompt_len, max_new, corpus_len);
  if (k < 1 || k > TI_LA_MAX_K) return ti_set_error(TI_ERR_ARG, "%s: k %d outside [1, %d]", fn, k, TI_LA_MAX_K);
  if (ngram < 1 || ngram > TI_LA_MAX_NGRAM)
    return ti_set_error(TI_ERR_ARG, "%s: ngram %d outside [1, %d]", fn, ngram, TI_LA_MAX_NGRAM);
  if (sp && (sp->top_k < 1 || sp->top_k > c.vocab))
    return ti_set_error(TI_ERR_ARG, "%s: top_k %d not in [1, vocab %d]", fn, sp->top_k, c.vocab);
  for (int i = 0; i < prompt_len; ++i)
    if (prompt[i] < 0 || prompt[i] >= c.vocab)
      return ti_set_error(TI_ERR_ARG, "%s: prompt token %d at %d outside [0, vocab %d)", fn, prompt[i], i, c.vocab);
  for (int i = 0; i < corpus_len; ++i)
    if (corpus[i] < 0 || corpus[i] >= c.vocab)
      return ti_set_error(TI_ERR_ARG, "%s: corpus token %d at %d outside [0, vocab %d)", fn, corpus[i], i, c.vocab);
  // the verify rows reach k slots past the last token fed
  if (start_pos < 0 || (int64_t)start_pos + prompt_len + max_new - 1 + k > c.max_seq)
    return ti_set_error(TI_ERR_ARG, "%s: start_pos %d + %d prompt + %d new - 1 + k %d > max_seq %d", fn, start_pos,
                        prompt_len, max_new, k, c.max_seq);
  const int64_t cap64 = (int64_t)corpus_len + prompt_len + max_new;
  if (cap64 > (1 << 28)) return ti_set_error(TI_ERR_ARG, "%s: history of %lld tokens", fn, (long long)cap64);
  const int cap = (int)cap64, R = k + 1;
  if (stream < e->share_n && start_pos < e->share_len) TI_TRY(share_clear(e));

  if (!e->la_logits) {
    TI_TRY(e->alloc_t(&e->la_logits, (size_t)(TI_LA_MAX_K + 1) * c.vocab));
    TI_TRY(e->alloc_t(&e->la_state, (size_t)TI_LA_STATE_WORDS + 4));
    TI_TRY(e->alloc_t(&e->la_row_tok, (size_t)TI_LA_MAX_K + 1));
    void* w = nullptr;   // (alloc zeroes it: the tickets' one-time arming)
    TI_TRY(e->alloc(&w, ti_attn_prefill_split_workspace_bytes(TI_LA_MAX_K + 1, c.heads, c.head_dim, 32)));
    e->la_ws = static_cast<float*>(w);
  }
  if (cap > e->la_hist_cap || max_new > e->la_out_cap) {   // the verify graphs bake these buffers in
    TI_TRY(drop_graphs(e));
    if (cap > e->la_hist_cap) {
      TI_TRY(e->alloc_t(&e->la_hist, (size_t)cap));
      e->la_hist_cap = cap;
    }
    if (max_new > e->la_out_cap) {
      TI_TRY(e->alloc_t(&e->la_out, (size_t)max_new));
      e->la_out_cap = max_new;
    }
  }
  if (sp) {
    // what the sampled verify graphs bake in, as ti_engine_generate_sampled does for the step graphs: the draw
    // and log-probability buffers, the sampler workspace (top_k > TI_SAMPLE_MAX_K, one row per verify row;
    // shared with the step graphs, whose max_batch rows it must still hold) and the sampler's parameters
    if (max_new > e->la_samp_cap) {
      TI_TRY(drop_graphs(e));
      const int scap = std::max(max_new, 64);
      TI_TRY(e->alloc_t(&e->la_draws, (size_t)scap));
      TI_TRY(e->alloc_t(&e->la_lps, (size_t)scap));
      e->la_samp_cap = scap;
    }
    TI_TRY(sampler_prepare(e, sp->temperature, sp->top_k, sp->top_p, std::max(c.max_batch, TI_LA_MAX_K + 1)));
    TI_TRY(ti_memcpy_h2d(e->la_draws, sp->draws, (size_t)max_new * 4, e->s));
  }
  TI_TRY(ensure_io(e, prompt_len, 1));
  TI_TRY(ti_memcpy_h2d(e->in_tokens + (size_t)stream * e->in_cap, prompt, (size_t)prompt_len * 4, e->s));
  std::vector<int32_t> hist((size_t)corpus_len + prompt_len);
  if (corpus_len) std::memcpy(hist.data(), corpus, (size_t)corpus_len * 4);
  std::memcpy(hist.data() + corpus_len, prompt, (size_t)prompt_len * 4);
  TI_TRY(ti_memcpy_h2d(e->la_hist, hist.data(), hist.size() * 4, e->s));
  int32_t st[TI_LA_STATE_WORDS + 4] = {(int32_t)hist.size(), start_pos + prompt_len - 1, 0, 0, 0, 0, 0, 0,
                                       ngram, max_new, e->stop_token, cap};
  TI_TRY(ti_memcpy_h2d(e->la_state, st, sizeof(st), e->s));
  // prompt[0 .. n - 2] as prompt chunks; prompt[n - 1] is row 0 of the first step
  TI_TRY(prefill_tokens(e, stream, prompt_len - 1, start_pos));
  hipGraphExec_t g = nullptr;
  TI_TRY(get_verify_graph(e, stream, k, la_splits(e, R), sp != nullptr, &g));
  // replays in growing chunks (4, 8, 16, .. 64), the state read back after each; at most max_new steps.  A
  // replay after `done` changes nothing (begin writes padding rows, accept returns) but costs a whole step, a
  // read-back costs microseconds: a chunk is no longer than the steps the rest needs at the tokens per step
  // seen so far (17 steps of 7.5 tokens ran 28 replays without this, profiles/lookahead_ab.txt)
  int ran = 0;
  for (int chunk = 4; ran < max_new && !st[3]; chunk = std::min(chunk * 2, 64)) {
    int S = std::min(chunk, max_new - ran);
    if (st[4] > 0 && st[2] > 0)
      S = std::min(S, std::max(1, (int)(((int64_t)(max_new - st[2]) * st[4] + st[2] - 1) / st[2])));
    for (int i = 0; i < S; ++i) E_CHECK(hipGraphLaunch(g, e->s), "hipGraphLaunch");
    ran += S;
    TI_TRY(ti_memcpy_d2h(st, e->la_state, TI_LA_STATE_WORDS * 4, e->s));   // (synchronises the stream)
  }
  e->n_decode_steps += (uint64_t)st[4];
  const int produced = std::min(std::max(st[2], 0), max_new);
  if (produced) TI_TRY(ti_memcpy_d2h(out_tokens, e->la_out, (size_t)produced * 4, e->s));
  for (int t = produced; t < max_new; ++t) out_tokens[t] = -1;
  if (sp && sp->out_logprobs) {
    if (produced) TI_TRY(ti_memcpy_d2h(sp->out_logprobs, e->la_lps, (size_t)produced * 4, e->s));
    for (int t = produced; t < max_new; ++t) sp->out_logprobs[t] = 0.0f;
  }
  if (stats) *stats = ti_lookahead_stats{st[4], st[5], st[6], st[2]};
  if (!st[3]) return ti_set_error(TI_ERR_HIP, "%s: not complete after %d verify steps (produced %d of %d)", fn, ran, st[2], max_new);
  return TI_OK;
}

}  // namespace

extern "C" {

int ti_engine_generate_lookahead(ti_engine* e, int stream, const int32_t* prompt, int prompt_len, int start_pos,
                                 const int32_t* corpus, int corpus_len, int k, int ngram, int max_new,
                                 int32_t* out_tokens, ti_lookahead_stats* stats) {
  return la_generate("ti_engine_generate_lookahead", e, stream, prompt, prompt_len, start_pos, corpus, corpus_len, k,
                     ngram, max_new, nullptr, out_tokens, stats);
}

int ti_engine_generate_lookahead_sampled(ti_engine* e, int stream, const int32_t* prompt, int prompt_len, int start_pos,
                                         const int32_t* corpus, int corpus_len, int k, int ngram, int max_new,
                                         float temperature, int top_k, float top_p, const float* draws,
                                         int32_t* out_tokens, float* out_logprobs, ti_lookahead_stats* stats) {
  const LaSampler sp{temperature, top_k, top_p, draws, out_logprobs};
  return la_generate("ti_engine_generate_lookahead_sampled", e, stream, prompt, prompt_len, start_pos, corpus,
                     corpus_len, k, ngram, max_new, &sp, out_tokens, stats);
}

}  // extern "C"
