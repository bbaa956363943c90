// engine_generate.cpp -- the entry points that run the step graph for whole calls: generate (greedy and sampled),
// single steps, the replay loop of the benchmark, scoring.
#include "engine_impl.hpp"

using namespace ti_eng;

namespace ti_eng {

// ti_engine_generate's body, shared with ti_engine_generate_sampled (`sampled`: the step graph's sampler on)
int generate_impl(ti_engine* e, int n, const int32_t* prompts, const int32_t* lens, int stride, const int32_t* start_pos,
                  int max_new, bool sampled, int32_t* out_tokens, float* last_logits) {
  if (!e || !prompts || !lens || !out_tokens) return ti_set_error(TI_ERR_ARG, "ti_engine_generate: null");
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  if (c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_generate: use ti_engine_compat_step for compat engines");
  if (n < 1 || n > c.max_batch || max_new < 1) return ti_set_error(TI_ERR_ARG, "ti_engine_generate: n=%d max_new=%d", n, max_new);
  int nin_max = 0;
  std::vector<int32_t> nin(n), base(n, 0);
  for (int m = 0; m < n; ++m) {
    if (lens[m] < 1 || lens[m] > stride) return ti_set_error(TI_ERR_ARG, "ti_engine_generate: prompt length %d", lens[m]);
    nin[m] = lens[m];
    nin_max = std::max(nin_max, lens[m]);
    if (start_pos) base[m] = start_pos[m];
  }
  const int steps = nin_max + max_new - 1;
  for (int m = 0; m < n; ++m)
    if (base[m] < 0 || base[m] + steps > c.max_seq)
      return ti_set_error(TI_ERR_ARG, "ti_engine_generate: stream %d needs %d KV slots > max_seq %d", m, base[m] + steps,
                          c.max_seq);
  bool shared = false;   // a registered prefix: cleared when a start position lies inside it, else used
  TI_TRY(share_begin(e, n, base.data(), &shared));
  const StepMode mode{true, sampled, shared, false};
  TI_TRY(ensure_io(e, stride, std::max(steps, 1)));
  std::vector<int32_t> in((size_t)n * e->in_cap, 0);
  for (int m = 0; m < n; ++m) std::memcpy(&in[(size_t)m * e->in_cap], prompts + (size_t)m * stride, (size_t)lens[m] * 4);
  TI_TRY(ti_memcpy_h2d(e->in_tokens, in.data(), in.size() * 4, e->s));
  TI_TRY(ti_memcpy_h2d(e->n_in, nin.data(), (size_t)n * 4, e->s));
  TI_TRY(ti_memcpy_h2d(e->base_pos, base.data(), (size_t)n * 4, e->s));
  if (sampled && e->pen_active())   // each stream's context so far: the registered prefix it continues, its prompt
    for (int m = 0; m < n; ++m) {
      const bool head = e->share_len > 0 && m < e->share_n && base[m] == e->share_len;
      TI_TRY(pen_reset_slot(e, m, e->share_tokens.data(), head ? e->share_len : 0, prompts + (size_t)m * stride, lens[m]));
    }
  if (sampled && e->guide_active()) TI_TRY(guide_start_slots(e, 0, n));   // the prompt is not run through the automaton
  // All but the last prompt token of the shortest prompt go through prefill; the decode loop
  // then starts at that step (same positions, same token feed, same outputs).  Greedy streams
  // whose prompts have one length: the last prompt token is a prefill row too, and the final
  // rms_norm + lm_head + argmax run on each stream's last hidden row (the reference's forward_pass
  // computes the last position's logits the same way, inference_engine.cpp:1429-1491), so the
  // first generated token costs one lm_head GEMM, not a decode step over every layer; the decode
  // loop starts at the step that feeds it.
  int s0 = 0;
  if (e->pf_rows > 0) {
    const int lmin = *std::min_element(nin.begin(), nin.end());
    const bool one_len = *std::max_element(nin.begin(), nin.end()) == lmin;
    const bool last_in_prefill = one_len && !sampled && lmin >= 2 && prefill_logits_on();
    s0 = last_in_prefill ? lmin : lmin - 1;
    const int last_rows = s0 > 0 ? (s0 - 1) % e->pf_rows + 1 : 0;   // rows of each stream's last chunk
    for (int m = 0; m < n; ++m) {
      TI_TRY(prefill_tokens(e, m, s0, base[m]));
      if (last_in_prefill && n > 1)   // (the next stream's chunks reuse h)
        TI_TRY(ti_memcpy_d2d(e->h_last + (size_t)m * c.hidden, e->h + (size_t)(last_rows - 1) * c.hidden,
                             (size_t)c.hidden * 4, e->s));
    }
    if (last_in_prefill) {
      // one stream: its row in place, argmax slots cleared by the chunk's step_begin
      if (n > 1) TI_TRY(ti_memset(e->argmax, 0, (size_t)n * TI_ARGMAX_SLOTS * 8, e->s));
      const float* x = n > 1 ? e->h_last : e->h + (size_t)(last_rows - 1) * c.hidden;
      TI_TRY(gemm_rows(e, e->lm, n, x, TI_X_F32_RMSNORM, c.hidden, e->out_norm, logits_epilogue(e, e->logits), 4, false));
    }
  }
  TI_TRY(ti_memcpy_h2d(e->step_ctr, &s0, 4, e->s));
  std::vector<int32_t> outd((size_t)n * e->out_cap);
  std::vector<unsigned long long> am;
  // generated token t of stream m once `ran` steps have run: the step feed record holds every
  // token but the last, which is still in the argmax slots
  auto token_at = [&](int m, int t, int ran) -> int32_t {
    const int produced = ran - nin[m] + 1;
    if (t < produced - 1) return outd[(size_t)m * e->out_cap + t];
    if (t == produced - 1) return key_token(am[m]);
    return -1;
  };
  int ran = steps;
  if (e->stop_token < 0) {
    TI_TRY(run_steps(e, n, mode, steps - s0));
    TI_TRY(ti_stream_sync(e->s));
    TI_TRY(ti_memcpy_d2h(outd.data(), e->out_tokens, outd.size() * 4, e->s));
    TI_TRY(read_argmax(e, n, am));
  } else {
    // chunks of 4, 8, 16, 32, then 64 steps; after each, every stream's new tokens are read back
    // (one small copy) and the loop ends once each has emitted the stop token
    ran = s0;
    bool all = false;
    auto read_back = [&]() -> int {   // every stream's tokens so far; all = each stopped or complete
      TI_TRY(ti_memcpy_d2h(outd.data(), e->out_tokens, outd.size() * 4, e->s));
      TI_TRY(read_argmax(e, n, am));   // (synchronises the stream)
      all = true;
      for (int m = 0; m < n && all; ++m) {
        bool hit = false;
        const int produced = ran - nin[m] + 1;
        for (int t = 0; t < std::min(produced, max_new) && !hit; ++t) hit = token_at(m, t, ran) == e->stop_token;
        all = hit || produced >= max_new;
      }
      return TI_OK;
    };
    // the prefill's last rows gave every stream its first token: it may already be the stop
    if (ran >= nin_max) TI_TRY(read_back());
    for (int chunk = 4; ran < steps && !all; chunk = std::min(chunk * 2, 64)) {
      const int S = std::min(chunk, steps - ran);
      TI_TRY(run_steps(e, n, mode, S));
      ran += S;
      TI_TRY(read_back());
    }
  }
  for (int m = 0; m < n; ++m) {
    bool stopped = false;
    for (int t = 0; t < max_new; ++t) {
      const int32_t tok = stopped ? -1 : token_at(m, t, ran);
      stopped = stopped || (e->stop_token >= 0 && tok == e->stop_token);
      out_tokens[(size_t)m * max_new + t] = tok;
    }
  }
  if (last_logits) TI_TRY(ti_memcpy_d2h(last_logits, e->logits, (size_t)n * c.vocab * 4, e->s));
  if (n == 1) TI_TRY(qa_fault_check(e));
  return TI_OK;
}

}  // namespace ti_eng

extern "C" {

int ti_engine_generate(ti_engine* e, int n, const int32_t* prompts, const int32_t* lens, int stride,
                       const int32_t* start_pos, int max_new, int32_t* out_tokens, float* last_logits) {
  if (!e || !prompts || !lens || !out_tokens) return ti_set_error(TI_ERR_ARG, "ti_engine_generate: null");
  TI_TRY(pen_refuse(e, "ti_engine_generate"));
  TI_TRY(guide_refuse(e, "ti_engine_generate"));
  return generate_impl(e, n, prompts, lens, stride, start_pos, max_new, false, out_tokens, last_logits);
}

int ti_engine_generate_sampled(ti_engine* e, int n, const int32_t* prompts, const int32_t* lens, int stride,
                               const int32_t* start_pos, int max_new, float temperature, int top_k, float top_p,
                               const float* draws, int32_t* out_tokens, float* out_logprobs) {
  if (!e || !draws) return ti_set_error(TI_ERR_ARG, "ti_engine_generate_sampled: null");
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  if (c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_generate_sampled: compat engine");
  if (n < 1 || n > c.max_batch || max_new < 1) return ti_set_error(TI_ERR_ARG, "ti_engine_generate_sampled: n=%d max_new=%d", n, max_new);
  if (top_k < 1 || top_k > c.vocab)
    return ti_set_error(TI_ERR_ARG, "ti_engine_generate_sampled: top_k %d not in [1, vocab %d]", top_k, c.vocab);
  TI_TRY(grow_step_draws(e, max_new));
  TI_TRY(sampler_prepare(e, temperature, top_k, top_p, c.max_batch));
  std::vector<float> d((size_t)n * e->draw_cap, 0.5f);
  for (int m = 0; m < n; ++m) std::memcpy(&d[(size_t)m * e->draw_cap], draws + (size_t)m * max_new, (size_t)max_new * 4);
  TI_TRY(ti_memcpy_h2d(e->draws, d.data(), d.size() * 4, e->s));
  TI_TRY(generate_impl(e, n, prompts, lens, stride, start_pos, max_new, true, out_tokens, nullptr));
  if (out_logprobs) {
    std::vector<float> lp((size_t)n * e->draw_cap);
    TI_TRY(ti_memcpy_d2h(lp.data(), e->lps, lp.size() * 4, e->s));
    for (int m = 0; m < n; ++m)
      for (int t = 0; t < max_new; ++t)
        out_logprobs[(size_t)m * max_new + t] = out_tokens[(size_t)m * max_new + t] < 0 ? 0.0f : lp[(size_t)m * e->draw_cap + t];
  }
  return TI_OK;
}

// ------------------------------------------------------------------------------ scoring
// InferenceEngine::compute_logprobs (inference_engine.cpp:873-954): the reference runs forward_pass
// over the sequence and reduces every position's logits on the host (:918-944).  Here the tokens run
// as prefill chunks into the slot's KV cache; after each chunk the final rms_norm + lm_head run on
// its rows of e->h in blocks of TI_SCORE_ROWS into sc_logits, and ti_logprob_rows leaves one
// log-probability (and argmax) per row on the device.  Nothing is read back until the end.
int ti_engine_score(ti_engine* e, int stream, const int32_t* tokens, int n, int start_pos, const int32_t* targets,
                    float* out_logprob, int32_t* out_top1) {
  if (!e || !tokens || !out_logprob) return ti_set_error(TI_ERR_ARG, "ti_engine_score: null");
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  if (c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_score: compat engine");
  if (n < 1) return ti_set_error(TI_ERR_ARG, "ti_engine_score: n=%d", n);
  if (stream < 0 || stream >= c.max_batch)
    return ti_set_error(TI_ERR_ARG, "ti_engine_score: stream %d of %d", stream, c.max_batch);
  if (start_pos < 0 || n > c.max_seq - start_pos)
    return ti_set_error(TI_ERR_ARG, "ti_engine_score: start_pos %d + %d tokens, max_seq %d", start_pos, n, c.max_seq);
  if (!targets) targets = tokens;
  for (int i = 0; i < n; ++i) {
    if (tokens[i] < 0 || tokens[i] >= c.vocab)
      return ti_set_error(TI_ERR_ARG, "ti_engine_score: token %d at %d outside [0, vocab %d)", tokens[i], i, c.vocab);
    if (targets[i] < -1 || targets[i] >= c.vocab)
      return ti_set_error(TI_ERR_ARG, "ti_engine_score: target %d at %d outside [-1, vocab %d)", targets[i], i, c.vocab);
  }
  if (stream < e->share_n && start_pos < e->share_len) TI_TRY(share_clear(e));
  if (!e->sc_logits) {
    TI_TRY(e->alloc_t(&e->sc_logits, (size_t)TI_SCORE_ROWS * c.vocab));
    TI_TRY(e->alloc_t(&e->sc_targets, (size_t)c.max_seq));
    TI_TRY(e->alloc_t(&e->sc_lp, (size_t)c.max_seq));
    TI_TRY(e->alloc_t(&e->sc_top1, (size_t)c.max_seq));
  }
  TI_TRY(ensure_io(e, n, 1));
  TI_TRY(ti_memcpy_h2d(e->in_tokens + (size_t)stream * e->in_cap, tokens, (size_t)n * 4, e->s));
  TI_TRY(ti_memcpy_h2d(e->sc_targets, targets, (size_t)n * 4, e->s));
  const int pf = prefill_chunk_rows(e);
  for (int t0 = 0; t0 < n; t0 += pf) {
    const int rows = std::min(pf, n - t0);
    TI_TRY(enqueue_prefill(e, stream, t0, rows, start_pos));
    for (int r0 = 0; r0 < rows; r0 += TI_SCORE_ROWS) {
      const int m = std::min(TI_SCORE_ROWS, rows - r0);
      TI_TRY(gemm_rows(e, e->lm, m, e->h + (size_t)r0 * c.hidden, TI_X_F32_RMSNORM, c.hidden, e->out_norm,
                       logits_epilogue(e, e->sc_logits, false), 4, false));
      TI_TRY(ti_logprob_rows(e->sc_logits, c.vocab, m, c.vocab, e->sc_targets + t0 + r0, e->sc_lp + t0 + r0,
                             e->sc_top1 + t0 + r0, e->s));
    }
  }
  TI_TRY(ti_memcpy_d2h(out_logprob, e->sc_lp, (size_t)n * 4, e->s));   // (synchronises the stream)
  if (out_top1) TI_TRY(ti_memcpy_d2h(out_top1, e->sc_top1, (size_t)n * 4, e->s));
  return TI_OK;
}

int ti_engine_step(ti_engine* e, int n, const int32_t* tokens, const int32_t* pos, float* logits) {
  if (!e || !tokens || !pos) return ti_set_error(TI_ERR_ARG, "ti_engine_step: null");
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  if (c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_step: compat engine");
  if (n < 1 || n > c.max_batch) return ti_set_error(TI_ERR_ARG, "ti_engine_step: n=%d", n);
  for (int m = 0; m < n; ++m)
    if (pos[m] < 0 || pos[m] >= c.max_seq) return ti_set_error(TI_ERR_ARG, "ti_engine_step: pos %d", pos[m]);
  bool shared = false;
  TI_TRY(share_begin(e, n, pos, &shared));
  TI_TRY(ensure_io(e, 1, 1));
  std::vector<int32_t> in((size_t)n * e->in_cap, 0), one(n, 1);
  for (int m = 0; m < n; ++m) in[(size_t)m * e->in_cap] = tokens[m];
  TI_TRY(ti_memcpy_h2d(e->in_tokens, in.data(), in.size() * 4, e->s));
  TI_TRY(ti_memcpy_h2d(e->n_in, one.data(), (size_t)n * 4, e->s));
  TI_TRY(ti_memcpy_h2d(e->base_pos, pos, (size_t)n * 4, e->s));
  TI_TRY(ti_memset(e->step_ctr, 0, 4, e->s));
  TI_TRY(run_steps(e, n, StepMode{true, false, shared, false}, 1));
  TI_TRY(ti_stream_sync(e->s));
  if (logits) TI_TRY(ti_memcpy_d2h(logits, e->logits, (size_t)n * c.vocab * 4, e->s));
  if (n == 1) TI_TRY(qa_fault_check(e));
  return TI_OK;
}

int ti_engine_compat_step(ti_engine* e, int placeholder_offset, float* logits) {
  if (!e || !e->c.compat) return ti_set_error(TI_ERR_ARG, "ti_engine_compat_step: not a compat engine");
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  const int H = c.hidden, I = c.inter, V = c.vocab;
  std::vector<int32_t> zero(1, 0);
  TI_TRY(ti_memset(e->step_ctr, 0, 4, e->s));
  ti_step_args sa{};
  sa.h = e->h;
  sa.hidden = H;
  sa.M = 1;
  sa.vocab = V;
  sa.placeholder_first = placeholder_offset;
  sa.argmax = e->argmax;
  sa.pos = e->pos;
  sa.base_pos = e->base_pos;
  sa.step_ctr = e->step_ctr;
  TI_TRY(ti_step_begin(&sa, e->s));
  for (int l = 0; l < c.layers; ++l) {
    DevLayer& L = e->layer[l];
    // TransformerLayer::forward without attention weights (inference_engine.cpp:293-296):
    // post_attn = add(x, x); ffn = relu(post_attn @ up) @ down (:392-398); out = add(post_attn, ffn).
    TI_TRY(ti_add_f32(e->h, e->h, e->h, H, e->s));
    TI_TRY(ti_matmul_f32(e->h, L.gu.f32, e->tmp, nullptr, 1, H, I, 1, e->s));
    TI_TRY(ti_matmul_f32(e->tmp, L.down.f32, e->h, e->h, 1, I, H, 2, e->s));
  }
  TI_TRY(ti_matmul_f32(e->h, e->lm.f32, e->logits, nullptr, 1, H, V, 0, e->s));
  TI_TRY(ti_stream_sync(e->s));
  if (logits) TI_TRY(ti_memcpy_d2h(logits, e->logits, (size_t)V * 4, e->s));
  return TI_OK;
}

int ti_engine_replay_prepare(ti_engine* e, int n, int kv_len, int start_token) {
  if (!e || e->c.compat) return ti_set_error(TI_ERR_ARG, "ti_engine_replay_prepare: bad engine");
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  if (n < 1 || n > c.max_batch || kv_len < 1 || kv_len > c.max_seq || start_token < 0 || start_token >= c.vocab)
    return ti_set_error(TI_ERR_ARG, "ti_engine_replay_prepare: n=%d kv_len=%d", n, kv_len);
  if (kv_len - 1 < e->share_len) TI_TRY(share_clear(e));
  TI_TRY(ensure_io(e, 1, 1));
  std::vector<int32_t> base(n, kv_len - 1), zero(n, 0);
  std::vector<unsigned long long> am((size_t)n * TI_ARGMAX_SLOTS, 0ull);
  for (int m = 0; m < n; ++m) am[(size_t)m * TI_ARGMAX_SLOTS] = 0xFFFFFFFFu - (uint32_t)start_token;
  TI_TRY(ti_memcpy_h2d(e->base_pos, base.data(), (size_t)n * 4, e->s));
  TI_TRY(ti_memcpy_h2d(e->n_in, zero.data(), (size_t)n * 4, e->s));
  TI_TRY(ti_memcpy_h2d(e->argmax, am.data(), am.size() * 8, e->s));
  TI_TRY(ti_memset(e->step_ctr, 0, 4, e->s));
  hipGraphExec_t g = nullptr;
  TI_TRY(get_graph(e, n, StepMode{}, &g));
  e->replay_M = n;
  return ti_stream_sync(e->s);
}

int ti_engine_replay_run(ti_engine* e, int steps) {
  if (!e || e->replay_M < 1) return ti_set_error(TI_ERR_ARG, "ti_engine_replay_run: call ti_engine_replay_prepare first");
  DeviceScope bind_(e);
  return run_steps(e, e->replay_M, StepMode{}, steps);
}

int ti_engine_sync(ti_engine* e) {
  if (!e) return ti_set_error(TI_ERR_ARG, "ti_engine_sync: null");
  DeviceScope bind_(e);
  TI_TRY(ti_stream_sync(e->s));
  return TI_OK;
}

int ti_engine_last_tokens(ti_engine* e, int n, int32_t* tokens) {
  if (!e || !tokens || n < 1 || n > e->c.max_batch) return ti_set_error(TI_ERR_ARG, "ti_engine_last_tokens");
  DeviceScope bind_(e);
  std::vector<unsigned long long> am;
  TI_TRY(read_argmax(e, n, am));
  for (int m = 0; m < n; ++m) tokens[m] = key_token(am[m]);
  return TI_OK;
}

}  // extern "C"
