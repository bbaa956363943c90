#include "engine_impl.hpp"

using namespace ti_eng;

// ------------------------------------------------------------------ continuous batching
// Requests flow through the engine's max_batch stream slots.  Every chunk of the device loop
// starts with each slot feeding one token at its own position (step_ctr 0, n_in 1): a
// continuing request its last generated token, a newly admitted one the last token of its
// prompt, whose other tokens were prefilled into the slot's KV (enqueue_prefill) just before.
// After the chunk the slots' new tokens are read back (the step feed record + the last
// argmax); finished requests (EOS, max_new) free their slot for the next queued request.
//
// ti_engine_serve_sampled (sp != null) is the same loop with the step graph's sampler on (StepMode::sampled).
// A chunk's step s is every slot's draw index s (step_ctr 0, n_in 1), so before
// the chunk each live slot's row of the [max_batch][draw_cap] draw buffer gets its request's next draws, and
// after it the row of log-probabilities is read back.  With sp == null nothing of this is enqueued.
//
// ti_engine_serve_requests (sp->params != null) is the sampled loop with request r's budget, stop token, sampler
// values and penalties its own: max_new is then the stride of the host arrays (>= every request's budget), the step
// graph is the rows-mode one (StepMode::rows), and the slots' table e->row_params is copied before a chunk whenever
// a slot changed hands.  With params == null nothing of this is enqueued either.
//
// ti_engine_serve_requests_guided (sp->guides != null) is the rows loop with request r under the library guide
// guides[r] (engine_guide.cpp; 0 = none): when some request names one (StepMode::rows_guide) the slot's table entry
// carries the handle, ti_guide_step_rows is in the graph, and a slot's state is reset at admission to its guide's
// start or to -1.  With no handle named nothing of this is enqueued.
struct ServeSampler {
  const float* draws;   // host [n_req][max_new]
  float* out_logprobs;  // host [n_req][max_new], nullable
  const ti_request_params* params = nullptr;   // host [n_req], nullable
  const int32_t* guides = nullptr;             // host [n_req] library handles (0 = none), nullable; with params only
};

static bool penalises(const ti_request_params& q) { return q.repetition != 1.0f || q.presence != 0.0f || q.frequency != 0.0f; }

static int serve_loop(const char* fn, ti_engine* e, int n_req, const int32_t* prompts, const int32_t* offsets,
                      int max_new, int eos, int chunk, const ServeSampler* sp, int32_t* out_tokens, int32_t* out_len) {
  const ti_engine_config& c = e->c;
  const int B = c.max_batch;
  const ti_request_params* rp = sp ? sp->params : nullptr;
  auto budget = [&](int r) { return rp ? rp[r].max_new : max_new; };
  auto stop = [&](int r) { return rp ? rp[r].stop_token : eos; };
  // A prefix registered for every slot (ti_engine_share_prefix with n_streams == max_batch): each prompt is the
  // continuation behind it, every slot -- idle ones too -- sits at or past P and never touches its copy of the
  // prefix, so a freed slot is reused without a new copy.  Registered for fewer slots: cleared.  P = 0: as ever.
  if (e->share_len > 0 && e->share_n != B) TI_TRY(share_clear(e));
  const int P = e->share_len;
  int max_len = 1;
  for (int r = 0; r < n_req; ++r) {
    const int L = offsets[r + 1] - offsets[r];
    if (L < 1 || P + L + budget(r) - 1 > c.max_seq)
      return ti_set_error(TI_ERR_ARG, "%s: request %d: %d prompt + %d new tokens exceed max_seq %d", fn, r, P + L, budget(r),
                          c.max_seq);
    max_len = std::max(max_len, L);
  }
  const int32_t* gh = rp ? sp->guides : nullptr;
  // some request penalises / has top_k above the LDS instance's / names a library guide
  bool rows_pen = false, rows_big = false, rows_guide = false;
  for (int r = 0; rp && r < n_req; ++r) {
    rows_pen = rows_pen || penalises(rp[r]);
    rows_big = rows_big || rp[r].top_k > TI_SAMPLE_MAX_K;
    rows_guide = rows_guide || (gh && gh[r] > 0);
  }
  // (the greedy loop is refused while they are active; the rows loop has its own, the engine-wide ones do not apply)
  const bool pen = rp ? rows_pen : sp && e->pen_active();
  // (the engine's one guide, or each request's own out of the library: the entry point refuses both in one call)
  const bool guide = sp && (rows_guide || e->guide_active());
  const StepMode mode{true,     sp != nullptr, P > 0 && B >= 2 && P >= e->share_min, pen || guide, rp != nullptr, rows_pen,
                      rows_big, rows_guide};
  auto slot_guide = [&](int r) { return rows_guide ? gh[r] : 0; };   // the handle the request's slot carries
  auto slot_pen = [&](int r) { return rp ? penalises(rp[r]) : pen; };   // does the request in the slot penalise
  if (rp) {   // what the rows-mode graphs bake in: the table, the penalty state, the workspace (only growth drops graphs)
    if (!e->row_params) TI_TRY(e->alloc_t(&e->row_params, (size_t)B));
    if (rows_pen) TI_TRY(pen_state_alloc(e));
    if (rows_big) TI_TRY(sampler_ws_reserve(e, ti_sample_workspace_bytes(c.vocab, c.vocab) * (size_t)B));
  }
  ti_row_params idle{};
  idle.temperature = idle.top_p = idle.repetition = 1.0f;
  idle.top_k = 1;
  std::vector<ti_row_params> table(rp ? B : 0, idle);
  bool table_moved = rp != nullptr;   // a slot changed hands since the last copy
  std::vector<int32_t> carry(B, -1);
  TI_TRY(ensure_io(e, max_len, chunk + 1));
  for (int i = 0; i < n_req * max_new; ++i) out_tokens[i] = -1;
  for (int r = 0; r < n_req; ++r) out_len[r] = 0;
  std::vector<int> slot_req(B, -1), slot_pos(B, 0), slot_tok(B, 0);
  std::vector<int32_t> in((size_t)B * e->in_cap, 0), nin(B, 1), base(B, 0), outd((size_t)B * e->out_cap);
  std::vector<unsigned long long> am;
  std::vector<float> dr, lp;
  if (sp) {
    dr.assign((size_t)B * e->draw_cap, 0.5f);
    lp.resize((size_t)B * e->draw_cap);
    if (sp->out_logprobs) std::fill(sp->out_logprobs, sp->out_logprobs + (size_t)n_req * max_new, 0.0f);
  }
  int next = 0, live = 0;
  for (;;) {
    // admit queued requests into free slots: prefill all but the prompt's last token
    std::vector<int> fresh;
    for (int m = 0; m < B && next < n_req; ++m)
      if (slot_req[m] < 0) {
        const int r = next++, L = offsets[r + 1] - offsets[r];
        slot_req[m] = r;
        slot_pos[m] = P + L - 1;
        slot_tok[m] = prompts[offsets[r] + L - 1];
        fresh.push_back(m);
        ++live;
      }
    if (live == 0) break;
    if (!fresh.empty()) {
      for (int m : fresh) {
        const int r = slot_req[m], L = offsets[r + 1] - offsets[r];
        std::memcpy(&in[(size_t)m * e->in_cap], prompts + offsets[r], (size_t)L * 4);
      }
      TI_TRY(ti_memcpy_h2d(e->in_tokens, in.data(), in.size() * 4, e->s));
      for (int m : fresh) {
        const int L = offsets[slot_req[m] + 1] - offsets[slot_req[m]];
        TI_TRY(prefill_tokens(e, m, L - 1, P));
        // the slot's histogram starts over: the registered prefix, then the whole prompt (its last token too)
        if (pen && slot_pen(slot_req[m])) TI_TRY(pen_reset_slot(e, m, e->share_tokens.data(), P, prompts + offsets[slot_req[m]], L));
        // a freed slot restarts at the guide's start state; the request's own guide's, or free without one
        if (guide) TI_TRY(rows_guide ? guide_reset_slot(e, m, gh[slot_req[m]]) : guide_start_slots(e, m, 1));
        if (rp) {
          const ti_request_params& q = rp[slot_req[m]];
          table[m] = ti_row_params{q.temperature, q.top_k, q.top_p, q.repetition, q.presence, q.frequency,
                                   {slot_guide(slot_req[m]), 0}};
          table_moved = true;
        }
      }
    }
    if (table_moved) {   // in stream order, like the draws: the graphs bake the pointer, never the values
      TI_TRY(ti_memcpy_h2d(e->row_params, table.data(), table.size() * sizeof(ti_row_params), e->s));
      table_moved = false;
    }
    if (pen || guide) {   // a continuing slot feeds a generated token the histogram / the automaton has not seen yet
      for (int m = 0; m < B; ++m) carry[m] = slot_req[m] >= 0 ? slot_tok[m] : -1;
      for (int m : fresh) carry[m] = -1;
      TI_TRY(ti_memcpy_h2d(e->pen_carry, carry.data(), (size_t)B * 4, e->s));
    }
    // one chunk: every slot feeds one token at its position; no slot may run past max_seq
    int S = chunk;
    for (int m = 0; m < B; ++m) {
      nin[m] = 1;
      base[m] = slot_req[m] >= 0 ? slot_pos[m] : P;
      in[(size_t)m * e->in_cap] = slot_req[m] >= 0 ? slot_tok[m] : 0;
      if (slot_req[m] >= 0) S = std::min(S, c.max_seq - slot_pos[m]);
    }
    // (stream order: these copies land after the prefill launches have read in_tokens)
    TI_TRY(ti_memcpy_h2d(e->in_tokens, in.data(), in.size() * 4, e->s));
    TI_TRY(ti_memcpy_h2d(e->n_in, nin.data(), (size_t)B * 4, e->s));
    TI_TRY(ti_memcpy_h2d(e->base_pos, base.data(), (size_t)B * 4, e->s));
    const int32_t zero = 0;
    TI_TRY(ti_memcpy_h2d(e->step_ctr, &zero, 4, e->s));
    if (sp) {   // request r's t-th new token takes draws[r][t], whatever slot and chunk it runs in
      for (int m = 0; m < B; ++m) {
        const int r = slot_req[m];
        if (r < 0) continue;
        const int nd = std::min(S, budget(r) - out_len[r]);
        std::memcpy(&dr[(size_t)m * e->draw_cap], sp->draws + (size_t)r * max_new + out_len[r], (size_t)nd * 4);
      }
      TI_TRY(ti_memcpy_h2d(e->draws, dr.data(), dr.size() * 4, e->s));
    }
    TI_TRY(run_steps(e, B, mode, S));
    TI_TRY(ti_memcpy_d2h(outd.data(), e->out_tokens, outd.size() * 4, e->s));
    if (sp && sp->out_logprobs) TI_TRY(ti_memcpy_d2h(lp.data(), e->lps, lp.size() * 4, e->s));
    TI_TRY(read_argmax(e, B, am));   // synchronises the stream
    for (int m = 0; m < B; ++m) {
      const int r = slot_req[m];
      if (r < 0) continue;
      // the token generated at chunk step s: fed back and recorded at step s + 1, the last
      // one still in the argmax slots
      for (int s = 0; s < S && slot_req[m] >= 0; ++s) {
        const int32_t tok = s < S - 1 ? outd[(size_t)m * e->out_cap + s] : key_token(am[m]);
        if (sp && sp->out_logprobs) sp->out_logprobs[(size_t)r * max_new + out_len[r]] = lp[(size_t)m * e->draw_cap + s];
        out_tokens[(size_t)r * max_new + out_len[r]++] = tok;
        slot_tok[m] = tok;
        if (out_len[r] >= budget(r) || tok == stop(r)) {
          slot_req[m] = -1;
          --live;
          if (rp) {   // the slot is idle until the next admission
            table[m] = idle;
            table_moved = true;
          }
        }
      }
      if (slot_req[m] >= 0) slot_pos[m] += S;
    }
  }
  return TI_OK;
}

extern "C" {

int ti_engine_serve(ti_engine* e, int n_req, const int32_t* prompts, const int32_t* offsets, int max_new, int eos,
                    int chunk, int32_t* out_tokens, int32_t* out_len) {
  if (!e || !prompts || !offsets || !out_tokens || !out_len || n_req < 1 || max_new < 1 || chunk < 1)
    return ti_set_error(TI_ERR_ARG, "ti_engine_serve: bad arguments");
  DeviceScope bind_(e);
  if (e->c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_serve: compat engine");
  TI_TRY(pen_refuse(e, "ti_engine_serve"));
  TI_TRY(guide_refuse(e, "ti_engine_serve"));
  return serve_loop("ti_engine_serve", e, n_req, prompts, offsets, max_new, eos, chunk, nullptr, out_tokens, out_len);
}

int ti_engine_serve_sampled(ti_engine* e, int n_req, const int32_t* prompts, const int32_t* offsets, int max_new,
                            int eos, int chunk, float temperature, int top_k, float top_p, const float* draws,
                            int32_t* out_tokens, int32_t* out_len, float* out_logprobs) {
  const char* fn = "ti_engine_serve_sampled";
  if (!e || !prompts || !offsets || !draws || !out_tokens || !out_len || n_req < 1 || max_new < 1 || chunk < 1)
    return ti_set_error(TI_ERR_ARG, "%s: bad arguments", fn);
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  if (c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "%s: compat engine", fn);
  if (top_k < 1 || top_k > c.vocab) return ti_set_error(TI_ERR_ARG, "%s: top_k %d not in [1, vocab %d]", fn, top_k, c.vocab);
  for (int r = 0; r < n_req; ++r) {   // (before the sampler's buffers move)
    const int L = offsets[r + 1] - offsets[r];
    if (L < 1 || L + max_new - 1 > c.max_seq)
      return ti_set_error(TI_ERR_ARG, "%s: request %d: %d prompt + %d new tokens exceed max_seq %d", fn, r, L, max_new,
                          c.max_seq);
  }
  // what the sampled step graphs bake in, as ti_engine_generate_sampled: a chunk needs `chunk` draws per slot
  TI_TRY(grow_step_draws(e, chunk));
  TI_TRY(sampler_prepare(e, temperature, top_k, top_p, c.max_batch));
  const ServeSampler sp{draws, out_logprobs};
  return serve_loop(fn, e, n_req, prompts, offsets, max_new, eos, chunk, &sp, out_tokens, out_len);
}

}  // extern "C"

// ti_engine_serve_requests (guides null) and ti_engine_serve_requests_guided
static int serve_requests(const char* fn, ti_engine* e, int n_req, const int32_t* prompts, const int32_t* offsets,
                          const ti_request_params* params, const int32_t* guides, int chunk, const float* draws,
                          int out_stride, int32_t* out_tokens, int32_t* out_len, float* out_logprobs) {
  if (!e || !prompts || !offsets || !draws || !out_tokens || !out_len || n_req < 1 || out_stride < 1 || chunk < 1)
    return ti_set_error(TI_ERR_ARG, "%s: bad arguments", fn);
  if (!params) return ti_set_error(TI_ERR_ARG, "%s: null params", fn);
  DeviceScope bind_(e);
  const ti_engine_config& c = e->c;
  if (c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "%s: compat engine", fn);
  // (the prefix the loop will treat prompts as continuations of: one registered for fewer slots is cleared there)
  const int P = e->share_len > 0 && e->share_n == c.max_batch ? e->share_len : 0;
  for (int r = 0; r < n_req; ++r) {   // (before the sampler's buffers move)
    const ti_request_params& q = params[r];
    const int L = offsets[r + 1] - offsets[r];
    if (q.max_new < 1 || q.max_new > out_stride)
      return ti_set_error(TI_ERR_ARG, "%s: request %d: max_new %d not in [1, out_stride %d]", fn, r, q.max_new, out_stride);
    if (q.stop_token < -1 || q.stop_token >= c.vocab)
      return ti_set_error(TI_ERR_ARG, "%s: request %d: stop_token %d not in [-1, vocab %d)", fn, r, q.stop_token, c.vocab);
    if (q.top_k < 1 || q.top_k > c.vocab)
      return ti_set_error(TI_ERR_ARG, "%s: request %d: top_k %d not in [1, vocab %d]", fn, r, q.top_k, c.vocab);
    if (!(std::isfinite(q.repetition) && q.repetition > 0.0f) || !std::isfinite(q.presence) || !std::isfinite(q.frequency))
      return ti_set_error(TI_ERR_ARG, "%s: request %d: repetition %g (finite, > 0), presence %g, frequency %g (finite)", fn, r,
                          (double)q.repetition, (double)q.presence, (double)q.frequency);
    if (L < 1 || P + L + q.max_new - 1 > c.max_seq)
      return ti_set_error(TI_ERR_ARG, "%s: request %d: %d prompt + %d new tokens exceed max_seq %d", fn, r, P + L, q.max_new,
                          c.max_seq);
  }
  for (int r = 0; guides && r < n_req; ++r) {
    const int h = guides[r];
    if (h < 0 || h > TI_GUIDE_CAP)
      return ti_set_error(TI_ERR_ARG, "%s: request %d: guide handle %d not in [0, TI_GUIDE_CAP %d]", fn, r, h, TI_GUIDE_CAP);
    if (h > 0 && (e->guide_lib.empty() || !e->guide_lib[h - 1].live))
      return ti_set_error(TI_ERR_ARG, "%s: request %d: guide handle %d is not live (ti_engine_add_guide)", fn, r, h);
    if (h > 0 && e->guide_active())
      return ti_set_error(TI_ERR_UNSUPPORTED, "%s: request %d names guide handle %d (ti_engine_add_guide) while the engine's "
                          "guide is set (ti_engine_set_guide): one source of constraint per call", fn, r, h);
  }
  TI_TRY(grow_step_draws(e, chunk));   // a chunk needs `chunk` draws per slot, as in ti_engine_serve_sampled
  const ServeSampler sp{draws, out_logprobs, params, guides};
  return serve_loop(fn, e, n_req, prompts, offsets, out_stride, -1, chunk, &sp, out_tokens, out_len);
}

extern "C" {

int ti_engine_serve_requests(ti_engine* e, int n_req, const int32_t* prompts, const int32_t* offsets,
                             const ti_request_params* params, int chunk, const float* draws, int out_stride,
                             int32_t* out_tokens, int32_t* out_len, float* out_logprobs) {
  return serve_requests("ti_engine_serve_requests", e, n_req, prompts, offsets, params, nullptr, chunk, draws, out_stride,
                        out_tokens, out_len, out_logprobs);
}

int ti_engine_serve_requests_guided(ti_engine* e, int n_req, const int32_t* prompts, const int32_t* offsets,
                                    const ti_request_params* params, const int32_t* guides, int chunk, const float* draws,
                                    int out_stride, int32_t* out_tokens, int32_t* out_len, float* out_logprobs) {
  return serve_requests("ti_engine_serve_requests_guided", e, n_req, prompts, offsets, params, guides, chunk, draws,
                        out_stride, out_tokens, out_len, out_logprobs);
}

}  // extern "C"
