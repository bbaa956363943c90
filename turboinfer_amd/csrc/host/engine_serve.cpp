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
struct ServeSampler {
  const float* draws;   // host [n_req][max_new]
  float* out_logprobs;  // host [n_req][max_new], nullable
};

static int serve_loop(const char* fn, ti_engine* e, int n_req, const int32_t* prompts, const int32_t* offsets,
                      int max_new, int eos, int chunk, const ServeSampler* sp, int32_t* out_tokens, int32_t* out_len) {
  const ti_engine_config& c = e->c;
  const int B = c.max_batch;
  // A prefix registered for every slot (ti_engine_share_prefix with n_streams == max_batch): each prompt is the
  // continuation behind it, every slot -- idle ones too -- sits at or past P and never touches its copy of the
  // prefix, so a freed slot is reused without a new copy.  Registered for fewer slots: cleared.  P = 0: as ever.
  if (e->share_len > 0 && e->share_n != B) TI_TRY(share_clear(e));
  const int P = e->share_len;
  int max_len = 1;
  for (int r = 0; r < n_req; ++r) {
    const int L = offsets[r + 1] - offsets[r];
    if (L < 1 || P + L + max_new - 1 > c.max_seq)
      return ti_set_error(TI_ERR_ARG, "%s: request %d: %d prompt + %d new tokens exceed max_seq %d", fn, r, P + L, max_new,
                          c.max_seq);
    max_len = std::max(max_len, L);
  }
  const bool pen = sp && e->pen_active();   // (the greedy loop is refused while they are active)
  const bool guide = sp && e->guide_active();
  const StepMode mode{true, sp != nullptr, P > 0 && B >= 2 && P >= e->share_min, pen || guide};
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
        if (pen) TI_TRY(pen_reset_slot(e, m, e->share_tokens.data(), P, prompts + offsets[slot_req[m]], L));
        if (guide) TI_TRY(guide_start_slots(e, m, 1));   // a freed slot restarts at the guide's start state
      }
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
        const int nd = std::min(S, max_new - out_len[r]);
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
        if (out_len[r] >= max_new || tok == eos) {
          slot_req[m] = -1;
          --live;
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
