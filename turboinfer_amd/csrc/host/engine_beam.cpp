#include "engine_impl.hpp"

using namespace ti_eng;

// ------------------------------------------------------------------------- beam search
// InferenceEngine::generate_beam_search / beam_search_decode (inference_engine.cpp:830-871,
// 1912-2069) with the reference's control flow, scoring and container orders (max-heap on
// log_prob, std::sort on probabilities and normalised scores) and its helpers softmax /
// apply_top_k_filtering / apply_top_p_filtering (:1798-1910).
// Where the reference recomputes every candidate from scratch with a full forward pass (:1961),
// here every live beam owns a stream slot whose KV cache holds its sequence: one batched decode
// step per expansion round gives all beams' next-token logits at once, and a beam that forks
// copies its parent's cache prefix into a free slot (ti_kv_copy_slots) -- the first child
// keeps the parent's slot.  One deviation from the reference's numbers: the reference reads
// seq_len x vocab "logits" of its full-sequence forward pass as one distribution; here a
// candidate's next-token distribution is its last position's logits.

namespace {
struct Beam {
  std::vector<int32_t> tokens;
  float log_prob = 0.0f;
  float normalized_score = 0.0f;
  bool finished = false;
  int slot = -1;      // stream slot whose cache holds tokens[0 .. size-2] (its parent's, until forked)
};

std::vector<float> beam_softmax(const std::vector<float>& lg) {
  std::vector<float> p(lg.size());
  const float mx = *std::max_element(lg.begin(), lg.end());
  float sum = 0.0f;
  for (size_t i = 0; i < lg.size(); ++i) {
    p[i] = std::exp(lg[i] - mx);
    sum += p[i];
  }
  if (sum > 0.0f)
    for (auto& x : p) x /= sum;
  return p;
}

std::vector<float> beam_top_k(const std::vector<float>& probs, size_t k) {
  std::vector<float> f = probs;
  if (k >= probs.size()) return f;
  std::vector<std::pair<float, size_t>> pi;
  for (size_t i = 0; i < probs.size(); ++i) pi.emplace_back(probs[i], i);
  std::sort(pi.begin(), pi.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
  for (size_t i = k; i < pi.size(); ++i) f[pi[i].second] = 0.0f;
  float sum = 0.0f;
  for (float x : f) sum += x;
  if (sum > 0.0f)
    for (auto& x : f) x /= sum;
  return f;
}

std::vector<float> beam_top_p(const std::vector<float>& probs, float p) {
  std::vector<float> f = probs;
  if (p >= 1.0f) return f;
  std::vector<std::pair<float, size_t>> pi;
  for (size_t i = 0; i < probs.size(); ++i) pi.emplace_back(probs[i], i);
  std::sort(pi.begin(), pi.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
  float cum = 0.0f;
  std::vector<bool> in(probs.size(), false);
  for (const auto& pr : pi) {
    cum += pr.first;
    in[pr.second] = true;
    if (cum >= p) break;
  }
  for (size_t i = 0; i < probs.size(); ++i)
    if (!in[i]) f[i] = 0.0f;
  float sum = 0.0f;
  for (float x : f) sum += x;
  if (sum > 0.0f)
    for (auto& x : f) x /= sum;
  return f;
}
}  // namespace

// Copy slot `src`'s cache positions [0, n) into slot `dst`, every layer, K and V.
int ti_eng::fork_slot(ti_engine* e, int src, int dst, int n) {
  const ti_engine_config& c = e->c;
  // an e4m3 cache goes as 2-byte units: half the element counts (ti_hip.h; head_dim >= 64 keeps every
  // count a multiple of 8 units)
  const int64_t d = e->kv8 ? 2 : 1;
  return ti_kv_copy_slots(e->kv_tab, 2 * c.layers, (int64_t)src * e->kv_stride / d, (int64_t)dst * e->kv_stride / d,
                          c.kv_heads, (int64_t)c.max_seq * c.head_dim / d, (int64_t)n * c.head_dim / d, e->s);
}

extern "C" {

int ti_engine_beam_search(ti_engine* e, const int32_t* prompt, int len, int max_new, int beam_size, float temperature,
                          int top_k, float top_p, float length_penalty, int eos, int32_t* out_tokens,
                          float* out_log_prob, float* out_score, int32_t* out_finished, int* out_count) {
  if (!e || !prompt || !out_count || len < 1 || max_new < 0 || (max_new > 0 && !out_tokens))
    return ti_set_error(TI_ERR_ARG, "ti_engine_beam_search: bad arguments");
  DeviceScope bind_(e);
  if (beam_size < 1) return ti_set_error(TI_ERR_ARG, "ti_engine_beam_search: Beam size must be greater than 0");
  const ti_engine_config& c = e->c;
  if (c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_beam_search: compat engine");
  TI_TRY(pen_refuse(e, "ti_engine_beam_search"));
  TI_TRY(guide_refuse(e, "ti_engine_beam_search"));
  if (len + max_new - 1 > c.max_seq)
    return ti_set_error(TI_ERR_ARG, "ti_engine_beam_search: %d + %d tokens exceed max_seq %d", len, max_new, c.max_seq);
  TI_TRY(share_clear(e));   // (the beams' slots are rewritten from row 0)
  // More beams than stream slots: every candidate's next-token logits come from a full pass over
  // its sequence in slot 0 (prefill + one step), as the reference recomputes each candidate
  // (:1961) -- slower, same decisions.
  const bool recompute = beam_size > c.max_batch;
  const size_t V = (size_t)c.vocab;
  std::vector<float> logits((size_t)std::max(c.max_batch, beam_size) * V);
  auto cmp = [](const Beam& a, const Beam& b) { return a.log_prob < b.log_prob; };
  std::priority_queue<Beam, std::vector<Beam>, decltype(cmp)> beam(cmp);
  Beam init;
  init.tokens.assign(prompt, prompt + len);
  init.slot = 0;
  beam.push(init);
  std::vector<Beam> done;
  const size_t bs = (size_t)beam_size, target = (size_t)len + (size_t)max_new;
  std::vector<int32_t> feed(c.max_batch), pos(c.max_batch);
  for (int step = 0; step < max_new; ++step) {
    std::vector<Beam> cur;
    while (!beam.empty()) {
      cur.push_back(beam.top());
      beam.pop();
    }
    if (cur.empty()) break;
    // next-token logits of every live beam: the prompt's prefill + first step into slot 0, then
    // one batched decode step over the slots (each feeds its last token at its own position;
    // slots no beam owns decode a dummy token into their own, unused cache)
    if (recompute) {
      for (size_t i = 0; i < cur.size(); ++i) {
        cur[i].slot = (int)i;   // row of `logits`
        const int n = (int)cur[i].tokens.size();
        int32_t tok = 0;
        TI_TRY(ti_engine_generate(e, 1, cur[i].tokens.data(), &n, n, nullptr, 1, &tok, logits.data() + i * V));
      }
    } else if (step == 0) {
      int32_t tok = 0;
      TI_TRY(ti_engine_generate(e, 1, prompt, &len, len, nullptr, 1, &tok, logits.data()));
    } else {
      int M = 0;
      for (const auto& cand : cur) M = std::max(M, cand.slot + 1);
      std::fill(feed.begin(), feed.end(), 0);
      std::fill(pos.begin(), pos.end(), 0);
      for (const auto& cand : cur) {
        feed[cand.slot] = cand.tokens.back();
        pos[cand.slot] = (int32_t)cand.tokens.size() - 1;
      }
      TI_TRY(ti_engine_step(e, M, feed.data(), pos.data(), logits.data()));
    }
    std::vector<Beam> next;
    for (const auto& cand : cur) {
      if (cand.finished) {
        done.push_back(cand);
        continue;
      }
      std::vector<float> lg(logits.begin() + (size_t)cand.slot * V, logits.begin() + (size_t)(cand.slot + 1) * V);
      if (temperature != 1.0f)
        for (auto& x : lg) x /= temperature;
      std::vector<float> probs = beam_softmax(lg);
      if (top_k > 0 && (size_t)top_k < probs.size()) probs = beam_top_k(probs, (size_t)top_k);
      if (top_p < 1.0f) probs = beam_top_p(probs, top_p);
      std::vector<std::pair<float, int>> pt;
      for (size_t i = 0; i < probs.size(); ++i)
        if (probs[i] > 0.0f) pt.emplace_back(probs[i], (int)i);
      std::sort(pt.begin(), pt.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
      const size_t ex = std::min(bs, pt.size());
      for (size_t i = 0; i < ex; ++i) {
        if (pt[i].first <= 0.0f) continue;
        Beam nb = cand;
        nb.tokens.push_back(pt[i].second);
        nb.log_prob += std::log(pt[i].first);
        nb.finished = pt[i].second == eos || nb.tokens.size() >= target;
        next.push_back(std::move(nb));
      }
    }
    for (auto& b : next) b.normalized_score = b.log_prob / std::pow((float)b.tokens.size(), length_penalty);
    std::sort(next.begin(), next.end(), [](const Beam& a, const Beam& b) { return a.normalized_score > b.normalized_score; });
    const size_t keep = std::min(bs, next.size());
    // slots of the surviving beams: the first survivor of each parent keeps the parent's slot,
    // the others fork the parent's cache (positions 0 .. parent length - 1) into a free slot
    std::vector<char> owned(c.max_batch, 0);
    std::vector<size_t> forks;
    for (size_t i = 0; i < (recompute ? 0 : keep); ++i) {
      if (next[i].finished) continue;
      if (!owned[next[i].slot]) owned[next[i].slot] = 1;
      else forks.push_back(i);
    }
    int free_slot = 0;
    for (size_t i : forks) {
      while (owned[free_slot]) ++free_slot;   // a free slot exists: at most beam_size <= max_batch survivors
      TI_TRY(fork_slot(e, next[i].slot, free_slot, (int)next[i].tokens.size() - 1));
      owned[free_slot] = 1;
      next[i].slot = free_slot;
    }
    for (size_t i = 0; i < keep; ++i) {
      if (next[i].finished) done.push_back(next[i]);
      else beam.push(next[i]);
    }
    if (done.size() >= bs) break;
  }
  while (!beam.empty()) {
    Beam b = beam.top();
    beam.pop();
    b.finished = true;
    done.push_back(b);
  }
  std::sort(done.begin(), done.end(), [](const Beam& a, const Beam& b) { return a.normalized_score > b.normalized_score; });
  const size_t nres = std::min(bs, done.size());
  *out_count = (int)nres;
  for (size_t r = 0; r < nres; ++r) {
    const Beam& b = done[r];
    for (int t = 0; t < max_new; ++t) {
      const size_t j = (size_t)len + (size_t)t;
      out_tokens[r * max_new + t] = j < b.tokens.size() ? b.tokens[j] : -1;
    }
    if (out_log_prob) out_log_prob[r] = b.log_prob;
    if (out_score) out_score[r] = b.normalized_score;
    if (out_finished) out_finished[r] = b.finished ? 1 : 0;
  }
  return TI_OK;
}

}  // extern "C"
