// sampling.cpp -- host-side helpers of the decode engine that must follow the reference's
// host arithmetic exactly: the RoPE (cos, sin) table and the token sampler.
#include <algorithm>
#include <cmath>
#include <limits>
#include <utility>
#include <vector>

#include "ti_engine.h"
#include "ti_hip.h"

int ti_set_error(int code, const char* fmt, ...);

extern "C" int ti_rope_table(const float* pos, int npos, int head_dim, float theta, float* out) {
  if (!pos || !out || npos < 1 || head_dim < 2 || (head_dim & 1))
    return ti_set_error(TI_ERR_ARG, "ti_rope_table: bad arguments");
  // TensorEngine::apply_rope (src/core/tensor_engine.cpp:1561-1566, 1595-1597):
  // freq_i = 1 / pow(theta, 2i / d); angle = pos * freq_i; (cos, sin) in fp32 via libm.
  const int half = head_dim / 2;
  std::vector<float> freq((size_t)half);
  for (int i = 0; i < half; ++i) freq[i] = 1.0f / std::pow(theta, (float)(2 * i) / (float)head_dim);
  for (int p = 0; p < npos; ++p)
    for (int i = 0; i < half; ++i) {
      const float ang = pos[p] * freq[i];
      out[((size_t)p * half + i) * 2] = std::cos(ang);
      out[((size_t)p * half + i) * 2 + 1] = std::sin(ang);
    }
  return TI_OK;
}

// InferenceEngine::sample_next_token (src/model/inference_engine.cpp:1554-1673) with the
// uniform draw u passed in (the engine owns the mt19937).  Equal logits are ordered by
// libstdc++'s std::sort exactly as in the reference, which decides ties under top-k.
extern "C" int ti_sample_token(const float* logits_in, int V, float temperature, int top_k, float top_p, float u,
                               int* token, float* logprob) {
  if (!logits_in || !token || V < 1) return ti_set_error(TI_ERR_ARG, "ti_sample_token: bad arguments");
  const size_t n = (size_t)V;
  std::vector<float> lg(logits_in, logits_in + n);
  if (temperature != 1.0f && temperature > 0.0f)
    for (float& l : lg) l /= temperature;
  if (top_k > 0 && (size_t)top_k < n) {
    std::vector<std::pair<float, int>> pr;
    pr.reserve(n);
    for (size_t i = 0; i < n; ++i) pr.emplace_back(lg[i], (int)i);
    std::sort(pr.begin(), pr.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    for (size_t i = (size_t)top_k; i < n; ++i) lg[pr[i].second] = -std::numeric_limits<float>::infinity();
  }
  const float mx = *std::max_element(lg.begin(), lg.end());
  std::vector<float> p(n);
  float sum = 0.0f;
  for (size_t i = 0; i < n; ++i) {
    p[i] = std::exp(lg[i] - mx);
    sum += p[i];
  }
  for (float& x : p) x /= sum;
  if (top_p < 1.0f) {
    std::vector<std::pair<float, int>> pr;
    pr.reserve(n);
    for (size_t i = 0; i < n; ++i) pr.emplace_back(p[i], (int)i);
    std::sort(pr.begin(), pr.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    float cum = 0.0f;
    size_t cut = n;
    for (size_t i = 0; i < n; ++i) {
      cum += pr[i].first;
      if (cum >= top_p) {
        cut = i + 1;
        break;
      }
    }
    for (size_t i = cut; i < n; ++i) p[pr[i].second] = 0.0f;
    float ns = 0.0f;
    for (float x : p) ns += x;
    if (ns > 0.0f)
      for (float& x : p) x /= ns;
  }
  float cum = 0.0f;
  for (size_t i = 0; i < n; ++i) {
    cum += p[i];
    if (u <= cum) {
      *token = (int)i;
      if (logprob) *logprob = std::log(p[i]);
      return TI_OK;
    }
  }
  *token = V - 1;
  if (logprob) *logprob = std::log(p[n - 1]);
  return TI_OK;
}

// The device loops' penalties (kernels/penalty.hip) on the host: llama.cpp's llama_sampler_penalties_apply over
// the whole context, four fp32 roundings per counted token.  This file compiles with -ffp-contract=off
// (Makefile), so no step is folded into an fma: bit for bit the device's numbers.
extern "C" int ti_penalize_logits(float* logits, int V, const int32_t* context, int n, float repetition, float presence,
                                  float frequency) {
  if (!logits || V < 1 || n < 0 || (!context && n > 0))
    return ti_set_error(TI_ERR_ARG, "ti_penalize_logits: bad arguments (vocab %d, n %d)", V, n);
  if (!(std::isfinite(repetition) && repetition > 0.0f) || !std::isfinite(presence) || !std::isfinite(frequency))
    return ti_set_error(TI_ERR_ARG, "ti_penalize_logits: repetition %g (finite, > 0), presence %g, frequency %g (finite)",
                        (double)repetition, (double)presence, (double)frequency);
  if (repetition == 1.0f && presence == 0.0f && frequency == 0.0f) return TI_OK;   // off, not the identity
  std::vector<int32_t> count((size_t)V, 0);
  std::vector<int32_t> seen;
  for (int i = 0; i < n; ++i) {
    const int32_t v = context[i];
    if (v < 0 || v >= V) continue;
    if (count[(size_t)v]++ == 0) seen.push_back(v);
  }
  for (const int32_t v : seen) {
    const float l = logits[v];
    const float a = l <= 0.0f ? l * repetition : l / repetition;
    const float b = (float)count[(size_t)v] * frequency;
    const float d = b + presence;
    logits[v] = a - d;
  }
  return TI_OK;
}

// Guided decoding (kernels/guide.hip) on the host: the contract of ti_engine.h ti_guide, validated here ...
extern "C" int ti_guide_check(const ti_guide* g, int V) {
  const char* fn = "ti_guide_check";
  if (!g || !g->row_ptr) return ti_set_error(TI_ERR_ARG, "%s: null guide or row_ptr", fn);
  if (V < 1) return ti_set_error(TI_ERR_ARG, "%s: vocab %d", fn, V);
  const int n = g->n_states;
  if (n < 1) return ti_set_error(TI_ERR_ARG, "%s: n_states %d < 1", fn, n);
  if (g->start < 0 || g->start >= n) return ti_set_error(TI_ERR_ARG, "%s: start %d outside [0, n_states %d)", fn, g->start, n);
  if (g->row_ptr[0] != 0) return ti_set_error(TI_ERR_ARG, "%s: row_ptr[0] = %lld, not 0", fn, (long long)g->row_ptr[0]);
  if (!g->tokens || !g->next) return ti_set_error(TI_ERR_ARG, "%s: null tokens or next", fn);
  for (int s = 0; s < n; ++s) {   // (before any list is read: a monotone row_ptr keeps every index below nnz)
    if (g->row_ptr[s + 1] < g->row_ptr[s]) return ti_set_error(TI_ERR_ARG, "%s: row_ptr decreases at state %d", fn, s);
    if (g->row_ptr[s + 1] == g->row_ptr[s]) return ti_set_error(TI_ERR_ARG, "%s: state %d has no transition", fn, s);
  }
  for (int s = 0; s < n; ++s) {
    const int64_t b = g->row_ptr[s], e = g->row_ptr[s + 1];
    for (int64_t i = b; i < e; ++i) {
      const int32_t v = g->tokens[i], nx = g->next[i];
      if (v < 0 || v >= V) return ti_set_error(TI_ERR_ARG, "%s: state %d: token %d outside [0, vocab %d)", fn, s, v, V);
      if (i > b && v <= g->tokens[i - 1])
        return ti_set_error(TI_ERR_ARG, "%s: state %d: token %d after %d (strictly ascending ids)", fn, s, v, g->tokens[i - 1]);
      if (nx < 0 || nx >= n) return ti_set_error(TI_ERR_ARG, "%s: state %d: next %d outside [0, n_states %d)", fn, s, nx, n);
    }
  }
  return TI_OK;
}

// ... and applied to one host row: the advance by the fed token, then -inf at every id the state does not allow.
extern "C" int ti_guide_apply(const ti_guide* g, int V, int state, int fed_token, float* logits, int* out_state) {
  if (!g || !g->row_ptr || !g->tokens || !g->next || V < 1 || g->n_states < 1 || state < -1 || state >= g->n_states ||
      fed_token < -1)
    return ti_set_error(TI_ERR_ARG, "ti_guide_apply: bad arguments (vocab %d, state %d, fed_token %d)", V, state, fed_token);
  int s = state;
  if (s >= 0 && fed_token >= 0) {
    const int32_t* b = g->tokens + g->row_ptr[s];
    const int32_t* e = g->tokens + g->row_ptr[s + 1];
    const int32_t* at = std::lower_bound(b, e, (int32_t)fed_token);
    s = at != e && *at == fed_token ? g->next[at - g->tokens] : -1;
  }
  if (out_state) *out_state = s;
  if (s < 0 || !logits) return TI_OK;
  int64_t i = g->row_ptr[s];
  const int64_t end = g->row_ptr[s + 1];
  for (int v = 0; v < V; ++v) {
    if (i < end && g->tokens[i] == v) ++i;
    else logits[v] = -std::numeric_limits<float>::infinity();
  }
  return TI_OK;
}
