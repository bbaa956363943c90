// inference_engine.cpp -- turboinfer::model::InferenceEngine on MI355X.
//
// InferenceEngineImpl (the reference's pimpl, inference_engine.hpp:214) owns one
// ti_engine (include/ti_engine.h): weights resolved by the reference's names
// (inference_engine.cpp:483-563) and uploaded once, KV / activations / step graph on the
// device.  Host logic here: the generate() contract (:734-802), batch validation
// (:1409-1427), sampling (:1554-1673, via ti_sample_token), statistics (:1014-1150).
#include "turboinfer/model/inference_engine.hpp"

#include <algorithm>
#include <map>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <iomanip>
#include <random>
#include <sstream>
#include <stdexcept>

#include "api_common.hpp"
#include "ti_engine.h"
#include "ti_hip.h"

namespace turboinfer {
namespace model {

using api::check;

namespace {

// generate()'s end-of-sequence token: the reference tests `next_token == 2` (inference_engine.cpp:759-760),
// not config.eos_token_id (which only its beam search reads, :2015)
constexpr int kGenerateEos = 2;

// The reference's public layouts are kept (a program built against its headers links against
// this library): InferenceConfig has no room for the MI355X options, so they come from the model's
// extra_params, then the environment, then the default (inference_engine.hpp header note).
static_assert(sizeof(InferenceConfig) == 48 && sizeof(GenerationResult) == 96, "reference layout (LP64)");
static_assert(sizeof(InferenceEngine) == 400, "reference layout (LP64)");
int engine_option(const ModelMetadata& md, const char* key, const char* env, int dflt) {
  const auto it = md.extra_params.find(key);
  if (it != md.extra_params.end()) return std::atoi(it->second.c_str());
  if (const char* v = std::getenv(env)) return std::atoi(v);
  return dflt;
}

// "turboinfer.kv_bits" / TI_KV_BITS: 16 (fp16 KV cache, the default) or 8 (e4m3, TI_BITS_KV8); any other value throws.
int kv_bits_option(const ModelMetadata& md) {
  const int b = engine_option(md, "turboinfer.kv_bits", "TI_KV_BITS", 16);
  if (b != 8 && b != 16) throw std::runtime_error("InferenceEngine: kv_bits must be 8 (e4m3 KV cache) or 16 (fp16)");
  return b;
}

// "turboinfer.lookahead" / TI_LOOKAHEAD: n-gram drafts verified per step by a request that runs alone, greedy
// (ti_engine_generate_lookahead) or sampled (ti_engine_generate_lookahead_sampled); 0 (the default) = off, up to
// 15; not with the e4m3 KV cache.
// TI_BATCH_SAMPLE_DEVICE=0: generate_batch keeps groups of sampled requests on the host-sampler loop (A/B knob)
bool batch_sample_device() {
  const char* v = std::getenv("TI_BATCH_SAMPLE_DEVICE");
  return v ? std::atoi(v) != 0 : true;
}

int lookahead_option(const ModelMetadata& md, int kv_bits) {
  const int k = engine_option(md, "turboinfer.lookahead", "TI_LOOKAHEAD", 0);
  if (k < 0 || k > TI_LA_MAX_K) throw std::runtime_error("InferenceEngine: lookahead must be 0 (off) .. 15 drafts per step");
  if (k > 0 && kv_bits == 8) throw std::runtime_error("InferenceEngine: lookahead needs the fp16 KV cache (kv_bits 16)");
  return k;
}

// "turboinfer.share_prefix" / TI_SHARE_PREFIX: n > 0 -- a device-loop group of generate_batch (two or more requests)
// whose prompts share a token prefix of at least n tokens registers it (ti_engine_share_prefix: prefilled once,
// attended once per step for all streams) and passes the continuations; 0 (the default) = off; negative throws;
// not with the e4m3 KV cache.
int share_prefix_option(const ModelMetadata& md, int kv_bits) {
  const int n = engine_option(md, "turboinfer.share_prefix", "TI_SHARE_PREFIX", 0);
  if (n < 0) throw std::runtime_error("InferenceEngine: share_prefix must be 0 (off) or a prefix length in tokens");
  if (n > 0 && kv_bits == 8) throw std::runtime_error("InferenceEngine: share_prefix needs the fp16 KV cache (kv_bits 16)");
  return n;
}

// "turboinfer.repetition_penalty" / TI_REPETITION_PENALTY (default 1), "turboinfer.presence_penalty" /
// TI_PRESENCE_PENALTY and "turboinfer.frequency_penalty" / TI_FREQUENCY_PENALTY (default 0): the penalties of
// ti_engine_set_penalties over each request's whole context (the reference's GenerationConfig has no such fields).
// Parsed as floats; anything else, a repetition that is not finite and > 0 or a non-finite presence / frequency
// throws.  Active (values other than 1, 0, 0): generate / generate_batch always take the sampled device loop (a
// greedy config runs top_k = 1), the host-sampler loop applies ti_penalize_logits, beam search throws.
float float_option(const ModelMetadata& md, const char* key, const char* env, float dflt) {
  const char* v = nullptr;
  const auto it = md.extra_params.find(key);
  if (it != md.extra_params.end()) v = it->second.c_str();
  else v = std::getenv(env);
  if (!v) return dflt;
  char* end = nullptr;
  const float f = std::strtof(v, &end);
  while (end && (*end == ' ' || *end == '\t')) ++end;
  if (end == v || *end != '\0' || !std::isfinite(f))
    throw std::runtime_error(std::string("InferenceEngine: ") + key + " must be a finite number, not \"" + v + "\"");
  return f;
}

struct Penalties {
  float repetition = 1.0f, presence = 0.0f, frequency = 0.0f;
  bool active() const { return repetition != 1.0f || presence != 0.0f || frequency != 0.0f; }
};

Penalties penalty_options(const ModelMetadata& md, int lookahead, bool compat) {
  Penalties p;
  p.repetition = float_option(md, "turboinfer.repetition_penalty", "TI_REPETITION_PENALTY", 1.0f);
  p.presence = float_option(md, "turboinfer.presence_penalty", "TI_PRESENCE_PENALTY", 0.0f);
  p.frequency = float_option(md, "turboinfer.frequency_penalty", "TI_FREQUENCY_PENALTY", 0.0f);
  if (!(p.repetition > 0.0f)) throw std::runtime_error("InferenceEngine: repetition_penalty must be greater than 0");
  if (p.active() && lookahead > 0)
    throw std::runtime_error("InferenceEngine: penalties and lookahead exclude each other (the verify rows are not penalised)");
  if (p.active() && compat)
    throw std::runtime_error("InferenceEngine: penalties need the device engine, not the reference_compat plumbing model");
  return p;
}

// "turboinfer.guide_file" / TI_GUIDE_FILE: a token automaton for guided decoding (ti_engine_set_guide)
// in a little-endian file: magic "TIGD", int32 version 1, int32 n_states, int32 start, int64 nnz,
// int64 row_ptr[n_states + 1], int32 tokens[nnz], int32 next[nnz].  With a guide generate / generate_batch always
// take the sampled device loop (a greedy config runs top_k = 1), the host-sampler loop applies ti_guide_apply, beam
// search and lookahead throw; an unreadable or malformed file throws naming the reason (the automaton itself is
// validated by ti_engine_set_guide against the model's vocabulary).
struct GuideFile {
  std::vector<int64_t> row_ptr;
  std::vector<int32_t> tokens, next;
  int32_t n_states = 0, start = 0;
  bool active() const { return n_states > 0; }
  ti_guide view() const { return ti_guide{n_states, start, row_ptr.data(), tokens.data(), next.data()}; }
};

GuideFile guide_option(const ModelMetadata& md, int lookahead, bool compat) {
  GuideFile g;
  std::string path;
  const auto it = md.extra_params.find("turboinfer.guide_file");
  if (it != md.extra_params.end()) path = it->second;
  else if (const char* v = std::getenv("TI_GUIDE_FILE")) path = v;
  if (path.empty()) return g;
  auto fail = [&](const std::string& why) -> void {
    throw std::runtime_error("InferenceEngine: guide_file \"" + path + "\": " + why);
  };
  if (lookahead > 0) fail("a guide and lookahead exclude each other (the verify rows are not guided)");
  if (compat) fail("a guide needs the device engine, not the reference_compat plumbing model");
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) fail("cannot be opened");
  struct Close {
    std::FILE* f;
    ~Close() { std::fclose(f); }
  } close_{f};
  char magic[4];
  int32_t head[3];
  int64_t nnz = 0;
  if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "TIGD", 4) != 0) fail("no TIGD magic");
  if (std::fread(head, 4, 3, f) != 3 || std::fread(&nnz, 8, 1, f) != 1) fail("truncated header");
  if (head[0] != 1) fail("version " + std::to_string(head[0]) + ", expected 1");
  if (head[1] < 1 || nnz < 1 || nnz > ((int64_t)1 << 40)) fail("n_states " + std::to_string(head[1]) + ", nnz " + std::to_string(nnz));
  g.row_ptr.resize((size_t)head[1] + 1);
  if (std::fread(g.row_ptr.data(), 8, g.row_ptr.size(), f) != g.row_ptr.size()) fail("truncated row_ptr");
  if (g.row_ptr.back() != nnz) fail("row_ptr ends at " + std::to_string(g.row_ptr.back()) + ", nnz is " + std::to_string(nnz));
  g.tokens.resize((size_t)nnz);
  g.next.resize((size_t)nnz);
  if (std::fread(g.tokens.data(), 4, (size_t)nnz, f) != (size_t)nnz || std::fread(g.next.data(), 4, (size_t)nnz, f) != (size_t)nnz)
    fail("truncated tokens / next");
  g.n_states = head[1];
  g.start = head[2];
  return g;
}

[[noreturn]] void off_path(const std::string& what, const char* row) {
  throw std::runtime_error("InferenceEngine::" + what + ": not part of the MI355X decode hot path (SURVEY.md 8(f) " +
                           row + ")");
}

const core::Tensor* find(const ModelData& m, std::initializer_list<std::string> names) {
  for (const auto& n : names)
    if (const core::Tensor* t = m.get_tensor(n)) return t;
  return nullptr;
}

const core::Tensor* layer_tensor(const ModelData& m, size_t l, const char* hf, const char* meta) {
  const std::string a = "model.layers." + std::to_string(l) + ".", b = "layers." + std::to_string(l) + ".";
  return find(m, {a + hf, b + meta, b + hf});
}

// A ModelData read from a llama GGUF (ModelLoader::load) carries llama.cpp's
// tensor names and [out][in] linear weights; the engine takes the reference's names and [in][out]
// (ti_engine.h slots).  llama.cpp's q / k rows are already ordered for adjacent-pair RoPE, the
// rotation apply_rope implements (tensor_engine.cpp:1602-1612), so only names and the transpose
// change.  A file without output.weight ties the lm_head to the embedding.
bool gguf_named(const ModelData& m) { return m.get_tensor("blk.0.ffn_up.weight") != nullptr; }

core::Tensor transposed_f32(const core::Tensor& t) {
  if (t.shape().ndim() != 2) throw std::runtime_error("InferenceEngine: GGUF linear weight is not 2-D");
  const size_t r = t.shape().size(0), c = t.shape().size(1);
  const std::vector<float> v = api::to_f32(t);
  core::Tensor o(core::TensorShape({c, r}), core::DataType::kFloat32);
  float* d = o.data_ptr<float>();
  for (size_t i = 0; i < r; ++i)
    for (size_t j = 0; j < c; ++j) d[j * r + i] = v[i * c + j];
  return o;
}

ModelData from_gguf_names(const ModelData& g) {
  ModelData m;
  m.metadata() = g.metadata();
  auto need = [&](const std::string& n) -> const core::Tensor& {
    const core::Tensor* t = g.get_tensor(n);
    if (!t) throw std::runtime_error("InferenceEngine: GGUF model lacks " + n);
    return *t;
  };
  m.add_tensor("token_embeddings.weight", need("token_embd.weight"));
  // older converters omit llama.vocab_size: the embedding's rows are the vocabulary
  const core::Tensor& emb = need("token_embd.weight");
  if (m.metadata().vocab_size == 0 && emb.shape().ndim() == 2) m.metadata().vocab_size = emb.shape().size(0);
  m.add_tensor("norm.weight", need("output_norm.weight"));
  const core::Tensor* out = g.get_tensor("output.weight");
  m.add_tensor("lm_head.weight", transposed_f32(out ? *out : need("token_embd.weight")));
  for (size_t l = 0; l < g.metadata().num_layers; ++l) {
    const std::string b = "blk." + std::to_string(l) + ".", r = "layers." + std::to_string(l) + ".";
    m.add_tensor(r + "attention.q_proj.weight", transposed_f32(need(b + "attn_q.weight")));
    m.add_tensor(r + "attention.k_proj.weight", transposed_f32(need(b + "attn_k.weight")));
    m.add_tensor(r + "attention.v_proj.weight", transposed_f32(need(b + "attn_v.weight")));
    m.add_tensor(r + "attention.o_proj.weight", transposed_f32(need(b + "attn_output.weight")));
    m.add_tensor(r + "feed_forward.w3.weight", transposed_f32(need(b + "ffn_gate.weight")));
    m.add_tensor(r + "feed_forward.w1.weight", transposed_f32(need(b + "ffn_up.weight")));
    m.add_tensor(r + "feed_forward.w2.weight", transposed_f32(need(b + "ffn_down.weight")));
    m.add_tensor(r + "attention_norm.weight", need(b + "attn_norm.weight"));
    m.add_tensor(r + "ffn_norm.weight", need(b + "ffn_norm.weight"));
  }
  return m;
}

// GGUF Q4_0 / Q8_0 checkpoints reach the engine as ggml dequantizes them (gguf.cpp): every
// 32-weight block along K of an output column is d * q with d fp16 and q an integer of
// [-8, 7] (Q4_0) or [-127, 127] (Q8_0).  Recover (q, d) exactly from the fp32 values so the
// engine holds the checkpoint's blocks as they are (group-32 tiles, TI_BITS_G32) instead of
// re-quantizing them per 128.  ggml's quantizers put the block's largest magnitude at q = -8
// (Q4_0, d = max / -8) or |q| = 127 (Q8_0), so the first candidate nearly always fits.
bool recover_g32(const std::vector<float>& w, size_t K, size_t N, int bits, std::vector<int8_t>& q,
                 std::vector<uint16_t>& d) {
  if (K % 32 || w.size() != K * N) return false;
  const int lo = bits == 4 ? -8 : -127, hi = bits == 4 ? 7 : 127;
  q.assign(K * N, 0);
  d.assign(K / 32 * N, 0);
  auto half_bits = [](float f) {
    const _Float16 h = (_Float16)f;
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
  };
  auto half_val = [](uint16_t u) {
    _Float16 h;
    std::memcpy(&h, &u, 2);
    return (float)h;
  };
  std::vector<float> cand;
  for (size_t n = 0; n < N; ++n)
    for (size_t b = 0; b < K / 32; ++b) {
      float xm = 0.0f;
      for (size_t k = 32 * b; k < 32 * b + 32; ++k)
        if (std::fabs(w[k * N + n]) > std::fabs(xm)) xm = w[k * N + n];
      if (xm == 0.0f) continue;   // all zero: q = 0, d = 0
      cand.clear();
      const float sgn = xm > 0.0f ? 1.0f : -1.0f, a = std::fabs(xm);
      if (bits == 4) {
        cand.push_back(-sgn * a / 8.0f);
        for (int j = 7; j >= 1; --j) {
          cand.push_back(sgn * a / (float)j);
          cand.push_back(-sgn * a / (float)j);
        }
      } else {
        for (int j = 127; j >= 1; --j) cand.push_back(a / (float)j);
      }
      bool found = false;
      for (float c : cand) {
        const uint16_t dh = half_bits(c);
        const float dd = half_val(dh);
        if (dd == 0.0f || !std::isfinite(dd)) continue;
        bool ok = true;
        for (size_t k = 32 * b; k < 32 * b + 32 && ok; ++k) {
          const float x = w[k * N + n], r = std::rint(x / dd);
          ok = r >= (float)lo && r <= (float)hi && r * dd == x;
        }
        if (!ok) continue;
        for (size_t k = 32 * b; k < 32 * b + 32; ++k) q[k * N + n] = (int8_t)std::rint(w[k * N + n] / dd);
        d[b * N + n] = dh;
        found = true;
        break;
      }
      if (!found) return false;
    }
  return true;
}

// GGUF Q4_1 checkpoints likewise: every block is fl(q * d + m) with q in [0, 15] and d, m fp16
// (gguf.cpp dequant_q4_1).  ggml's Q4_1 quantizer maps the block minimum to q = 0 (so m is the
// smallest value, exactly) and the maximum to q = 15; d is the fp16 nearest (max - m) / 15 or
// one of its neighbours.  Every candidate is verified weight by weight.
bool recover_q41(const std::vector<float>& w, size_t K, size_t N, std::vector<int8_t>& q, std::vector<uint16_t>& d,
                 std::vector<uint16_t>& m) {
  if (K % 32 || w.size() != K * N) return false;
  q.assign(K * N, 0);
  d.assign(K / 32 * N, 0);
  m.assign(K / 32 * N, 0);
  auto half_bits = [](float f) {
    const _Float16 h = (_Float16)f;
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
  };
  auto half_val = [](uint16_t u) {
    _Float16 h;
    std::memcpy(&h, &u, 2);
    return (float)h;
  };
  for (size_t n = 0; n < N; ++n)
    for (size_t b = 0; b < K / 32; ++b) {
      float lo = INFINITY, hi = -INFINITY;
      for (size_t k = 32 * b; k < 32 * b + 32; ++k) {
        lo = std::min(lo, w[k * N + n]);
        hi = std::max(hi, w[k * N + n]);
      }
      const uint16_t mh = half_bits(lo);
      if (half_val(mh) != lo) return false;
      m[b * N + n] = mh;
      if (hi == lo) continue;   // constant block: q = 0, d = 0
      const uint16_t d0 = half_bits((hi - lo) / 15.0f);
      bool found = false;
      for (int dj : {0, 1, -1, 2, -2}) {
        const uint16_t dh = (uint16_t)(d0 + dj);
        const float dd = half_val(dh);
        if (!(dd > 0.0f) || !std::isfinite(dd)) continue;
        bool ok = true;
        for (size_t k = 32 * b; k < 32 * b + 32 && ok; ++k) {
          const float x = w[k * N + n], r = std::rint((x - lo) / dd);
          ok = r >= 0.0f && r <= 15.0f && r * dd + lo == x;
        }
        if (!ok) continue;
        for (size_t k = 32 * b; k < 32 * b + 32; ++k) q[k * N + n] = (int8_t)std::rint((w[k * N + n] - lo) / dd);
        d[b * N + n] = dh;
        found = true;
        break;
      }
      if (!found) return false;
    }
  return true;
}

bool is_int(const core::Tensor& t) {
  return t.dtype() == core::DataType::kInt8 || t.dtype() == core::DataType::kInt32 ||
         t.dtype() == core::DataType::kInt16 || t.dtype() == core::DataType::kUInt8;
}

}  // namespace

class InferenceEngineImpl {
 public:
  ti_engine* eng = nullptr;
  ti_engine_config cfg{};
  int capacity = 1;      // streams one device call holds
  int kv_bits = 16;      // 8: e4m3 KV cache (TI_BITS_KV8 at ti_engine_create; cfg.bits stays the weight format)
  int lookahead = 0;     // > 0: a request that runs alone (greedy or sampled) verifies this many n-gram drafts per step
  int share_prefix = 0;  // > 0: a device-loop group whose prompts share at least this many leading tokens registers them
  Penalties pen;         // active: every request runs the sampled device loop under ti_engine_set_penalties
  GuideFile guide;       // active: every request runs the sampled device loop under ti_engine_set_guide
  bool compat = false;
  std::mt19937 rng;
  size_t total_generations = 0, total_tokens = 0, total_forward_passes = 0;
  float total_time_ms = 0.0f, peak_tps = 0.0f;

  bool gguf_src = false;  // built from a GGUF-read ModelData (llama.cpp names)
  // group-32 blocks recovered per linear weight (recover_g32 / recover_q41), reused by upload()
  struct Blocks {
    std::vector<int8_t> q;
    std::vector<uint16_t> d, m;   // m: Q4_1 block minimums
  };
  std::map<const core::Tensor*, Blocks> g32;

  static bool recover(const std::vector<float>& w, size_t K, size_t N, int bits, Blocks& b) {
    return (bits & TI_BITS_AFF) ? recover_q41(w, K, N, b.q, b.d, b.m)
                                : recover_g32(w, K, N, bits & ~TI_BITS_G32, b.q, b.d);
  }

  InferenceEngineImpl() { rng.seed((unsigned)std::chrono::steady_clock::now().time_since_epoch().count()); }

  // every linear weight of the model is exact group-32 blocks of `bits` (4 | G32, 8 | G32 or
  // 4 | G32 | AFF; cached on success)
  bool all_g32(const ModelData& m, size_t L, size_t H, size_t qd, size_t kvd, size_t I, size_t V, int bits) {
    g32.clear();
    auto one = [&](const core::Tensor* t, size_t K, size_t N) {
      if (!t || t->shape().total_size() != K * N) return false;
      return recover(api::to_f32(*t), K, N, bits, g32[t]);
    };
    bool ok = one(find(m, {"lm_head.weight", "output.weight"}), H, V);
    for (size_t l = 0; l < L && ok; ++l)
      ok = one(layer_tensor(m, l, "self_attn.q_proj.weight", "attention.q_proj.weight"), H, qd) &&
           one(layer_tensor(m, l, "self_attn.k_proj.weight", "attention.k_proj.weight"), H, kvd) &&
           one(layer_tensor(m, l, "self_attn.v_proj.weight", "attention.v_proj.weight"), H, kvd) &&
           one(layer_tensor(m, l, "self_attn.o_proj.weight", "attention.o_proj.weight"), qd, H) &&
           one(layer_tensor(m, l, "mlp.gate_proj.weight", "feed_forward.w3.weight"), H, I) &&
           one(layer_tensor(m, l, "mlp.up_proj.weight", "feed_forward.w1.weight"), H, I) &&
           one(layer_tensor(m, l, "mlp.down_proj.weight", "feed_forward.w2.weight"), I, H);
    if (!ok) g32.clear();
    return ok;
  }
  ~InferenceEngineImpl() {
    if (eng) ti_engine_destroy(eng);
  }

  void upload(int slot, int layer, const core::Tensor& t, size_t K, size_t N, int bits) {
    if ((bits & TI_BITS_G32) && t.shape().total_size() == K * N) {   // exact blocks when the weight has them
      auto it = g32.find(&t);
      Blocks b;
      if (it != g32.end()) {
        b = std::move(it->second);
        g32.erase(it);
      }
      if (!b.q.empty() || recover(api::to_f32(t), K, N, bits, b)) {
        if (bits & TI_BITS_AFF)
          check(ti_engine_set_tensor_q1(eng, slot, layer, reinterpret_cast<const uint8_t*>(b.q.data()), b.d.data(),
                                        b.m.data()),
                "ti_engine_set_tensor_q1");
        else
          check(ti_engine_set_tensor_q(eng, slot, layer, b.q.data(), b.d.data()), "ti_engine_set_tensor_q");
        return;
      }
    }   // otherwise quantized below (ggml's Q4_1 rounding on affine engines, ti_wpack_host)
    if (t.shape().total_size() != K * N)
      throw std::runtime_error("InferenceEngine: weight for slot " + std::to_string(slot) + " layer " +
                               std::to_string(layer) + " has " + std::to_string(t.shape().total_size()) +
                               " elements, expected " + std::to_string(K) + "x" + std::to_string(N));
    const std::vector<float> v = api::to_f32(t);
    int mode = TI_SCALE_GROUP;
    if (is_int(t)) {
      mode = TI_SCALE_UNIT;   // Quantizer output: the reference multiplies the raw integers (convert_dtype)
      const float lo = bits == 4 ? -8.0f : -128.0f, hi = bits == 4 ? 7.0f : 127.0f;
      if (bits != 16)
        for (float x : v)
          if (x < lo || x > hi)
            throw std::runtime_error("InferenceEngine: integer weight value " + std::to_string(x) +
                                     " does not fit the " + std::to_string(bits) + "-bit tiles");
    }
    check(ti_engine_set_tensor(eng, slot, layer, v.data(), mode), "ti_engine_set_tensor");
  }

  void upload_vec(int slot, int layer, const core::Tensor& t, size_t n) {
    if (t.shape().total_size() != n)
      throw std::runtime_error("InferenceEngine: vector for slot " + std::to_string(slot) + " has " +
                               std::to_string(t.shape().total_size()) + " elements, expected " + std::to_string(n));
    const std::vector<float> v = api::to_f32(t);
    check(ti_engine_set_tensor(eng, slot, layer, v.data(), TI_SCALE_UNIT), "ti_engine_set_tensor");
  }

  // The device engine of cfg (filled in by the caller but for the stream capacity).
  void create(const InferenceConfig& c) {
    cfg.attn_splits = 0;
    if (compat) kv_bits = 16;   // the plumbing model has no KV cache
    // streams held at once: the configured batch, bounded to 64 GiB of KV
    const double kv_stream = 2.0 * cfg.layers * cfg.kv_heads * cfg.head_dim * (kv_bits / 8.0) * cfg.max_seq;
    capacity = (int)std::max<size_t>(1, std::min<size_t>(c.max_batch_size, (size_t)(64.0 * (1ull << 30) / kv_stream)));
    capacity = std::min(capacity, 64);
    cfg.max_batch = compat ? 1 : capacity;
    check(ti_init(cfg.device), "ti_init");
    ti_engine_config ec = cfg;
    if (kv_bits == 8) ec.bits |= TI_BITS_KV8;
    check(ti_engine_create(&ec, &eng), "ti_engine_create");
    // generate() ends its device loop at EOS (token id 2, inference_engine.cpp:759-764)
    if (!compat) check(ti_engine_set_stop(eng, kGenerateEos), "ti_engine_set_stop");
    if (pen.active()) check(ti_engine_set_penalties(eng, pen.repetition, pen.presence, pen.frequency), "ti_engine_set_penalties");
    if (guide.active()) {
      const ti_guide g = guide.view();
      check(ti_engine_set_guide(eng, &g), "ti_engine_set_guide");
    }
  }

  // Metadata without tensors (the reference's own test programs build engines this way and run
  // them on its placeholder fallbacks, inference_engine.cpp:293-296, 377-380, 672-684): the
  // engine's seeded synthetic llama model of that shape (ti_engine_synth), INT4 unless the
  // weight_bits option says 8 or 16.
  void build_synthetic(const ModelMetadata& md, const InferenceConfig& c, int gpu) {
    const int H = (int)md.hidden_size, nh = (int)md.num_heads;
    cfg.vocab = (int)md.vocab_size;
    cfg.hidden = H;
    cfg.layers = (int)md.num_layers;
    cfg.heads = nh;
    cfg.kv_heads = nh;
    cfg.head_dim = H / nh;
    cfg.inter = md.intermediate_size ? (int)md.intermediate_size : 4 * H;
    cfg.rope_theta = md.rope_theta > 0.0f ? md.rope_theta : 10000.0f;
    cfg.eps = 1e-5f;
    const int bits = engine_option(md, "turboinfer.weight_bits", "TI_WEIGHT_BITS", 0);
    cfg.bits = bits == 8 || bits == 16 ? bits : 4;
    kv_bits = kv_bits_option(md);
    lookahead = lookahead_option(md, kv_bits);
    share_prefix = share_prefix_option(md, kv_bits);
    pen = penalty_options(md, lookahead, false);
    guide = guide_option(md, lookahead, false);
    cfg.max_seq = (int)std::max<size_t>(1, c.max_sequence_length);
    cfg.compat = 0;
    cfg.device = gpu;
    compat = false;
    create(c);
    check(ti_engine_synth(eng, 0x7475726269ull, 0.0f), "ti_engine_synth");
  }

  void build(const ModelData& m, const InferenceConfig& c) {
    if (gguf_named(m)) {
      gguf_src = true;
      return build(from_gguf_names(m), c);
    }
    const ModelMetadata& md = m.metadata();
    const size_t H = md.hidden_size, L = md.num_layers, nh = md.num_heads, V = md.vocab_size;
    size_t I = md.intermediate_size;
    if (!H || !L || !nh || !V || H % nh) throw std::runtime_error("InferenceEngine: incomplete model metadata");
    const size_t hd = H / nh;
    const int gpu = engine_option(md, "turboinfer.gpu_index", "TI_GPU_INDEX", 0);
    if (m.num_tensors() == 0) {
      // a tensorless ModelData (what the reference's test programs build) runs the seeded synthetic
      // model of that shape only when asked: otherwise a checkpoint that failed to load would decode
      // plausible-looking tokens from random weights
      if (engine_option(md, "turboinfer.synthetic", "TI_SYNTHETIC", 0) != 1)
        throw std::runtime_error("InferenceEngine: the model has metadata but no tensors (set "
                                 "extra_params[\"turboinfer.synthetic\"] = \"1\" or TI_SYNTHETIC=1 for the "
                                 "seeded synthetic model of this shape)");
      return build_synthetic(md, c, gpu);
    }
    const core::Tensor* q0 = layer_tensor(m, 0, "self_attn.q_proj.weight", "attention.q_proj.weight");
    const core::Tensor* k0 = layer_tensor(m, 0, "self_attn.k_proj.weight", "attention.k_proj.weight");
    const core::Tensor* up0 = layer_tensor(m, 0, "mlp.up_proj.weight", "feed_forward.w1.weight");
    const core::Tensor* lm = find(m, {"lm_head.weight", "output.weight"});
    if (!up0 || !lm) throw std::runtime_error("InferenceEngine: model has no FFN up / lm_head weights");
    if (!I) I = up0->shape().total_size() / H;
    compat = (q0 == nullptr);

    // weight format
    int bits = engine_option(md, "turboinfer.weight_bits", "TI_WEIGHT_BITS", 0);
    if (bits == 0) {
      bits = 16;
      if (is_int(*up0)) {
        bits = up0->dtype() == core::DataType::kInt32 ? 4 : 8;
        const std::vector<float> v = api::to_f32(*up0);
        for (float x : v)
          if (x < -8.0f || x > 7.0f) bits = 8;
      } else if (gguf_src && q0) {   // Q4_0 / Q4_1 / Q8_0 checkpoint: keep its blocks
        const size_t kvd = k0 ? k0->shape().total_size() / H : H;
        if (all_g32(m, L, H, H, kvd, I, V, 4 | TI_BITS_G32)) bits = 4 | TI_BITS_G32;
        else if (all_g32(m, L, H, H, kvd, I, V, 4 | TI_BITS_G32 | TI_BITS_AFF)) bits = 4 | TI_BITS_G32 | TI_BITS_AFF;
        else if (all_g32(m, L, H, H, kvd, I, V, 8 | TI_BITS_G32)) bits = 8 | TI_BITS_G32;
      }
    }
    if (bits != 4 && bits != 8 && bits != 16 && bits != (4 | TI_BITS_G32) && bits != (8 | TI_BITS_G32) &&
        bits != (4 | TI_BITS_G32 | TI_BITS_AFF))
      throw std::runtime_error(
          "InferenceEngine: weight_bits must be 4, 8, 16, 4 / 8 | 32 (group-32 blocks) or 4 | 32 | 64 (Q4_1 blocks)");
    cfg.vocab = (int)V;
    cfg.hidden = (int)H;
    cfg.layers = (int)L;
    cfg.heads = (int)nh;
    cfg.head_dim = (int)hd;
    cfg.kv_heads = (int)nh;
    if (k0) {
      const size_t kvd = k0->shape().total_size() / H;
      if (kvd % hd || !kvd) throw std::runtime_error("InferenceEngine: k_proj width not a multiple of head_dim");
      cfg.kv_heads = (int)(kvd / hd);
    }
    cfg.inter = (int)I;
    cfg.rope_theta = md.rope_theta > 0.0f ? md.rope_theta : 10000.0f;
    cfg.eps = 1e-5f;
    cfg.bits = compat ? 16 : bits;
    kv_bits = kv_bits_option(md);
    lookahead = compat ? 0 : lookahead_option(md, kv_bits);
    share_prefix = compat ? 0 : share_prefix_option(md, kv_bits);
    pen = penalty_options(md, lookahead, compat);
    guide = guide_option(md, lookahead, compat);
    cfg.max_seq = (int)std::max<size_t>(1, c.max_sequence_length);
    cfg.compat = compat ? 1 : 0;
    cfg.device = gpu;
    create(c);

    for (size_t l = 0; l < L; ++l) {
      const int li = (int)l;
      const core::Tensor* up = layer_tensor(m, l, "mlp.up_proj.weight", "feed_forward.w1.weight");
      const core::Tensor* down = layer_tensor(m, l, "mlp.down_proj.weight", "feed_forward.w2.weight");
      if (!up || !down) throw std::runtime_error("InferenceEngine: layer " + std::to_string(l) + " lacks FFN weights");
      upload(TI_W_UP, li, *up, H, I, cfg.bits);
      upload(TI_W_DOWN, li, *down, I, H, cfg.bits);
      if (compat) continue;
      const size_t qd = nh * hd, kvd = (size_t)cfg.kv_heads * hd;
      const core::Tensor* q = layer_tensor(m, l, "self_attn.q_proj.weight", "attention.q_proj.weight");
      const core::Tensor* k = layer_tensor(m, l, "self_attn.k_proj.weight", "attention.k_proj.weight");
      const core::Tensor* v = layer_tensor(m, l, "self_attn.v_proj.weight", "attention.v_proj.weight");
      const core::Tensor* o = layer_tensor(m, l, "self_attn.o_proj.weight", "attention.o_proj.weight");
      const core::Tensor* g = layer_tensor(m, l, "mlp.gate_proj.weight", "feed_forward.w3.weight");
      const core::Tensor* an = layer_tensor(m, l, "input_layernorm.weight", "attention_norm.weight");
      const core::Tensor* fn = layer_tensor(m, l, "post_attention_layernorm.weight", "ffn_norm.weight");
      if (!q || !k || !v || !o || !g || !an || !fn)
        throw std::runtime_error("InferenceEngine: layer " + std::to_string(l) +
                                 " lacks attention / gate / norm weights (a llama model needs all of them)");
      upload(TI_W_Q, li, *q, H, qd, cfg.bits);
      upload(TI_W_K, li, *k, H, kvd, cfg.bits);
      upload(TI_W_V, li, *v, H, kvd, cfg.bits);
      upload(TI_W_O, li, *o, qd, H, cfg.bits);
      upload(TI_W_GATE, li, *g, H, I, cfg.bits);
      upload_vec(TI_V_ATTN_NORM, li, *an, H);
      upload_vec(TI_V_FFN_NORM, li, *fn, H);
    }
    upload(TI_W_LM_HEAD, 0, *lm, H, V, cfg.bits);
    if (!compat) {
      const core::Tensor* norm = find(m, {"norm.weight", "model.norm.weight"});
      const core::Tensor* emb = find(m, {"token_embeddings.weight", "embed_tokens.weight"});
      if (!norm || !emb) throw std::runtime_error("InferenceEngine: llama model needs norm.weight and the token embeddings");
      upload_vec(TI_V_OUT_NORM, 0, *norm, H);
      upload_vec(TI_E_EMBED, 0, *emb, V * H);
    }
  }

  // sample_next_token (inference_engine.cpp:1554-1673) with the engine's mt19937 draw
  int sample(const float* logits, const InferenceConfig& c, std::vector<float>* logprobs) {
    std::uniform_real_distribution<float> dist(0.0f, 1.0f);
    const float u = dist(rng);
    int tok = 0;
    float lp = 0.0f;
    check(ti_sample_token(logits, cfg.vocab, c.temperature, (int)std::min<size_t>(c.top_k, (size_t)cfg.vocab), c.top_p,
                          u, &tok, &lp),
          "ti_sample_token");
    if (logprobs) logprobs->push_back(lp);
    return tok;
  }
};

InferenceEngine::InferenceEngine(const ModelData& model_data, const InferenceConfig& config)
    : model_metadata_(model_data.metadata()), config_(config), impl_(std::make_unique<InferenceEngineImpl>()) {
  if (config_.device == core::ComputeDevice::kCPU)
    throw std::runtime_error("InferenceEngine: this build runs on MI355X (gfx950) only; kCPU is the reference's path");
  impl_->build(model_data, config_);
}

InferenceEngine::InferenceEngine(const std::string& model_path, const InferenceConfig& config)
    : InferenceEngine(ModelLoader::load(model_path), config) {}

InferenceEngine::~InferenceEngine() = default;
InferenceEngine::InferenceEngine(InferenceEngine&&) noexcept = default;
InferenceEngine& InferenceEngine::operator=(InferenceEngine&&) noexcept = default;

void InferenceEngine::set_config(const InferenceConfig& config) {
  if (config.max_sequence_length != config_.max_sequence_length)
    throw std::runtime_error("InferenceEngine::set_config: max_sequence_length is fixed when the device engine is built");
  config_ = config;
}

void InferenceEngine::validate_input_tokens(const std::vector<int>& tokens) const {
  if (tokens.empty()) throw std::runtime_error("Input tokens cannot be empty");
  if (tokens.size() > config_.max_sequence_length)
    throw std::runtime_error("Input sequence length exceeds maximum allowed length");
  for (int t : tokens)
    if (t < 0 || t >= impl_->cfg.vocab) throw std::runtime_error("Input token id " + std::to_string(t) + " out of vocabulary");
}

void InferenceEngine::validate_batch_size(size_t batch_size) const {
  if (batch_size == 0) throw std::runtime_error("Batch size cannot be zero");
  if (batch_size > config_.max_batch_size) throw std::runtime_error("Batch size exceeds maximum allowed batch size");
}

GenerationResult InferenceEngine::generate(const std::string&, size_t, bool) {
  off_path("generate(std::string)", "-- the tokenizer; pass token ids");
}

GenerationResult InferenceEngine::generate(const std::vector<int>& input_tokens, size_t max_new_tokens,
                                           bool include_logprobs) {
  return generate_batch(std::vector<std::vector<int>>{input_tokens}, max_new_tokens, include_logprobs).at(0);
}

std::vector<GenerationResult> InferenceEngine::generate_batch(const std::vector<std::string>&, size_t, bool) {
  off_path("generate_batch(std::vector<std::string>)", "-- the tokenizer; pass token ids");
}

std::vector<GenerationResult> InferenceEngine::generate_batch(const std::vector<std::vector<int>>& batches,
                                                              size_t max_new_tokens, bool include_logprobs) {
  validate_batch_size(batches.size());
  for (const auto& b : batches) validate_input_tokens(b);
  InferenceEngineImpl& im = *impl_;
  const size_t maxlen = config_.max_sequence_length;
  const int V = im.cfg.vocab;
  std::vector<GenerationResult> results(batches.size());
  // The contract of generate() (inference_engine.cpp:734-802): stop after EOS or once the
  // sequence reaches max_sequence_length; otherwise stop_reason "max_new_tokens".  EOS is token
  // id 2 whatever config.eos_token_id says (:759-760 hard-codes it; only beam search reads the
  // config, :2015).  total_time_ms is whole milliseconds (duration_cast<milliseconds>, :778-780)
  // and tokens_per_second = generated / (total_time_ms / 1000), inf (or NaN) under 1 ms (:782).
  auto finish = [&](GenerationResult& r, const std::vector<int>& prompt, const std::vector<int>& fresh,
                    const std::vector<float>& lps, float ms) {
    r.tokens = prompt;
    r.finished = false;
    for (size_t i = 0; i < fresh.size(); ++i) {
      r.tokens.push_back(fresh[i]);
      if (i < lps.size()) r.logprobs.push_back(lps[i]);
      if (fresh[i] == kGenerateEos) {
        r.finished = true;
        r.stop_reason = "eos_token";
        break;
      }
      if (r.tokens.size() >= maxlen) {
        r.finished = true;
        r.stop_reason = "max_length";
        break;
      }
    }
    if (!r.finished) r.stop_reason = "max_new_tokens";
    r.total_time_ms = static_cast<float>(static_cast<long long>(ms));
    const size_t gen = r.tokens.size() - prompt.size();
    r.tokens_per_second = gen / (r.total_time_ms / 1000.0f);
    im.total_generations++;
    im.total_tokens += gen;
    im.total_time_ms += r.total_time_ms;
    im.peak_tps = std::max(im.peak_tps, r.tokens_per_second);
  };
  // new tokens a request can take before max_length stops it (at least one is sampled)
  auto budget = [&](size_t plen) {
    return std::max<size_t>(1, std::min(max_new_tokens, maxlen > plen ? maxlen - plen : 1));
  };
  if (max_new_tokens == 0) {
    for (size_t i = 0; i < batches.size(); ++i) finish(results[i], batches[i], {}, {}, 0.0f);
    return results;
  }

  if (im.compat) {
    // reference_compat: placeholder-embedding plumbing model, one request at a time
    std::vector<float> logits(V);
    for (size_t i = 0; i < batches.size(); ++i) {
      const auto t0 = std::chrono::steady_clock::now();
      const auto& p = batches[i];
      std::vector<int> fresh;
      std::vector<float> lps;
      check(ti_engine_compat_step(im.eng, (int)((p.size() - 1) * im.cfg.hidden), logits.data()), "ti_engine_compat_step");
      im.total_forward_passes++;
      const size_t n = budget(p.size());
      for (size_t s = 0; s < n; ++s) {
        const int tok = im.sample(logits.data(), config_, include_logprobs ? &lps : nullptr);
        fresh.push_back(tok);
        if (tok == kGenerateEos || p.size() + fresh.size() >= maxlen || s + 1 == n) break;
        check(ti_engine_compat_step(im.eng, 0, logits.data()), "ti_engine_compat_step");
        im.total_forward_passes++;
      }
      const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
      finish(results[i], p, fresh, lps, ms);
    }
    return results;
  }

  // (active penalties, a guide: only the sampled device loop applies them, so a greedy config runs it with top_k = 1)
  const bool greedy = config_.top_k == 1 && !include_logprobs && !im.pen.active() && !im.guide.active();
  // The shared-prefix option: the leading tokens common to a device-loop group of two or more requests, when
  // there are at least `share_prefix` of them, are registered (prefilled once, for every stream slot, so the next
  // generate_batch with the same prefix finds them registered) and the group passes its continuations with
  // start_pos = P.  Every request keeps at least one own prompt token.  The positions are those of the full
  // prompts, so KV room, budgets and the stop handling do not change.  -> P, 0 when the group runs as ever.
  auto share_group = [&](size_t c0, int n) -> size_t {
    if (im.share_prefix <= 0 || n < 2) return 0;
    const auto& a = batches[c0];
    size_t common = a.size(), shortest = a.size();
    for (int m = 1; m < n; ++m) {
      const auto& b = batches[c0 + m];
      shortest = std::min(shortest, b.size());
      size_t k = 0;
      while (k < common && k < b.size() && b[k] == a[k]) ++k;
      common = k;
    }
    if (common < (size_t)im.share_prefix || shortest < 2) return 0;
    const size_t P = std::min(common, shortest - 1);
    const std::vector<int32_t> pre(a.begin(), a.begin() + (std::ptrdiff_t)P);
    check(ti_engine_share_prefix(im.eng, pre.data(), (int)P, im.capacity), "ti_engine_share_prefix");
    return P;
  };
  // Requests go to the device together, `capacity` at a time.  A greedy group advances in
  // lock step from position 0, so the longest prompt bounds everyone's KV room: when that
  // would cut a request short of its budget, the group is run one request at a time.
  size_t group = (size_t)im.capacity;
  if (greedy) {
    size_t longest = 0;
    for (const auto& b : batches) longest = std::max(longest, b.size());
    for (const auto& b : batches)
      if (budget(b.size()) > (size_t)im.cfg.max_seq + 1 - longest) group = 1;
  }
  for (size_t c0 = 0; c0 < batches.size(); c0 += group) {
    const int n = (int)std::min<size_t>(group, batches.size() - c0);
    const auto t0 = std::chrono::steady_clock::now();
    size_t stride = 1, want = 1;
    for (int m = 0; m < n; ++m) {
      stride = std::max(stride, batches[c0 + m].size());
      want = std::max(want, budget(batches[c0 + m].size()));
    }
    std::vector<std::vector<int>> fresh(n);
    std::vector<std::vector<float>> lps(n);
    // forward passes = the engine's decode steps + prompt chunks actually run (the device loop
    // stops at EOS in chunks, so this is not the planned step count)
    uint64_t d0 = 0, p0 = 0, d1 = 0, p1 = 0;
    check(ti_engine_counters(im.eng, &d0, &p0), "ti_engine_counters");
    // the device sampler's range of top_k (sampled, or greedy with include_logprobs)
    const bool sampled_k = !greedy && config_.top_k >= 1 && config_.top_k <= (size_t)V;
    // a group of such requests runs ti_engine_generate_sampled with n streams: in lock step from position 0, so
    // it must leave every request its budget (steps = longest prompt + new - 1 <= max_seq); otherwise, and under
    // TI_BATCH_SAMPLE_DEVICE=0 (A/B knob), the host-sampler loop below
    const bool sampled_group = sampled_k && n > 1 && batch_sample_device() && want <= (size_t)im.cfg.max_seq + 1 - stride &&
                               stride <= (size_t)im.cfg.max_seq;
    const bool device_loop = greedy || (sampled_k && (n == 1 || sampled_group));
    if (greedy) {
      // the whole token loop on the device (argmax feedback); it stops once every request of the
      // group emitted EOS (ti_engine_set_stop), the length limit is applied after
      std::vector<int32_t> prompts((size_t)n * stride, 0), lens(n), out((size_t)n * want);
      for (int m = 0; m < n; ++m) {
        const auto& p = batches[c0 + m];
        std::copy(p.begin(), p.end(), prompts.begin() + (size_t)m * stride);
        lens[m] = (int32_t)p.size();
      }
      // the longest prompt sets the step count (steps = longest + new - 1 <= max_seq)
      const size_t steps_new = std::min(want, (size_t)im.cfg.max_seq + 1 - stride);
      // a request that runs alone, with the lookahead option: the same tokens, several per step where the text
      // repeats itself (no corpus, 3-grams); it needs k KV rows of head-room, without them the plain loop runs
      if (im.lookahead > 0 && n == 1 && steps_new >= 1 &&
          stride + steps_new - 1 + (size_t)im.lookahead <= (size_t)im.cfg.max_seq) {
        check(ti_engine_generate_lookahead(im.eng, 0, prompts.data(), lens[0], 0, nullptr, 0, im.lookahead, 3,
                                           (int)steps_new, out.data(), nullptr),
              "ti_engine_generate_lookahead");
      } else if (const size_t P = share_group(c0, n)) {   // the continuations behind the registered prefix
        const std::vector<int32_t> start(n, (int32_t)P);
        for (int m = 0; m < n; ++m) lens[m] -= (int32_t)P;
        check(ti_engine_generate(im.eng, n, prompts.data() + P, lens.data(), (int)stride, start.data(), (int)steps_new,
                                 out.data(), nullptr),
              "ti_engine_generate");
      } else {
        check(ti_engine_generate(im.eng, n, prompts.data(), lens.data(), (int)stride, nullptr, (int)steps_new,
                                 out.data(), nullptr),
              "ti_engine_generate");
      }
      for (int m = 0; m < n; ++m) {
        const size_t b = budget(batches[c0 + m].size());
        for (size_t t = 0; t < std::min(b, steps_new); ++t) fresh[m].push_back(out[(size_t)m * steps_new + t]);
      }
    } else if (sampled_k && n == 1) {
      // one request with top-k sampling (any k up to the vocabulary): the whole loop on the device
      // (ti_engine_generate_sampled), fed the engine's mt19937 draws in the reference's order;
      // the generator then advances by the draws the request actually used (one per token).
      // With the lookahead option and its k KV rows of head-room: the same tokens for the same draws, several
      // per step where the text repeats itself (ti_engine_generate_lookahead_sampled; no corpus, 3-grams).
      const auto& p = batches[c0];
      const size_t steps_new = std::min(want, (size_t)im.cfg.max_seq + 1 - p.size());
      std::mt19937 saved = im.rng;
      std::uniform_real_distribution<float> dist(0.0f, 1.0f);
      std::vector<float> draws(steps_new), lp(steps_new);
      for (float& d : draws) d = dist(im.rng);
      std::vector<int32_t> prompt(p.begin(), p.end()), out(steps_new);
      const int32_t len = (int32_t)p.size();
      if (im.lookahead > 0 && steps_new >= 1 &&
          p.size() + steps_new - 1 + (size_t)im.lookahead <= (size_t)im.cfg.max_seq) {
        check(ti_engine_generate_lookahead_sampled(im.eng, 0, prompt.data(), len, 0, nullptr, 0, im.lookahead, 3,
                                                   (int)steps_new, config_.temperature, (int)config_.top_k,
                                                   config_.top_p, draws.data(), out.data(), lp.data(), nullptr),
              "ti_engine_generate_lookahead_sampled");
      } else {
        check(ti_engine_generate_sampled(im.eng, 1, prompt.data(), &len, (int)p.size(), nullptr, (int)steps_new,
                                         config_.temperature, (int)config_.top_k, config_.top_p, draws.data(),
                                         out.data(), lp.data()),
              "ti_engine_generate_sampled");
      }
      const size_t b = budget(p.size());
      for (size_t t = 0; t < std::min(b, steps_new); ++t) {
        fresh[0].push_back(out[t]);
        if (include_logprobs) lps[0].push_back(lp[t]);
        if (out[t] == kGenerateEos || p.size() + fresh[0].size() >= maxlen) break;
      }
      im.rng = saved;
      im.rng.discard(fresh[0].size());
    } else if (sampled_group) {
      // several such requests: the same device loop with n streams.  Draws come from the engine's mt19937,
      // steps_new per request, request-major, and the generator stays advanced by all of them.  There is no
      // draw order to preserve for a parallel group: the reference seeds its generator from the clock and runs
      // a batch one request after the other (inference_engine.cpp:804-828), and the host loop below already
      // consumes draws step-major across the group.  Tokens are cut at EOS and at the budget here.
      const size_t steps_new = want;
      std::uniform_real_distribution<float> dist(0.0f, 1.0f);
      std::vector<float> draws((size_t)n * steps_new), lp((size_t)n * steps_new);
      for (float& d : draws) d = dist(im.rng);
      std::vector<int32_t> prompts((size_t)n * stride, 0), lens(n), out((size_t)n * steps_new);
      for (int m = 0; m < n; ++m) {
        const auto& p = batches[c0 + m];
        std::copy(p.begin(), p.end(), prompts.begin() + (size_t)m * stride);
        lens[m] = (int32_t)p.size();
      }
      const size_t P = share_group(c0, n);   // > 0: the continuations behind the registered prefix
      const std::vector<int32_t> start(n, (int32_t)P);
      for (int m = 0; m < n; ++m) lens[m] -= (int32_t)P;
      check(ti_engine_generate_sampled(im.eng, n, prompts.data() + P, lens.data(), (int)stride, P ? start.data() : nullptr,
                                       (int)steps_new, config_.temperature, (int)config_.top_k, config_.top_p, draws.data(),
                                       out.data(), lp.data()),
            "ti_engine_generate_sampled");
      for (int m = 0; m < n; ++m) {
        const auto& p = batches[c0 + m];
        const size_t b = budget(p.size());
        for (size_t t = 0; t < std::min(b, steps_new); ++t) {
          const int32_t tok = out[(size_t)m * steps_new + t];
          if (tok < 0) break;   // (past the stop token)
          fresh[m].push_back(tok);
          if (include_logprobs) lps[m].push_back(lp[(size_t)m * steps_new + t]);
          if (tok == kGenerateEos || p.size() + fresh[m].size() >= maxlen) break;
        }
      }
    } else {
      // logits to the host every step: the reference sampler (temperature / top-k / top-p / draw)
      std::vector<float> logits((size_t)n * V);
      std::vector<int32_t> tok(n), pos(n, 0);
      std::vector<size_t> fed(n, 0);   // prompt tokens consumed
      std::vector<bool> done(n, false);
      std::vector<int32_t> ctx;   // (active penalties: the request's prompt and new tokens so far)
      std::vector<int> gstate(n, im.guide.start);   // (a guide: each request's automaton state)
      const ti_guide gview = im.guide.view();
      const size_t steps = stride + want - 1;
      for (size_t s = 0; s < steps; ++s) {
        for (int m = 0; m < n; ++m) {
          const auto& p = batches[c0 + m];
          tok[m] = fed[m] < p.size() ? p[fed[m]] : (fresh[m].empty() ? 0 : fresh[m].back());
          pos[m] = (int32_t)std::min<size_t>(s, (size_t)im.cfg.max_seq - 1);
        }
        check(ti_engine_step(im.eng, n, tok.data(), pos.data(), logits.data()), "ti_engine_step");
        im.total_forward_passes++;
        bool all_done = true;
        for (int m = 0; m < n; ++m) {
          const auto& p = batches[c0 + m];
          if (fed[m] < p.size()) ++fed[m];
          if (fed[m] < p.size() || done[m]) {
            all_done = all_done && done[m];
            continue;
          }
          if (im.pen.active()) {   // the device loops' penalties, bit for bit, before the host sampler
            ctx.assign(p.begin(), p.end());
            ctx.insert(ctx.end(), fresh[m].begin(), fresh[m].end());
            check(ti_penalize_logits(&logits[(size_t)m * V], V, ctx.data(), (int)ctx.size(), im.pen.repetition,
                                     im.pen.presence, im.pen.frequency),
                  "ti_penalize_logits");
          }
          if (im.guide.active())   // the device loops' guide step, bit for bit: consume the token just fed, then mask
            check(ti_guide_apply(&gview, V, gstate[m], fresh[m].empty() ? -1 : fresh[m].back(), &logits[(size_t)m * V],
                                 &gstate[m]),
                  "ti_guide_apply");
          const int t = im.sample(&logits[(size_t)m * V], config_, include_logprobs ? &lps[m] : nullptr);
          fresh[m].push_back(t);
          if (t == kGenerateEos || fresh[m].size() >= budget(p.size())) done[m] = true;
          all_done = all_done && done[m];
        }
        if (all_done) break;
      }
    }
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (device_loop) {   // (the host-sampler loop counts its own steps)
      check(ti_engine_counters(im.eng, &d1, &p1), "ti_engine_counters");
      im.total_forward_passes += (size_t)((d1 - d0) + (p1 - p0));
    }
    for (int m = 0; m < n; ++m) finish(results[c0 + m], batches[c0 + m], fresh[m], lps[m], ms);
  }
  return results;
}

// generate_beam_search (inference_engine.cpp:830-871): the beam loop runs in ti_engine_beam_search
// (beams as KV stream slots, one batched device step per round, the reference's host ranking);
// results keep only the new tokens and, with include_logprobs, the beam's average log-probability
// per token.  max_new_tokens = 0 gives the prompt back as one finished result with no tokens.
std::vector<GenerationResult> InferenceEngine::generate_beam_search(const std::vector<int>& input_tokens,
                                                                   size_t max_new_tokens, size_t beam_size,
                                                                   bool include_logprobs) {
  if (beam_size == 0) throw std::runtime_error("Beam size must be greater than 0");
  validate_input_tokens(input_tokens);
  InferenceEngineImpl& im = *impl_;
  if (im.compat) off_path("generate_beam_search on the reference_compat plumbing model", "rank 4");
  if (im.pen.active())
    throw std::runtime_error("InferenceEngine::generate_beam_search: beam search does not apply the repetition / presence / "
                             "frequency penalties this engine was built with");
  if (im.guide.active())
    throw std::runtime_error("InferenceEngine::generate_beam_search: beam search does not follow the guide (guide_file) this "
                             "engine was built with");
  std::vector<GenerationResult> results;
  const int nb = (int)beam_size, mn = (int)max_new_tokens;
  std::vector<int32_t> prompt(input_tokens.begin(), input_tokens.end()), out((size_t)nb * mn);
  std::vector<float> lp(nb);
  std::vector<int32_t> fin(nb);
  int count = 0;
  const auto t0 = std::chrono::steady_clock::now();
  check(ti_engine_beam_search(im.eng, prompt.data(), (int)prompt.size(), mn, nb, config_.temperature,
                              (int)std::min<size_t>(config_.top_k, (size_t)im.cfg.vocab), config_.top_p,
                              config_.length_penalty, config_.eos_token_id, out.data(), lp.data(), nullptr, fin.data(),
                              &count),
        "ti_engine_beam_search");
  const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (int r = 0; r < count; ++r) {
    GenerationResult g;
    for (int t = 0; t < mn && out[(size_t)r * mn + t] >= 0; ++t) g.tokens.push_back(out[(size_t)r * mn + t]);
    g.finished = fin[r] != 0;
    if (include_logprobs && !g.tokens.empty()) g.logprobs.assign(g.tokens.size(), lp[r] / (float)g.tokens.size());
    g.total_time_ms = ms;
    results.push_back(std::move(g));
  }
  return results;
}
// compute_logprobs (inference_engine.cpp:873-954): element i is log p(tokens[i]) under the logits of
// position i (the reference's indexing, :934-942), scored on the device by ti_engine_score in stream
// slot 0 from position 0.  Unlike the reference, a device error throws (check) instead of coming
// back as a vector of -18.0f (LOGPROB_COMPUTATION_ERROR, :948-953): a sentinel would hide a GPU failure.
std::vector<float> InferenceEngine::compute_logprobs(const std::vector<int>& tokens) {
  validate_input_tokens(tokens);
  InferenceEngineImpl& im = *impl_;
  if (im.compat) off_path("compute_logprobs on the reference_compat plumbing model", "rank 1");
  const std::vector<int32_t> t(tokens.begin(), tokens.end());
  std::vector<float> lp(t.size());
  check(ti_engine_score(im.eng, 0, t.data(), (int)t.size(), 0, nullptr, lp.data(), nullptr), "ti_engine_score");
  return lp;
}
std::vector<int> InferenceEngine::encode(const std::string&) { off_path("encode", "-- the tokenizer"); }
std::string InferenceEngine::decode(const std::vector<int>&) { off_path("decode", "-- the tokenizer"); }

void InferenceEngine::reset_state() {
  if (!impl_) return;
  impl_->total_generations = impl_->total_tokens = impl_->total_forward_passes = 0;
  impl_->total_time_ms = impl_->peak_tps = 0.0f;
  impl_->rng.seed((unsigned)std::chrono::steady_clock::now().time_since_epoch().count());
  // the KV cache needs no clearing: every request starts writing at position 0
}

size_t InferenceEngine::memory_usage() const {
  if (!impl_ || !impl_->eng) return 0;
  size_t w = 0, kv = 0;
  check(ti_engine_memory(impl_->eng, &w, &kv), "ti_engine_memory");
  return w + kv;
}

std::string InferenceEngine::performance_stats() const {
  if (!impl_) return "Performance statistics unavailable (engine not initialized)";
  const InferenceEngineImpl& im = *impl_;
  std::ostringstream os;
  os << std::fixed << std::setprecision(2);
  os << "=== TurboInfer Performance Statistics (MI355X) ===\n";
  os << "  Total Generations: " << im.total_generations << "\n";
  os << "  Total Tokens Generated: " << im.total_tokens << "\n";
  os << "  Total Generation Time: " << im.total_time_ms << " ms\n";
  os << "  Forward Passes: " << im.total_forward_passes << "\n";
  if (im.total_time_ms > 0.0f)
    os << "  Average Tokens/Second: " << (im.total_tokens / (im.total_time_ms / 1000.0f)) << "\n";
  os << "  Peak Tokens/Second: " << im.peak_tps << "\n";
  os << "  Device Memory: " << (memory_usage() / (1024.0 * 1024.0)) << " MB (weights " << (im.cfg.bits & ~(TI_BITS_G32 | TI_BITS_AFF))
     << "-bit" << ((im.cfg.bits & TI_BITS_AFF) ? " affine group-32 blocks" : (im.cfg.bits & TI_BITS_G32) ? " group-32 blocks" : "") << (im.kv_bits == 8 ? ", fp8 KV, " : ", fp16 KV, ") << im.capacity
     << " stream(s) x " << im.cfg.max_seq << " slots)\n";
  os << "  Mode: " << (im.compat ? "reference_compat (plumbing model)" : "llama decode") << "\n";
  return os.str();
}

std::unique_ptr<InferenceEngine> create_engine(const std::string& model_path, const InferenceConfig& config) {
  return std::make_unique<InferenceEngine>(model_path, config);
}

// Reference inference_engine.cpp:2075-2082: build an engine from the checkpoint, then
// generate(prompt) and decode().  The checkpoint loads (GGUF); the string prompt
// needs the tokenizer, which is out of scope, so this throws from generate(std::string) rather
// than returning text it cannot produce.
std::string quick_generate(const std::string& model_path, const std::string& prompt, size_t max_tokens,
                           float temperature) {
  InferenceConfig config;
  config.temperature = temperature;
  InferenceEngine engine(model_path, config);
  auto result = engine.generate(prompt, max_tokens);
  return engine.decode(result.tokens);
}

}  // namespace model
}  // namespace turboinfer
