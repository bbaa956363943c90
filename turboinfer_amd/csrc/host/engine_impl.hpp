// engine_impl.hpp -- what the engine's translation units (engine*.cpp) share: the ti_engine struct, the error
// macros, and the declarations of the internals (namespace ti_eng), each defined in the file named beside it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <compare>
#include <queue>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <utility>
#include <vector>

#include "ti_engine.h"
#include "ti_hip.h"

int ti_set_error(int code, const char* fmt, ...);
int ti_check_hip(hipError_t e, const char* what);

#define E_CHECK(expr, what)                                \
  do {                                                     \
    hipError_t _e = (expr);                                \
    if (_e != hipSuccess) return ti_check_hip(_e, what);   \
  } while (0)
#define TI_TRY(expr)                 \
  do {                               \
    const int _rc = (expr);          \
    if (_rc != TI_OK) return _rc;    \
  } while (0)

namespace ti_eng {

struct DevLinear {
  void* tiles = nullptr;
  uint16_t* scales = nullptr;
  float* f32 = nullptr;     // compat: reference-layout fp32 [K][N]
  int K = 0, N = 0;
};

struct DevLayer {
  DevLinear qkv, o, gu, down;
  float* attn_norm = nullptr;
  float* ffn_norm = nullptr;
  uint16_t* kc = nullptr;   // fp16 elements; e4m3 bytes on a TI_BITS_KV8 engine (ti_engine::kv_at)
  uint16_t* vc = nullptr;
};

// What one decode step's launch sequence depends on besides its row count: chosen by the entry point and passed
// down to run_steps / get_graph / enqueue_step, which build the cache key from the same object.
struct StepMode {
  bool advance = false;   // the lm_head advances step_ctr (the device loop); off: a replay step
  bool sampled = false;   // ti_penalty_step / ti_guide_step (when active) + ti_sample_step behind the lm_head
  bool shared = false;    // the registered prefix attended once for all streams (ti_attn_decode_shared)
  bool carry = false;     // the penalty / guide step takes each slot's pen_carry token first (the serve loop's chunks)
  // ti_engine_serve_requests: the launches behind the lm_head read each row's values from e->row_params
  bool rows = false;      // ti_penalty_step_rows (with rows_pen) / ti_sample_step_rows instead of the scalar forms
  bool rows_pen = false;  // rows: some request of the call penalises, the penalty launch is in the graph
  bool rows_big = false;  // rows: some request's top_k is above TI_SAMPLE_MAX_K, every row on the workspace instance
  bool rows_guide = false;  // rows: some request names a library guide, ti_guide_step_rows is in the graph
};

// Everything a captured graph bakes in that can differ between two live graphs.  Whatever else enqueue_step or
// enqueue_verify read (buffers, sampler parameters, penalty values, share_len, fold / qkv_attn settings) is
// dropped with the whole cache when it changes (drop_graphs).
struct GraphKey {
  enum Kind : int { Step, Verify } kind;
  int rows;     // M, or k + 1
  int slot;     // Verify: the stream slot; Step: 0
  int splits;   // Verify: la_splits; Step: 0
  bool advance, sampled, shared, carry;
  bool row_table, rows_pen, rows_big;   // StepMode's rows / rows_pen / rows_big, false in a Verify key
  bool rows_guide;                      // StepMode's rows_guide, false in a Verify key
  auto operator<=>(const GraphKey&) const = default;
};

}  // namespace ti_eng

struct ti_engine {
  ti_engine_config c{};
  hipStream_t s = nullptr;
  std::vector<void*> allocs;
  using DevLinear = ti_eng::DevLinear;
  using DevLayer = ti_eng::DevLayer;
  std::vector<DevLayer> layer;
  DevLinear lm;
  uint16_t* emb = nullptr;
  float* out_norm = nullptr;
  float* rope_cs = nullptr;
  // step buffers
  float* h = nullptr;
  float* h_last = nullptr;   // [max_batch][hidden]: each stream's last prompt row (ti_engine_generate)
  float* q = nullptr;
  float* tmp = nullptr;        // compat FFN activations (fp32)
  float* logits = nullptr;
  float* ws = nullptr;
  uint16_t* attn = nullptr;
  uint16_t* act = nullptr;
  uint16_t* xn = nullptr;      // fp16 rms_norm rows for the batched-rows GEMM [R][hidden]
  // single-stream steps with the rms_norm folded behind the GEMM (ti_hip.h TI_X_F16_FOLDED):
  // the epilogue that writes h also writes fx = fp16(h * next norm weight) and its workgroups'
  // sums of h^2 (ss); the next projection stages fx and divides its outputs by the rms
  bool fold_on = true;         // TI_FOLD=0 / ti_engine_set_fold
  uint16_t* fx = nullptr;      // [hidden]
  float* ss = nullptr;         // [256]
  // batched fold (17..64 int4 rows): the producers' (O, down) epilogues write xn = fp16(h * next
  // norm weight) and per-column-group sums of h^2 per row [n_cg][TI_FOLD_SS_ROWS]
  float* ss_rows = nullptr;
  // single-stream attention leaves its split merge to the O projection (ti_attn_decode_partials
  // + TI_X_ATTN_SPLITS): no arrival-ticket hand-off at the end of the attention launch
  bool part_on = true;         // TI_ATTN_PART=0 turns it off
  uint16_t* part_o = nullptr;  // [heads][TI_ATTN_MAX_PART_SPLITS][head_dim]
  float* part_ml = nullptr;    // [heads][TI_ATTN_MAX_PART_SPLITS][2]
  // one stream (head_dim 64 GQA or head_dim 128 MHA): QKV and the attention in one launch (ti_qkv_attn_partials,
  // DESIGN 4.19), O merging its splits (TI_X_ATTN_SPLITS); TI_QKV_ATTN=0 turns it off
  bool qa_on = true;
  void* qa_xchg = nullptr;     // the q exchange of ti_qkv_attn_partials (zeroed once, generations kept)
  // on-device sampling (ti_engine_generate_sampled): the step graph of StepMode::sampled ends with ti_sample_step
  float samp_t = 1.0f, samp_p = 1.0f;
  int samp_k = 1;
  float* draws = nullptr;      // [max_batch][draw_cap] uniform draws, per new token
  float* lps = nullptr;        // [max_batch][draw_cap] log p of the sampled tokens
  int draw_cap = 0;
  void* splitk_ws = nullptr;   // tile GEMM split-K workspace (ti_epilogue.splitk_ws), int4 engines
  size_t splitk_bytes = 0;
  void* samp_ws = nullptr;     // ti_sample_step_ws workspace (top_k > TI_SAMPLE_MAX_K)
  size_t samp_ws_bytes = 0;
  // prefill (forward_pass over prompt tokens): up to pf_rows prompt tokens of one stream run
  // as rows of the batched path, sharing that stream's KV cache (stride 0)
  int pf_rows = 0;             // 0 = off (prompts consumed one token per decode step)
  int rows_cap = 0;            // R = max(max_batch, pf_rows): rows the step buffers hold
  int32_t* pf_ones = nullptr;  // [pf_rows] 1
  int32_t* pf_zero = nullptr;  // [1] 0
  int32_t* pf_base = nullptr;  // [pf_rows] positions of the chunk's rows
  // ti_engine_score (allocated by its first call; no step graph reads or writes them)
  float* sc_logits = nullptr;    // [TI_SCORE_ROWS][vocab] logits of one block of chunk rows
  int32_t* sc_targets = nullptr; // [max_seq]
  float* sc_lp = nullptr;        // [max_seq]
  int32_t* sc_top1 = nullptr;    // [max_seq]
  // ti_engine_generate_lookahead (allocated by its first call, outside ti_engine_memory; the verify graphs,
  // GraphKey::Verify in `graphs`, bake these pointers: growing hist / out drops them)
  float* la_logits = nullptr;    // [TI_LA_MAX_K + 1][vocab] logits of the verify rows
  int32_t* la_state = nullptr;   // [TI_LA_STATE_WORDS] then cfg [4] (ti_lookahead_args)
  int32_t* la_row_tok = nullptr; // [TI_LA_MAX_K + 1]
  int32_t* la_hist = nullptr;    // [la_hist_cap] corpus ++ prompt ++ generated
  int32_t* la_out = nullptr;     // [la_out_cap]
  int la_hist_cap = 0, la_out_cap = 0;
  float* la_ws = nullptr;        // ti_attn_prefill_split workspace (16 rows, 32 splits)
  // ti_engine_generate_lookahead_sampled: its verify graphs (GraphKey::sampled) also bake the
  // sampler's parameters (samp_t / samp_k / samp_p, samp_ws) and these two; a change of either drops the graphs
  float* la_draws = nullptr;     // [la_samp_cap] the request's uniform draws, per new token
  float* la_lps = nullptr;       // [la_samp_cap] log p of the sampled tokens
  int la_samp_cap = 0;
  // ti_engine_share_prefix: rows [0, share_len) of slots [0, share_n) are identical (slot 0's prefill, copied)
  // and nobody writes them while registered.  ti_engine_generate / _step / the serve loop pass StepMode::shared
  // to their batched steps when these may attend the prefix once for all streams (ti_attn_decode_shared);
  // the step-graph key carries it, and a change of registration drops the graphs (share_len is baked in).
  std::vector<int32_t> share_tokens;
  int share_len = 0, share_n = 0;
  int share_min = 0;             // TI_SHARE_MIN: the shortest prefix that takes the shared attention
  float* share_ws = nullptr;     // ti_attn_decode_shared workspace (max_batch streams, 32 splits)
  // ti_engine_set_penalties: active iff the values differ from (1, 0, 0).  The sampled step graphs then run
  // ti_penalty_step between the lm_head and the sampler; the values, the state and the carry row are baked in
  // (a change of values drops the graphs; StepMode::carry, the serve loop's, is a graph key field).  Allocated by the
  // first activation, outside ti_engine_memory.
  float pen_rep = 1.0f, pen_pres = 0.0f, pen_freq = 0.0f;
  bool pen_active() const { return pen_rep != 1.0f || pen_pres != 0.0f || pen_freq != 0.0f; }
  ti_penalty_state pen{};        // counts / seen [max_batch][vocab], n_seen [max_batch]
  int32_t* pen_ctx = nullptr;    // [max_seq] one stream's context on its way to ti_penalty_reset
  int32_t* pen_carry = nullptr;  // [max_batch] each slot's input token of a serve chunk when it is a generated one
  // ti_engine_set_guide (engine_guide.cpp): active iff guide.mask is set.  The sampled step graphs then run
  // ti_guide_step behind ti_penalty_step; the device guide, the state row and the carry row (pen_carry, shared
  // with the penalties) are baked in, and setting or clearing a guide drops the graphs.  Outside ti_engine_memory.
  ti_guide_dev guide{};          // CSR + per-state allow-bitmask on the device (guide_bufs)
  int guide_start = 0;
  int32_t* guide_state = nullptr;  // [max_batch] each slot's automaton state, -1 = free or dead
  std::vector<void*> guide_bufs;   // the live guide's device buffers, freed when it is replaced
  bool guide_active() const { return guide.mask != nullptr; }
  // ti_engine_add_guide (engine_guide.cpp): the guide library of ti_engine_serve_requests_guided.  Handle h is entry
  // h - 1 of a device table [TI_GUIDE_CAP] of descriptors, all-zero where unused; the rows_guide step graphs bake in
  // the table's pointer only (ti_guide_step_rows), so adding and removing guides drops no graph.  Allocated by the
  // first add, outside ti_engine_memory; nothing but a request that names a handle reads it.
  struct LibGuide {
    bool live = false;
    int start = 0;
    std::vector<void*> bufs;   // the entry's CSR and bitmask on the device
  };
  ti_guide_dev* guide_table = nullptr;   // device [TI_GUIDE_CAP]
  std::vector<LibGuide> guide_lib;       // host [TI_GUIDE_CAP] once the table exists
  // ti_engine_serve_requests: each slot's sampler and penalty values, read by the rows-mode step graphs
  // (StepMode::rows), which bake in this pointer only.  Allocated by the first call, outside ti_engine_memory.
  ti_row_params* row_params = nullptr;   // [max_batch]
  unsigned long long* argmax = nullptr;
  int32_t* pos = nullptr;
  int32_t* base_pos = nullptr;
  int32_t* step_ctr = nullptr;
  int32_t* n_in = nullptr;
  int32_t* in_tokens = nullptr;
  int32_t* out_tokens = nullptr;
  int in_cap = 0, out_cap = 0;
  // generate() stop token (ti_engine_set_stop): the device loop runs in chunks and ends once every
  // stream has emitted it (the reference's `break` at EOS, inference_engine.cpp:760-764); -1 = none
  int32_t stop_token = -1;
  uint64_t n_decode_steps = 0;   // step-graph replays (ti_engine_counters)
  uint64_t n_prefill_chunks = 0; // prompt chunks through enqueue_prefill
  uint64_t n_graphs_captured = 0, n_graphs_dropped = 0;   // the graph cache's misses and drops (ti_engine_graph_counters)
  int splits_max = 1;
  int64_t kv_stride = 0;         // elements between the stream slots of a layer cache
  // TI_BITS_KV8 (taken out of c.bits at creation, which then holds the weight format alone): the
  // caches hold e4m3 bytes -- every QKV launch sets ti_epilogue.kv_fp8, the attention runs the _f8
  // entry points (prompt chunks too, at stride 0), the fused QKV + attention launch is off
  bool kv8 = false;
  size_t kv_esz() const { return kv8 ? 1 : 2; }   // bytes per cache element
  uint16_t* kv_at(uint16_t* base, size_t elems) const {
    return reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(base) + elems * kv_esz());
  }
  uint16_t** kv_tab = nullptr;   // device [2 * layers]: every layer's K then V cache base (ti_kv_copy_slots)
  size_t weight_bytes = 0, kv_bytes = 0;
  std::map<ti_eng::GraphKey, hipGraphExec_t> graphs;   // step and verify graphs (get_graph, get_verify_graph)
  int replay_M = 0;

  int qd() const { return c.heads * c.head_dim; }
  int kvd() const { return c.kv_heads * c.head_dim; }

  int alloc(void** p, size_t bytes) {
    TI_TRY(ti_malloc(p, bytes));
    allocs.push_back(*p);
    E_CHECK(hipMemsetAsync(*p, 0, bytes, s), "hipMemsetAsync(alloc)");
    return TI_OK;
  }
  template <class T>
  int alloc_t(T** p, size_t count) {
    void* v = nullptr;
    TI_TRY(alloc(&v, count * sizeof(T)));
    *p = static_cast<T*>(v);
    return TI_OK;
  }
  int alloc_linear(DevLinear& L, int K, int N) {
    L.K = K;
    L.N = N;
    if (c.compat) {
      TI_TRY(alloc_t(&L.f32, (size_t)K * N));
      weight_bytes += (size_t)K * N * 4;
      return TI_OK;
    }
    const size_t tb = ti_wpack_tile_bytes(c.bits, K, N), sb = ti_wpack_scale_bytes(c.bits, K, N);
    TI_TRY(alloc(&L.tiles, tb));
    if (sb) {
      void* p = nullptr;
      TI_TRY(alloc(&p, sb));
      L.scales = static_cast<uint16_t*>(p);
    }
    weight_bytes += tb + sb;
    return TI_OK;
  }
  // attention workgroups aimed at: one 8-wave workgroup per CU (128 / 256 / 512 measured 717 / 751 /
  // 681 tok/s); GQA partials with 8 splits
  static constexpr int attn_target = 256;
  static constexpr int gqa_part_splits = 8;
  int splits_for(int M) const {
    if (c.attn_splits > 0) return c.attn_splits;
    // one stream of a GQA model (>= 4 q-heads per kv-head) with a small cache per kv-head
    // (<= 1 MiB of K + V: TinyLlama at 2048): few long splits whose partials the O projection
    // merges (part_usable), instead of 64+ short splits merged by a last arriver
    // (attention run head by head: ti_attn_decode_partials' GQA expansion, heads x splits workgroups)
    if (M == 1 && gqa_part_splits >= 2 && part_on && c.heads >= 4 * c.kv_heads &&
        (size_t)c.max_seq * c.head_dim * 4 <= ((size_t)1 << 20))
      return std::min(gqa_part_splits, std::max(2, std::min(c.max_seq / 64, (attn_target + c.heads - 1) / c.heads)));
    // one 8-wave attention workgroup per CU: a second round of workgroups costs a whole
    // workgroup latency (load, merge hand-off) for little bandwidth (tools/probe_attn.hip)
    const int target = attn_target;
    int sp = (target + c.kv_heads * M - 1) / (c.kv_heads * M);
    const int cap = std::max(1, c.max_seq / 64);
    return std::max(1, std::min(sp, std::min(cap, 64)));
  }

  ~ti_engine() {
    for (auto& g : graphs) hipGraphExecDestroy(g.second);
    for (void* p : allocs) hipFree(p);
    for (void* p : guide_bufs) hipFree(p);
    for (auto& g : guide_lib)
      for (void* p : g.bufs) hipFree(p);
    if (s) hipStreamDestroy(s);
  }
};

namespace ti_eng {

// Every ti_engine_* entry binds the engine's device for its duration and restores the caller's
// current device on return (lazy allocations, graph (re)instantiation and launches all run on
// e->c.device whatever device the calling thread has current): several engines on several
// devices can be driven from one process, from any host thread (the reference
// binds its device in TensorEngine::initialize, tensor_engine.cpp:425-487).
struct DeviceScope {
  int prev = -1;
  bool changed = false;
  explicit DeviceScope(int device) {
    if (device >= 0 && hipGetDevice(&prev) == hipSuccess && prev != device) changed = hipSetDevice(device) == hipSuccess;
  }
  explicit DeviceScope(const ti_engine* e) : DeviceScope(e ? e->c.device : -1) {}
  ~DeviceScope() {
    if (changed) hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

// In-step launch stamps (ti_engine_stamp_steps): while a stamped step graph is being captured on this
// thread, every decode launcher asks ti_stamp_next for its workgroups' slot (kernels/common.hpp
// stamp_end: kStampWords = 24 words per workgroup) and the launch's kind / tag / grid are recorded.
constexpr int kStampWords = 24;   // = ti::kStampWords (kernels/common.hpp)
struct StampCtx {
  bool on = false;
  unsigned long long* base = nullptr;   // NULL: the sizing pass (record only)
  int tag = TI_STAMP_TAG_OTHER;
  std::vector<int32_t> info;            // [launch][3] kind, tag, workgroups (0 = unstamped)
  std::vector<size_t> offs;             // word offset of each launch's slot (second pass)
};
extern thread_local StampCtx g_stamp;   // engine_diag.cpp
inline void stamp_tag(int t) { g_stamp.tag = t; }

// The token of a greedy argmax / sampler key (low word: 0xFFFFFFFF - token, so the larger key is the lower token).
inline int32_t key_token(unsigned long long key) { return (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)); }

// ---- engine.cpp: shared-prefix registration, penalties
int share_clear(ti_engine* e);
int share_begin(ti_engine* e, int M, const int32_t* base, bool* use);
int pen_reset_slot(ti_engine* e, int m, const int32_t* head, int n_head, const int32_t* tail, int n_tail);
int pen_refuse(const ti_engine* e, const char* fn);

// ---- engine_guide.cpp: ti_engine_set_guide's state
int guide_refuse(const ti_engine* e, const char* fn);
int guide_start_slots(ti_engine* e, int first, int count);
int guide_enqueue(ti_engine* e, int M, StepMode mode);
int guide_reset_slot(ti_engine* e, int slot, int handle);

// ---- engine_step.cpp: projections, attention routing, the step plan and its epilogues
bool packed_rows(const ti_engine* e, int M);
int gemm_rows(ti_engine* e, const DevLinear& W, int M, const void* x, int x_kind, int ldx, const float* nw,
              const ti_epilogue& epi, size_t out_elem, bool last_gets_ctr);
int attn_merged(ti_engine* e, bool packed, const uint16_t* kc, const uint16_t* vc, int64_t stride, int M, int splits);
int attn_partials(ti_engine* e, const uint16_t* kc, const uint16_t* vc, int M, int splits);
bool fold_usable(ti_engine* e, int M);
bool qa_usable(ti_engine* e, int M);
int qa_fault_check(ti_engine* e);
// Which forms one decode step of M streams takes: enqueue_step launches by it, ti_engine_time_kernel times by it.
struct StepPlan {
  int M;
  bool fold;     // one stream: every rms_norm input handed over as fx + ss partials by its producer
  bool bfold;    // 17..64 int4 rows: O / down write xn and per-row sums of h^2, the consumers normalise behind the GEMM
  bool part;     // the O projection merges the attention's split partials
  bool qa;       // QKV + attention in one launch (ti_qkv_attn_partials)
  bool packed;   // fp16 operands in fragment order (TI_X_F16_PACKED)
  int splits;    // of the decode attention
};
StepPlan plan_step(ti_engine* e, int M);
void fold_into(const ti_engine* e, const StepPlan& p, ti_epilogue& ep, const float* w, int n_next);
void norm_in(const ti_engine* e, const StepPlan& p, int n_ss, int bn_ss, const void*& x, int& xk, int& ldx,
             const float*& nw, ti_epilogue& ep, int n);
ti_step_args step_args(const ti_engine* e, int M);
ti_epilogue qkv_epilogue(const ti_engine* e, uint16_t* kc, uint16_t* vc, int64_t stream_stride);
ti_epilogue resid_epilogue(const ti_engine* e);
ti_epilogue silu_epilogue(const ti_engine* e, bool packed);
ti_epilogue logits_epilogue(const ti_engine* e, float* out, bool argmax = true);
int enqueue_step(ti_engine* e, int M, StepMode mode);
// prompt chunks
enum PfAttn { PF_ATTN_MFMA = 0, PF_ATTN_DECODE = 1, PF_ATTN_DECODE_PACKED = 2 };
bool prefill_attn_on();
bool prefill_logits_on();
PfAttn prefill_attn_route(const ti_engine* e, int rows);
int prefill_chunk_rows(const ti_engine* e);
int enqueue_prefill(ti_engine* e, int m, int t0, int rows, int base);
int enqueue_prefill_layers(ti_engine* e, int m, int rows, int split_attn);
int prefill_tokens(ti_engine* e, int slot, int n, int base);
// the graph cache
int capture_graph(ti_engine* e, const std::function<int()>& enqueue, hipGraphExec_t* out);
int cached_graph(ti_engine* e, const GraphKey& key, const std::function<int()>& enqueue, hipGraphExec_t* out);
int drop_graphs(ti_engine* e);
int get_graph(ti_engine* e, int M, StepMode mode, hipGraphExec_t* out);
int run_steps(ti_engine* e, int M, StepMode mode, int n);
int ensure_io(ti_engine* e, int in_cap, int out_cap);
int read_argmax(ti_engine* e, int n, std::vector<unsigned long long>& keys);
int grow_step_draws(ti_engine* e, int need);
int sampler_prepare(ti_engine* e, float t, int k, float p, int ws_rows);
int sampler_ws_reserve(ti_engine* e, size_t bytes);
int pen_state_alloc(ti_engine* e);

// ---- engine_generate.cpp
int generate_impl(ti_engine* e, int n, const int32_t* prompts, const int32_t* lens, int stride, const int32_t* start_pos,
                  int max_new, bool sampled, int32_t* out_tokens, float* last_logits);

// ---- engine_beam.cpp
int fork_slot(ti_engine* e, int src, int dst, int n);

}  // namespace ti_eng
