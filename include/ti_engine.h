/*
 * ti_engine.h -- extern "C" decode engine: the device-resident state behind
 * turboinfer::model::InferenceEngine (its pimpl InferenceEngineImpl,
 * include/turboinfer/model/inference_engine.hpp:214 in the reference) exported as a flat
 * C-ABI so the benchmark, the tests and other-language hosts can drive it.
 *
 * Replaces, per decode step, InferenceEngine::forward_pass_incremental
 * (src/model/inference_engine.cpp:1493-1552) -> TransformerLayer::forward_incremental
 * (:244-279) -> KVCache::update_incremental (:78-160), plus greedy sample_next_token
 * (:1554-1673, top_k = 1) and the generate() loop (:734-802).
 *
 * One engine = one device + one HIP stream + B decode streams (requests) whose fp16 (or, with
 * TI_BITS_KV8, e4m3) KV caches live in that device's HBM.  Independent engines on different devices are
 * independent replicas (no collectives).
 */
#ifndef TI_ENGINE_H
#define TI_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ti_engine ti_engine;

typedef struct ti_engine_config {
  int32_t vocab, hidden, layers, heads, kv_heads, head_dim, inter;
  float rope_theta;        /* ModelMetadata::rope_theta (reference default 10000) */
  float eps;               /* rms_norm eps, reference default 1e-5 (tensor_engine.hpp:185) */
  int32_t bits;            /* weight format: 4 (INT4 g128), 8 (INT8 g128), 16 (fp16); | TI_BITS_KV8
                              (ti_hip.h): K / V kept as e4m3 bytes, half the cache memory -- the
                              one-stream fused QKV + attention launch is then off; prompt chunks
                              attend through ti_attn_prefill_f8 where an fp16-cache engine takes
                              ti_attn_prefill; not with compat (TI_ERR_ARG) */
  int32_t max_seq;         /* KV slots per stream */
  int32_t max_batch;       /* decode streams held by the engine */
  int32_t compat;          /* 1 = reference_compat: placeholder embeddings, attention
                              bypass, ReLU FFN, fp32 weights (benchmark plumbing model) */
  int32_t device;
  int32_t attn_splits;     /* 0 = auto */
} ti_engine_config;

enum ti_slot {
  TI_W_Q = 0, TI_W_K, TI_W_V, TI_W_O, TI_W_GATE, TI_W_UP, TI_W_DOWN, /* per layer, [K][N] */
  TI_W_LM_HEAD,                                                    /* [hidden][vocab]   */
  TI_V_ATTN_NORM, TI_V_FFN_NORM,                                   /* per layer, [hidden] */
  TI_V_OUT_NORM,                                                   /* [hidden] */
  TI_E_EMBED                                                       /* [vocab][hidden]   */
};

int ti_engine_create(const ti_engine_config* cfg, ti_engine** out);
int ti_engine_destroy(ti_engine* e);
int ti_engine_get_stream(ti_engine* e, void** stream);
int ti_engine_memory(ti_engine* e, size_t* weight_bytes, size_t* kv_bytes);

/* Upload one tensor given in the reference layout (fp32 host memory); linear weights are
 * quantized + packed per the engine's bits (scale_mode: ti_hip.h TI_SCALE_*). */
int ti_engine_set_tensor(ti_engine* e, int slot, int layer, const float* data, int scale_mode);
/* Engines created with bits = 4 or 8 | TI_BITS_G32 (ti_hip.h: group-32 weights, GGUF Q4_0 /
 * Q8_0 blocks): a linear weight given exactly, q int8 [K][N] (reference layout) and fp16 block
 * scales d [K/32][N], weight = d * q -- no re-quantization.  ti_engine_set_tensor on such an
 * engine quantizes fp32 weights per 32-block (absmax / 7 or / 127). */
int ti_engine_set_tensor_q(ti_engine* e, int slot, int layer, const int8_t* q, const uint16_t* d);
/* GGUF Q4_1 blocks (model_loader.cpp:165-182, ggml's format) kept exact on an engine with bits
 * 4 | TI_BITS_G32 | TI_BITS_AFF: q uint8 [K][N_src] (0..15), d and m fp16 [K/32][N_src],
 * weight = d * q + m (ti_wpack_q1_host). */
int ti_engine_set_tensor_q1(ti_engine* e, int slot, int layer, const uint8_t* q, const uint16_t* d, const uint16_t* m);
/* Synthetic model of SURVEY 8(d) generated on the device (bit-identical to the oracle's
 * or_model_synth for the same seed / jitter). */
int ti_engine_synth(ti_engine* e, uint64_t seed, float norm_jitter);
/* Fill KV slots [0, n) of `stream` (all layers) with seeded fp16 U(-1,1) (or_model_fill_kv). */
int ti_engine_fill_kv(ti_engine* e, int stream, int n, uint64_t seed);

/* (a TI_BITS_KV8 engine stores the e4m3 of exactly those fp16 values) */
/* Copy rows [pos0, pos0 + n) of one stream slot's K (which = 0) or V (which = 1) cache of `layer` to
 * the host as [kv_heads][n][head_dim] in the engine's own element type: fp16 bits (2 bytes), or e4m3
 * bytes on a TI_BITS_KV8 engine.  For inspecting or persisting a slot; synchronises the engine's
 * stream.  TI_ERR_ARG before any copy: null e / out, a compat engine, layer outside [0, layers),
 * stream outside [0, max_batch), which not 0 / 1, pos0 < 0, n < 1, pos0 + n > max_seq. */
int ti_engine_read_kv(ti_engine* e, int layer, int stream, int which, int pos0, int n, void* out);

/* Greedy generation for n_streams independent requests, entirely on the device: every
 * stream starts at position start_pos[s] (NULL = 0), consumes its prompt one token per
 * step, then feeds back its argmax.  out_tokens [n_streams][max_new] receives the first
 * max_new generated tokens; last_logits (nullable) [n_streams][vocab] the logits of the
 * final step. */
int ti_engine_generate(ti_engine* e, int n_streams, const int32_t* prompts, const int32_t* prompt_lens,
                       int prompt_stride, const int32_t* start_pos, int max_new, int32_t* out_tokens,
                       float* last_logits);

/* Stop token of ti_engine_generate / ti_engine_generate_sampled (-1 = none, the default).  When
 * set, the device loop runs in chunks of 4, 8, 16, 32, then 64 steps, and after each chunk the new
 * tokens are read back; the loop ends once every stream has emitted the token, as the reference's
 * generate() breaks at EOS (inference_engine.cpp:760-764, token id 2).  A stream's tokens end at its
 * first stop token (included); the rest of its max_new entries are -1. */
int ti_engine_set_stop(ti_engine* e, int32_t token);
/* Step-graph replays (decode steps, each covering every stream of its call) and prompt chunks
 * (prefill) this engine has run since it was created. */
int ti_engine_counters(ti_engine* e, uint64_t* decode_steps, uint64_t* prefill_chunks);
/* The graph cache since creation: graphs captured into it (a step or verify graph the cache did not hold), and
 * graphs dropped from it (a setter or a grown buffer changed something they bake in).  Two calls between which
 * neither number moves replayed the graphs they found.  Either pointer may be null. */
int ti_engine_graph_counters(ti_engine* e, uint64_t* captured, uint64_t* dropped);

/* A prompt prefix shared by the streams of a batch (a system prompt, a few-shot header): prefilled once,
 * attended once per step for all streams (ti_attn_decode_shared, ti_hip.h).
 * ti_engine_share_prefix prefills tokens[0 .. n) at positions [0, n) of slot 0 as prompt chunks, copies those
 * KV rows to slots 1 .. n_streams - 1 and registers (tokens, n, n_streams).  n == 0 clears the registration.  A
 * call whose tokens and n_streams equal the live registration returns at once (ti_engine_counters does not
 * move): the system-prompt cache across calls.  While registered, rows [0, n) of slots [0, n_streams) are
 * identical and nobody writes them: an entry point that would write such a row (ti_engine_fill_kv,
 * ti_engine_beam_search; ti_engine_generate / _generate_sampled / _score / the lookahead calls / ti_engine_step
 * with a start position below n) clears the registration before it enqueues anything and then behaves as
 * without one.  A change of registration drops the captured step graphs (the prefix length is baked in).
 * Use: requests pass only their continuation as the prompt, with start_pos[m] = n.  ti_engine_generate,
 * ti_engine_generate_sampled and ti_engine_step with 2 <= streams <= n_streams, every start position >= n and
 * n >= TI_SHARE_MIN (environment, read when the engine is created) run their batched steps on
 * ti_attn_decode_shared; one-stream steps and prompt chunks are as ever (each slot holds its copy).
 * ti_engine_serve / _serve_sampled under a registration with n_streams == max_batch treat each request's prompt
 * as the continuation behind the prefix (room: n + prompt + max_new - 1 <= max_seq; idle slots sit at position
 * n); with fewer streams registered they clear it.
 * TI_ERR_ARG: null e, null tokens with n > 0, n < 0, n >= max_seq, n_streams outside [2, max_batch], a token
 * outside [0, vocab).  TI_ERR_UNSUPPORTED: a compat engine, a TI_BITS_KV8 engine. */
int ti_engine_share_prefix(ti_engine* e, const int32_t* tokens, int n, int n_streams);
/* The live registration's prefix length and streams (0, 0 when none); either pointer may be null. */
int ti_engine_shared_prefix(ti_engine* e, int* len, int* n_streams);

/* ti_engine_generate with the reference sampler on the device: after each
 * step's lm_head, ti_sample_step applies sample_next_token (inference_engine.cpp:1554-1673:
 * temperature, top-k, softmax, top-p, the draw) and feeds the token back, so the loop never
 * returns to the host.  draws [n][max_new]: the uniform draw of each stream's t-th new token
 * (the reference takes them from its engine's mt19937, uniform_real_distribution<float>);
 * 1 <= top_k <= vocab (above TI_SAMPLE_MAX_K the engine keeps a sampler workspace).  out_logprobs (nullable) [n][max_new] = log p of
 * each sampled token. */
int ti_engine_generate_sampled(ti_engine* e, int n_streams, const int32_t* prompts, const int32_t* prompt_lens,
                               int prompt_stride, const int32_t* start_pos, int max_new, float temperature,
                               int top_k, float top_p, const float* draws, int32_t* out_tokens, float* out_logprobs);

/* Repetition, presence and frequency penalties of the sampled device loops (no reference counterpart: its
 * GenerationConfig has none; the arithmetic is llama.cpp's llama_sampler_penalties_apply with
 * penalty_last_n = -1, ti_hip.h ti_penalty_step).  Engine state, like ti_engine_set_stop.  A stream's context
 * is the token sequence its request has consumed so far: the prompt, then its generated tokens; count[v] is
 * the number of occurrences of v in it, with no window.  Before the sampler sees a row of raw logits (before
 * temperature), every token with count[v] > 0 is rewritten:
 *   a = l <= 0 ? l * repetition : l / repetition;  out = a - (float(count) * frequency + presence)
 * each step rounded once to fp32.  (1, 0, 0), the default, means off: the engine then enqueues exactly what
 * it does without this call.  While the values differ from (1, 0, 0) the penalties are active:
 *   ti_engine_generate_sampled: the context is the prompt as passed (whether its tokens run as prompt chunks
 *     or decode steps), then the stream's new tokens.  Under a live ti_engine_share_prefix registration a
 *     stream with start_pos == the prefix length has the registered prefix tokens at the head of its context,
 *     so a registered run penalises what the unregistered run of the full prompts would.  With any other
 *     start_pos > 0 only the tokens passed count: the engine does not know what the slot's earlier KV rows were.
 *   ti_engine_serve_sampled: the request's prompt (behind the registered prefix when the loop treats prompts
 *     as continuations), then its new tokens, whatever slot and chunk they run in; a slot freed by one
 *     request starts empty for the next.
 *   top_k = 1 through either is greedy decoding with penalties.
 *   ti_engine_generate, ti_engine_serve, both lookahead calls and ti_engine_beam_search produce tokens and
 *     cannot penalise: TI_ERR_UNSUPPORTED, naming the function, before anything is enqueued.
 *   ti_engine_step, ti_engine_score, the replay / timing entry points return the model's own numbers.
 * The values and the state buffers (token counts and distinct-token lists for max_batch slots, a context
 * upload scratch, the serve loop's carry row; allocated on the first activation, outside what
 * ti_engine_memory reports) are baked into the step graphs: a change of values drops the captured graphs.
 * TI_ERR_ARG: null e, repetition not finite and > 0, presence or frequency not finite.
 * TI_ERR_UNSUPPORTED: a compat engine. */
int ti_engine_set_penalties(ti_engine* e, float repetition, float presence, float frequency);
/* The values in force ((1, 0, 0) when never set); any pointer may be null. */
int ti_engine_get_penalties(ti_engine* e, float* repetition, float* presence, float* frequency);

/* Token-automaton guided decoding in the sampled device loops (no reference counterpart).  The
 * engine has no tokenizer, so a constraint -- JSON or regex shaped text, a choice set, banned tokens, a forced
 * continuation -- arrives as constrained-decoding toolkits precompute it: a deterministic automaton over token
 * ids, state -> {token id -> next state}, as CSR on the host:
 *   n_states >= 1, start in [0, n_states)
 *   row_ptr [n_states + 1]  row_ptr[0] = 0, non-decreasing; nnz = row_ptr[n_states]
 *   tokens  [nnz]           strictly ascending within a state, each in [0, vocab)
 *   next    [nnz]           each in [0, n_states)
 * and every state has at least one transition (a state that allows nothing would hand the sampler a row
 * without a finite entry).  ti_guide_check validates exactly this (TI_ERR_ARG naming the first violation).
 * Per stream slot the engine keeps one int32 state, -1 = free or dead: the row is left alone.  For the row that
 * produces a stream's new token t (the sampler's own index), with 0 <= t < the draw capacity:
 *   1. the token this step fed is consumed when it is a generated one (for t >= 1 the stream's token t - 1; for
 *      t == 0 the serve loop's carry token): state <- next of that token in the state, or -1 when the state has
 *      no such transition (after a stop token in a lock-step batch; the sampler's u <= 0 and last-token
 *      fall-backs);
 *   2. with state >= 0, every column v < vocab that is not a transition of the state becomes -inf (bits
 *      0xFF800000); every allowed column keeps its bits.
 * The prompt is not run through the automaton: a request starts in `start`.  Order in the step: lm_head,
 * ti_penalty_step (when penalties are active), ti_guide_step, the sampler; reported log-probabilities are
 * those of the constrained distribution.  top_k = 1 is constrained greedy decoding; a one-state automaton that
 * omits some ids is a token ban; a chain of one-transition states forces a continuation. */
typedef struct ti_guide {
  int32_t n_states;
  int32_t start;
  const int64_t* row_ptr;
  const int32_t* tokens;
  const int32_t* next;
} ti_guide;
/* Engine state, like ti_engine_set_penalties: the guide is copied to the device with a per-state allow-bitmask
 * (buffers outside what ti_engine_memory reports, replaced by the next call), every slot's state becomes -1 and
 * the captured graphs are dropped.  A null g clears the guide; with none set the engine enqueues exactly what
 * it does without this call.  While a guide is set:
 *   ti_engine_generate_sampled puts every stream in `start` before its first step and runs ti_guide_step in
 *     its step graph (shared prefix included).
 *   ti_engine_serve_sampled puts a slot in `start` when a request is admitted into it, and passes each
 *     chunk's input token in the carry row, whatever slot and chunk a request runs in.
 *   ti_engine_generate, ti_engine_serve, both lookahead calls and ti_engine_beam_search produce tokens and
 *     cannot follow a guide: TI_ERR_UNSUPPORTED, naming the function, before anything is enqueued.
 *   ti_engine_step, ti_engine_score, the replay / timing entry points return the model's own numbers.
 * One automaton per engine through this call; requests that need different automata, or none, in one batch name
 * guides of the engine's library instead (ti_engine_add_guide, ti_engine_serve_requests_guided, below).  Any KV
 * format.
 * TI_ERR_ARG: null e, a guide ti_guide_check rejects for the engine's vocab.  TI_ERR_UNSUPPORTED: a compat engine. */
int ti_engine_set_guide(ti_engine* e, const ti_guide* g);
/* out [max_batch]: every slot's current state (-1 everywhere when no guide is set).  After a sampled call a
 * slot holds the state its last step masked with: every generated token but the last consumed (a step consumes
 * the token it is fed); a caller that continues a request advances it by that last token (ti_guide_apply).  In a
 * lock-step batch of unequal prompt lengths, or behind a stop token, a stream steps on to the batch's last step
 * and its state follows the tokens of those steps, which the call does not return. */
int ti_engine_guide_states(ti_engine* e, int32_t* out);

/* The guide library: up to TI_GUIDE_CAP guides live on the engine at once, and each request of
 * ti_engine_serve_requests_guided names one by its handle, or none.  Handle h is entry h - 1 of a device table of
 * ti_guide_dev descriptors (ti_hip.h ti_guide_step_rows), all-zero where unused; the step graphs bake in the
 * table's pointer, never an entry, so neither call below drops a captured graph.
 * ti_engine_add_guide validates g with ti_guide_check, builds the per-state allow-bitmask as ti_engine_set_guide
 * does, uploads both (buffers outside what ti_engine_memory reports, as are the table and -- allocated by the
 * first add when absent -- the slots' state row and carry row), takes the lowest free handle (1 .. TI_GUIDE_CAP,
 * *out_handle) and writes that one table entry in stream order.  The host keeps the handle's `start`.
 * ti_engine_remove_guide synchronises the stream, zeroes the entry (handle 0: every entry) and frees its buffers;
 * a zeroed entry is inert.  ti_engine_guide_count: live handles.
 * The library is inert until a request names a handle: no other entry point refuses, changes its launch list or
 * reads it, and ti_engine_set_guide and its single guide are independent of it.
 * TI_ERR_ARG: null e / g / out_handle / out, a guide ti_guide_check rejects for the engine's vocab, a full library,
 * a handle outside [0, TI_GUIDE_CAP] or (other than 0) not live.  TI_ERR_UNSUPPORTED: add on a compat engine. */
#define TI_GUIDE_CAP 64
int ti_engine_add_guide(ti_engine* e, const ti_guide* g, int* out_handle);
int ti_engine_remove_guide(ti_engine* e, int handle);
int ti_engine_guide_count(ti_engine* e, int* out);

/* InferenceEngine::generate_beam_search (inference_engine.cpp:830-871, 1912-2069): the
 * reference's beam loop (max-heap on log-probability, expansion by the beam_size most probable
 * tokens after temperature / softmax / top-k / top-p renormalisation (:1798-1910), length-
 * normalised ranking log_prob / len^length_penalty, early stop at beam_size finished beams),
 * with each candidate's next-token distribution from its last position's logits.  Every live
 * beam owns a stream slot holding its KV cache: one batched decode step per expansion round, a
 * fork copies the parent's cache prefix (the reference recomputes each candidate, :1961), so
 * beam_size <= max_batch.  max_new = 0 returns the prompt as one finished beam (no tokens).
 * Results best first: out_tokens [beam_size][max_new] (new tokens, -1 padded), out_log_prob,
 * out_score (normalised), out_finished [beam_size] (nullable), *out_count beams returned. */
int ti_engine_beam_search(ti_engine* e, const int32_t* prompt, int prompt_len, int max_new, int beam_size,
                          float temperature, int top_k, float top_p, float length_penalty, int eos_token,
                          int32_t* out_tokens, float* out_log_prob, float* out_score, int32_t* out_finished,
                          int* out_count);

/* Continuous batching (generate_batch, inference_engine.cpp:804-828, at
 * serving scale): n_req greedy requests through the engine's max_batch stream slots.  The
 * device loop runs in chunks of up to `chunk` steps; between chunks, requests that ended
 * (eos_token, max_new) leave their slot and queued requests take it: the prompt is prefilled
 * into that slot's KV and the request joins the next chunk at its last prompt token, while the
 * other slots continue at their own positions.  prompts: concatenated token ids, request r
 * = prompts[offsets[r] .. offsets[r+1]); out_tokens [n_req][max_new] (-1 padded), out_len
 * [n_req] = tokens produced (the eos token included). */
int ti_engine_serve(ti_engine* e, int n_req, const int32_t* prompts, const int32_t* offsets, int max_new, int eos_token,
                    int chunk, int32_t* out_tokens, int32_t* out_len);
/* ti_engine_serve with the step graph's sampler on (ti_sample_step, as in ti_engine_generate_sampled):
 * request r's t-th new token is sample_next_token(its logits, temperature, top_k, top_p, draws[r][t]),
 * whatever slot and chunk it runs in.  Every chunk starts at step 0 with one token per slot, so before a chunk
 * the host places each live slot's next draws into that slot's row of the engine's draw buffer, and after it
 * reads the slot's log-probabilities back.  Draws of a request cut short by eos_token are unused.
 * draws (host, [n_req][max_new]); out_logprobs (host, [n_req][max_new], nullable): log p of each token, 0.0
 * past out_len.  1 <= top_k <= vocab; top_k = 1 returns ti_engine_serve's tokens.  The sampler's parameters
 * and buffers are baked into the step graphs: a change drops them (ti_engine_generate_sampled).
 * TI_ERR_ARG before anything is enqueued: ti_engine_serve's, null draws, top_k outside [1, vocab]. */
int ti_engine_serve_sampled(ti_engine* e, int n_req, const int32_t* prompts, const int32_t* offsets, int max_new,
                            int eos_token, int chunk, float temperature, int top_k, float top_p, const float* draws,
                            int32_t* out_tokens, int32_t* out_len, float* out_logprobs);
/* ti_engine_serve_sampled with every request carrying its own budget, stop token, sampler parameters and
 * penalties, all of them through one loop and one batch (a greedy extraction next to a creative completion).
 * The launches between the lm_head and the feedback read each stream row's values from a device table
 * [max_batch] of ti_row_params (ti_hip.h: ti_penalty_step_rows, ti_guide_step when a guide is set -- the
 * engine's one guide, for every request, as in ti_engine_serve_sampled; per-request guides are
 * ti_engine_serve_requests_guided's, below -- and ti_sample_step_rows).  The step
 * graph bakes in the table's pointer only; before a chunk that follows an admission or a departure the host
 * copies the table in stream order, as it does the draws (idle slots hold temperature 1, top_k 1, top_p 1,
 * penalties (1, 0, 0)).  So different parameters, within a call or between calls, drop no graph.
 *   params [n_req]; draws, out_tokens (-1 padded), out_logprobs (nullable; 0.0 past out_len) are host
 *   [n_req][out_stride] with out_stride >= every max_new; out_len [n_req].
 *   A request ends at its own max_new or its own stop_token (included, as eos_token is).
 *   ti_penalty_step_rows is in the graph only when some request of the call penalises (values other than
 *   (1, 0, 0)); only then is the penalty state allocated (as ti_engine_set_penalties allocates it), and a slot's
 *   histogram is reset at admission only for a request that penalises: from the registered prefix, when the loop
 *   treats prompts as continuations of it, and the prompt.
 *   When some request's top_k exceeds TI_SAMPLE_MAX_K the call's graph runs every row on the sampler's
 *   workspace instance (the engine's workspace grows to max_batch rows of vocab; growing a buffer drops graphs).
 *   ti_engine_set_penalties' values and ti_engine_set_stop do not apply to this call and are not changed by it.
 * Contract: request r's tokens and log-probabilities are bit for bit what ti_engine_serve_sampled returns for r
 * on an engine of the same shape and max_batch called with r's (max_new, stop_token as eos_token, temperature,
 * top_k, top_p) and draws[r], ti_engine_set_penalties set to r's three values -- whatever the other requests'
 * parameters, the slot and the chunking are (the batched kernels compute every row from its own inputs).
 * Exception: in a call where some request has top_k > TI_SAMPLE_MAX_K, rows are the sampler's tokens for their own
 * parameters (pinned to the host sampler) but not promised bit-equal to the LDS instance's.
 * TI_ERR_ARG before anything is enqueued, naming the request: ti_engine_serve_sampled's checks, null params,
 * max_new < 1 or > out_stride, stop_token outside [-1, vocab), top_k outside [1, vocab], penalty values
 * ti_engine_set_penalties would reject, registered prefix + prompt + the request's max_new - 1 beyond max_seq.
 * TI_ERR_UNSUPPORTED: a compat engine. */
typedef struct ti_request_params {
  int32_t max_new;                          /* >= 1 */
  int32_t stop_token;                       /* -1: none */
  float temperature;
  int32_t top_k;                            /* 1 <= top_k <= vocab */
  float top_p;
  float repetition, presence, frequency;    /* (1, 0, 0): off */
} ti_request_params;                        /* 32 bytes */
int ti_engine_serve_requests(ti_engine* e, int n_req, const int32_t* prompts, const int32_t* offsets,
                             const ti_request_params* params, int chunk, const float* draws, int out_stride,
                             int32_t* out_tokens, int32_t* out_len, float* out_logprobs);
/* ti_engine_serve_requests with request r under the library guide guides[r] (host, [n_req]; a handle of
 * ti_engine_add_guide, or 0 for none; guides nullable): the greedy extraction takes its JSON or choice-set automaton
 * into the same batch as the creative completion that must not have one.  With a null guides, or every handle 0,
 * the call IS ti_engine_serve_requests (which is this call with guides == NULL) and enqueues exactly what that does.
 * When some request names a handle:
 *   the slot's entry of the ti_row_params table carries the handle in reserved[0] (0 for an unguided request and
 *     for an idle slot), and ti_guide_step_rows -- behind the penalty launch, before the sampler -- is in the
 *     call's step graph (its own graph key, like the penalty launch's); the carry row is on;
 *   at admission the slot's state is reset to the start state of the request's guide, or to -1 for a request
 *     without one (ti_engine_guide_states then reads -1 for that slot);
 *   the prompt, and a registered shared prefix before it, is not run through the automaton.
 * Contract: request r's tokens and log-probabilities are bit for bit what ti_engine_serve_requests returns for r on
 * a fresh engine of the same shape and max_batch with ti_engine_set_guide set to r's guide (no guide set for
 * handle 0) -- whatever the other requests' guides and parameters, the slot and the chunking.  The workspace-instance
 * exception of ti_engine_serve_requests holds unchanged.  Any KV format.
 * TI_ERR_ARG before anything is enqueued, naming the request: ti_engine_serve_requests', a handle outside
 * [0, TI_GUIDE_CAP], a handle that is not live.  TI_ERR_UNSUPPORTED: some request names a handle while
 * ti_engine_set_guide's guide is set (one source of constraint per call); a compat engine. */
int ti_engine_serve_requests_guided(ti_engine* e, int n_req, const int32_t* prompts, const int32_t* offsets,
                                    const ti_request_params* params, const int32_t* guides, int chunk,
                                    const float* draws, int out_stride, int32_t* out_tokens, int32_t* out_len,
                                    float* out_logprobs);

/* Teacher-forced scoring of a token sequence on the device (InferenceEngine::compute_logprobs,
 * inference_engine.cpp:873-954; Quantizer::validate_quantization_accuracy is built on it,
 * quantization.cpp:548-549).  tokens[i] (host, [n]) is fed at position start_pos + i of stream slot
 * `stream`, after whatever that slot's KV cache holds in [0, start_pos); out_logprob[i] (host, [n])
 * is the log-probability of targets[i] under the model's output distribution after tokens[0..i],
 * and out_top1[i] (host, [n], nullable) that distribution's argmax (lowest index on ties).
 * targets (host, [n]): -1 = no target (0.0); NULL = tokens, the reference's own indexing (:934-942:
 * position pos scores tokens[pos] with logits[pos]).  Perplexity passes targets[i] = tokens[i+1]
 * and targets[n-1] = -1.
 * The tokens run as prefill chunks (ti_engine_set_prefill's rows; when that is 0, the chunk
 * ti_engine_serve uses), never as decode steps; after each chunk the final rms_norm + lm_head run on
 * every row, TI_SCORE_ROWS rows at a time, into a logits scratch ([TI_SCORE_ROWS][vocab] fp32,
 * allocated by the first call, outside what ti_engine_memory reports and outside the step graphs),
 * and ti_logprob_rows (ti_hip.h) reduces each row to its two numbers.  One synchronisation and one
 * copy of the n results at the end.  On return the slot's KV rows [start_pos, start_pos + n) hold
 * what a prefill of the same tokens writes: ti_engine_generate or ti_engine_score with
 * start_pos + n continues from there.  ti_engine_counters: prefill_chunks rises by the number of
 * chunks, decode_steps does not move.
 * TI_ERR_ARG, before anything is enqueued: null e / tokens / out_logprob, n < 1, stream outside
 * [0, max_batch), start_pos < 0, start_pos + n > max_seq, a token outside [0, vocab), a target
 * outside [-1, vocab).  TI_ERR_UNSUPPORTED: a compat engine. */
#define TI_SCORE_ROWS 128
int ti_engine_score(ti_engine* e, int stream, const int32_t* tokens, int n, int start_pos, const int32_t* targets,
                    float* out_logprob, int32_t* out_top1);

/* Lookahead greedy decoding of ONE request in stream slot `stream` (no reference counterpart: the reference's
 * generate() runs one forward pass per token, inference_engine.cpp:734-802).  Each verify step feeds the
 * last token and up to k tokens drafted by an n-gram lookup in corpus ++ prompt ++ generated (ti_hip.h
 * ti_lookahead_begin) as k + 1 rows of one prompt chunk -- weights read once, the attention by
 * ti_attn_prefill_split -- and keeps the drafts the rows' greedy tokens confirm (ti_lookahead_accept): between
 * 1 and k + 1 tokens of exactly the greedy sequence per step.  prompt[0 .. n - 2] run as prompt chunks,
 * prompt[n - 1] is row 0 of the first step.  The step is one captured graph per (slot, k, splits), kept with
 * the step graphs; it replays in chunks of 4, 8, 16, 32, then 64 with one small read-back of the device state
 * after each, until done, at most max_new steps.  The k + 1 rows' logits and the history live in buffers
 * allocated by the first call, outside what ti_engine_memory reports.  The verify step runs without the
 * folded rms_norm and without the fused QKV + attention launch (both are one-row paths).
 * corpus (host, [corpus_len], nullable with corpus_len 0): reference text the continuation may repeat.
 * out_tokens (host, [max_new]): the greedy tokens, -1 after a stop token (ti_engine_set_stop applies; the
 * stop token is included).  stats (nullable): verify steps run, drafts proposed, drafts accepted, tokens
 * produced.  ti_engine_counters: decode_steps rises by the verify steps, prefill_chunks by the prompt chunks.
 * On return the slot's KV rows [start_pos, start_pos + prompt_len + produced - 1) are what
 * ti_engine_generate would have left; the next k rows are scratch (rejected drafts).  Generation continues
 * from there with either entry point (the last produced token as prompt, start_pos + prompt_len + produced - 1).
 * TI_ERR_ARG before anything is enqueued: null e / prompt / out_tokens, null corpus with corpus_len != 0,
 * stream outside [0, max_batch), prompt_len < 1, max_new < 1, k outside [1, 15], ngram outside [1, 8],
 * corpus_len < 0, a prompt or corpus token outside [0, vocab), start_pos < 0,
 * start_pos + prompt_len + max_new - 1 + k > max_seq (the verify rows need k slots of head-room).
 * TI_ERR_UNSUPPORTED: a compat engine, a TI_BITS_KV8 engine. */
typedef struct ti_lookahead_stats { int32_t steps, drafted, accepted, produced; } ti_lookahead_stats;
int ti_engine_generate_lookahead(ti_engine* e, int stream, const int32_t* prompt, int prompt_len, int start_pos,
                                 const int32_t* corpus, int corpus_len, int k, int ngram, int max_new,
                                 int32_t* out_tokens, ti_lookahead_stats* stats);

/* Lookahead decoding of ONE SAMPLED request: new token number t (0-based) is sample_next_token(logits after
 * the text so far, temperature, top_k, top_p, draws[t]) -- what ti_engine_generate_sampled computes for one
 * stream with the same draws -- several tokens per verify step.  The step is ti_engine_generate_lookahead's
 * with ti_lookahead_sample (ti_hip.h) between the lm_head and ti_lookahead_accept: row j is sampled with
 * draws[produced + j], and draft j + 1 is kept iff it equals row j's sampled token.  This is not rejection
 * sampling: the output is the sequential sampler's sequence for these draws, up to rounding between kernel
 * routes (the verify rows run the batched-rows kernels, a decode step the one-row ones).  top_k = 1 is the
 * greedy call with log-probabilities.
 * Everything ti_engine_generate_lookahead documents applies: the prompt chunks, the chunked replay with the
 * state read-back, ti_engine_set_stop, the counters, the k rows of head-room, what the slot's KV holds on return
 * and how generation continues.  draws (host, [max_new]).  out_logprobs (host, [max_new], nullable): log p of
 * each sampled token, 0.0 where out_tokens is -1.
 * The sampled verify graph is cached next to the greedy one (its own key); both stay valid side by side.  The
 * sampler's parameters, its workspace (top_k > TI_SAMPLE_MAX_K: TI_LA_MAX_K + 1 rows) and the device draw /
 * log-probability buffers are baked into it: when one of them changes or grows, every cached graph is dropped
 * and recaptured on demand, as ti_engine_generate_sampled does.
 * TI_ERR_ARG before anything is enqueued: those of ti_engine_generate_lookahead, null draws, top_k outside
 * [1, vocab].  TI_ERR_UNSUPPORTED: a compat engine, a TI_BITS_KV8 engine. */
int ti_engine_generate_lookahead_sampled(ti_engine* e, int stream, const int32_t* prompt, int prompt_len, int start_pos,
                                         const int32_t* corpus, int corpus_len, int k, int ngram, int max_new,
                                         float temperature, int top_k, float top_p, const float* draws,
                                         int32_t* out_tokens, float* out_logprobs, ti_lookahead_stats* stats);

/* Prefill of ti_engine_generate's prompts (reference forward_pass, inference_engine.cpp:
 * 1429-1491): all but the last token of the shortest prompt are processed `rows` tokens at a
 * time as rows of the batched GEMMs and causal attention over the stream's own KV cache,
 * instead of one token per decode step.  Greedy streams whose prompts have one length (at least
 * 2 tokens) run the last token as a prefill row too, and their first token comes from the final
 * rms_norm + lm_head on that row (env TI_PREFILL_LOGITS=0: a decode step instead).
 * Default: TI_GEMM_MAX_ROWS (int4) or 16; 0 = off. */
int ti_engine_set_prefill(ti_engine* e, int rows);
/* The attention entry point (ti_hip.h) a prompt chunk of `rows` rows takes on this engine, as a label
 * in the style of ti_gemm_kernel_name: "ti_attn_prefill" / "ti_attn_prefill_f8" (row-major chunks: up
 * to 16 rows, and more than 64 on int4 engines), "ti_attn_decode_packed" / "ti_attn_decode_packed_f8"
 * (packed chunks: int4, 17-64 rows), "ti_attn_decode" / "ti_attn_decode_f8" (row-major chunks under
 * env TI_ATTN_PREFILL=0); the _f8 names on a TI_BITS_KV8 engine.  Decided by the predicates the
 * prefill itself launches by.  TI_ERR_ARG: null e / buf, rows < 1, len < 1; TI_ERR_UNSUPPORTED: a
 * compat engine. */
int ti_engine_prefill_attn_name(ti_engine* e, int rows, char* buf, int len);

/* Fused hand-offs of single-stream steps: (1) the folded rms_norm (ti_hip.h TI_X_F16_FOLDED):
 * the epilogue that updates the residual also writes fp16(h * next norm weight) and
 * per-workgroup sums of h^2, and the next projection divides its outputs by the rms instead of
 * normalising its input first; (2) the attention's split partials (ti_attn_decode_partials)
 * merged by the O projection (TI_X_ATTN_SPLITS) when the step uses 2..8 splits.  Default on
 * (env TI_FOLD=0 / TI_ATTN_PART=0 turn them off one by one).
 * on = 0/1 sets both, -1 leaves them; *active (nullable) receives whether 1-stream steps fold. */
int ti_engine_set_fold(ti_engine* e, int on, int* active);

/* QKV and attention of single-stream steps in one launch (ti_hip.h ti_qkv_attn_partials; int4 / int8
 * weights, hidden <= 4096, with the fold and split partials on, at head_dim 64 GQA (TinyLlama-1.1B)
 * and head_dim 128 MHA (Llama-2-7B); ti_qkv_attn_supported decides).  Default on (env TI_QKV_ATTN=0
 * turns it off).  Replaces round 4's function of the same name (removed then), with new semantics.
 * on = 0/1 sets it, -1 leaves it; *active (nullable) receives whether 1-stream steps of this engine
 * use it.  Changing it drops the engine's captured step graphs. */
int ti_engine_set_qkv_attn(ti_engine* e, int on, int* active);

/* One decode step: token[s] at position pos[s] for each stream; logits [n][vocab] to host
 * (used for non-greedy sampling and per-step parity). */
int ti_engine_step(ti_engine* e, int n_streams, const int32_t* tokens, const int32_t* pos, float* logits);

/* reference_compat step (compat engines): placeholder row offset, logits [vocab] to host. */
int ti_engine_compat_step(ti_engine* e, int placeholder_offset, float* logits);

/* Benchmark replay: every stream decodes at fixed position kv_len - 1 (reads
 * exactly kv_len cache slots), greedy feedback from start_token.  prepare captures the
 * step graph; run enqueues `steps` replays without synchronising. */
int ti_engine_replay_prepare(ti_engine* e, int n_streams, int kv_len, int start_token);
int ti_engine_replay_run(ti_engine* e, int steps);
int ti_engine_sync(ti_engine* e);
/* tokens decided by the last replay step, [n_streams] */
int ti_engine_last_tokens(ti_engine* e, int n_streams, int32_t* tokens);

/* In-step launch timing (bench.py's roofline; not a reference interface -- the reference
 * times wall clock only, benchmarks/benchmark_inference.cpp:309-384).  The replay step graph
 * (ti_engine_replay_prepare) is captured again with every decode kernel writing, per workgroup,
 * s_memrealtime stamps (100 MHz) of wave 0's entry and of each wave's end into an engine-owned
 * device buffer; `steps` (<= 256) steps are captured back to back into one graph, which is launched
 * once untimed and once read.  Per launch i < min(*n_launch, cap): info[3 i ..] = {kind, tag, workgroups} (workgroups 0:
 * the launch writes no stamps) and t[TI_STAMP_FIELDS i ..] the means over the steps, in us, of
 *   [0] span    first workgroup entry -> last wave end
 *   [1] period  first entry -> the next launch's first entry (the next step's first launch after a
 *               step's last): the launch's share of the step, its boundary included (the very last
 *               launch: its span + the mean boundary)
 *   [2] entry skew  first -> last workgroup entry
 *   [3] wave skew   per workgroup, first -> last wave end, averaged over the workgroups
 *   [4] tail        median workgroup end -> last wave end
 *   [5] gap         last wave end -> the next launch's first entry (the boundary; the last launch: the mean)
 *   [6] workgroups that ran on a CU another workgroup of the launch also ran on (a count)
 *   [7..12] diagnostic builds (TI_STAMP_PHASES): wave 0's phase marks, entry -> mark, workgroup mean
 *   [13]    diagnostic builds: per workgroup, first -> last wave's end of stream, workgroup mean
 * *n_launch receives the launches per step.  With env TI_STAMP_RAW=<file> the stamp words as read are
 * also written to that file (per-workgroup questions: tools/stamp_split_ends.py). */
#define TI_STAMP_FIELDS 14
enum { TI_STAMP_KIND_OTHER = 0, TI_STAMP_KIND_GEMV = 1, TI_STAMP_KIND_ATTN = 2, TI_STAMP_KIND_BEGIN = 3,
       TI_STAMP_KIND_ROWS = 4, TI_STAMP_KIND_TILE = 5, TI_STAMP_KIND_RMSNORM = 6, TI_STAMP_KIND_MB = 7 };
enum { TI_STAMP_TAG_BEGIN = 0, TI_STAMP_TAG_QKV = 1, TI_STAMP_TAG_ATTN = 2, TI_STAMP_TAG_O = 3,
       TI_STAMP_TAG_GATE_UP = 4, TI_STAMP_TAG_DOWN = 5, TI_STAMP_TAG_LM_HEAD = 6, TI_STAMP_TAG_OTHER = 7 };
int ti_engine_stamp_steps(ti_engine* e, int steps, int cap, int32_t* info, double* t, int* n_launch);

/* Live per-kernel timing: the step's launches of class `which` (0 qkv, 1 o, 2 gate/up,
 * 3 down, 4 lm_head, 5 attention), `reps` of them cycling through the layers,
 * captured into a graph that is replayed back to back (several ms) between two HIP events on
 * the engine stream.  avg_us = average per launch; bytes = algorithmic HBM bytes per launch. */
int ti_engine_time_kernel(ti_engine* e, int which, int n_streams, int kv_len, int reps, double* avg_us,
                          double* bytes);

/* ------------------------------------------------------------- host helpers */
/* RoPE (cos, sin) pairs for each of npos positions: out [npos][head_dim/2][2], computed on the
 * host with the reference formula (tensor_engine.cpp:1561-1566, 1595-1597) in fp32 libm. */
int ti_rope_table(const float* pos, int npos, int head_dim, float theta, float* out);
/* InferenceEngine::sample_next_token (inference_engine.cpp:1554-1673) with the uniform draw u
 * supplied: temperature, top-k (std::sort ranking, reference tie order), softmax, top-p. */
int ti_sample_token(const float* logits, int vocab, float temperature, int top_k, float top_p, float u,
                    int* token, float* logprob);
/* The penalties of ti_engine_set_penalties on the host, bit for bit the device's arithmetic (ti_hip.h
 * ti_penalty_step), for callers' own loops over ti_engine_step + ti_sample_token: logits [vocab] is rewritten
 * in place at every token that occurs in context[0 .. n) (ids outside [0, vocab) are ignored); all other
 * elements, and every element under (1, 0, 0), keep their bits.  TI_ERR_ARG: null logits, vocab < 1, n < 0,
 * null context with n > 0, repetition not finite and > 0, presence or frequency not finite. */
int ti_penalize_logits(float* logits, int vocab, const int32_t* context, int n, float repetition, float presence,
                       float frequency);
/* The guide of ti_engine_set_guide on the host, bit for bit what the device writes (ti_hip.h ti_guide_step),
 * for callers' own loops over ti_engine_step + ti_sample_token.  ti_guide_check validates g for a vocabulary
 * (the contract above): TI_OK, or TI_ERR_ARG naming the first violation.  ti_guide_apply takes a slot's state
 * (-1: free or dead), first consumes fed_token (-1: none; a token the state has no transition on leads to -1),
 * stores the new state in *out_state (nullable), and with a new state >= 0 sets every logits[v], v < vocab, that
 * is not a transition of it to -inf; all other elements, and every element under a state of -1, keep their
 * bits.  logits may be null (advance only).  g is taken as checked.  TI_ERR_ARG: null g, vocab < 1, state
 * outside [-1, n_states), fed_token < -1. */
int ti_guide_check(const ti_guide* g, int vocab);
int ti_guide_apply(const ti_guide* g, int vocab, int state, int fed_token, float* logits, int* out_state);

#ifdef __cplusplus
}
#endif
#endif /* TI_ENGINE_H */
