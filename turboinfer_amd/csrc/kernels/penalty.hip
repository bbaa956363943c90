// penalty.hip -- repetition / presence / frequency penalties on a stream's whole context, applied to the raw
// logits between the lm_head and the sampler (ti_hip.h ti_penalty_step).
//
// llama.cpp's llama_sampler_penalties_apply with penalty_last_n = -1: for every token v that occurs in the
// stream's context (count[v] > 0)
//   a = l <= 0 ? l * repetition : l / repetition;  b = float(count) * frequency;  d = b + presence;  out = a - d
// each step rounded once to fp32.  The file compiles with -ffp-contract=off (Makefile), so b + presence and
// a - d stay an add and a subtract (hipcc's default would contract them into fmas; the __f*_rn intrinsics
// are plain operators in this toolchain and would contract the same way), and the division is the
// correctly rounded one: a NumPy float32 restatement matches bit for bit (tests/penalty_ref.py).
//
// The state per stream slot is a histogram counts[V] and the list seen[0 .. n_seen) of its non-zero entries,
// so a step costs O(distinct tokens), not O(V): one workgroup per stream notes the token the step fed (one
// thread), and behind a barrier all threads walk the list.  Nothing leaves the workgroup's own rows.
#include <cmath>

#include "common.hpp"

namespace ti {

constexpr int kPenThreads = 1024;   // penalty_step_kernel: 16 waves walk the list
constexpr int kPenResetThreads = 256;
constexpr int kPenBatch = 4;        // list entries per thread whose loads are in flight together

__device__ __forceinline__ float pen_apply(float l, int count, float repetition, float presence, float frequency) {
  const float a = l <= 0.0f ? l * repetition : l / repetition;
  const float b = (float)count * frequency;
  const float d = b + presence;
  return a - d;
}

// One stream's step with its three values (the kernel arguments, or the row's table entry)
__device__ __forceinline__ void penalty_step_row(const ti_penalty_args& a, float repetition, float presence, float frequency) {
  __shared__ int s_n;
  const int m = blockIdx.x, tid = threadIdx.x;
  int t = 0;   // the row's draw index, as sample_kernel computes it
  if (a.step_ctr) t = (*a.step_ctr - a.advance) - (a.n_in ? a.n_in[m] - 1 : 0);
  if (t < 0 || t >= a.draw_stride) return;   // a prompt step or past the budget: nothing moves
  int32_t* counts = a.state.counts + (size_t)m * a.V;
  int32_t* seen = a.state.seen + (size_t)m * a.V;
  if (tid == 0) {
    int n = min(max(a.state.n_seen[m], 0), a.V);
    int tok = -1;   // the token this step fed, when it is a generated one
    if (t >= 1) {
      if (a.out_tokens && t - 1 < a.out_stride) tok = a.out_tokens[(size_t)m * a.out_stride + (t - 1)];
    } else if (a.carry) {
      tok = a.carry[m];
    }
    if (tok >= 0 && tok < a.V) {
      const int c = counts[tok];
      counts[tok] = c + 1;
      if (c <= 0 && n < a.V) seen[n++] = tok;
      a.state.n_seen[m] = n;
    }
    s_n = n;
  }
  __syncthreads();   // thread 0's count and list entry are visible to the walk
  const int n = s_n;
  float* lg = a.logits + (size_t)m * a.ldl;
  // Three dependent loads per entry (id, its count, its logit), each a likely HBM miss behind a step that streamed
  // the weights through the caches: kPenBatch entries per thread go through each stage together.
  for (int i0 = tid; i0 < n; i0 += kPenThreads * kPenBatch) {
    int v[kPenBatch], c[kPenBatch];
    float l[kPenBatch];
#pragma unroll
    for (int k = 0; k < kPenBatch; ++k) {
      const int i = i0 + k * kPenThreads;
      v[k] = i < n ? seen[i] : -1;
      if (v[k] < 0 || v[k] >= a.V) v[k] = -1;   // (past the list, or stale state of a slot nobody reset)
    }
#pragma unroll
    for (int k = 0; k < kPenBatch; ++k) c[k] = v[k] >= 0 ? counts[v[k]] : 0;
#pragma unroll
    for (int k = 0; k < kPenBatch; ++k) l[k] = c[k] > 0 ? lg[v[k]] : 0.0f;
#pragma unroll
    for (int k = 0; k < kPenBatch; ++k)
      if (c[k] > 0) lg[v[k]] = pen_apply(l[k], c[k], repetition, presence, frequency);
  }
}

__global__ __launch_bounds__(kPenThreads) void penalty_step_kernel(const ti_penalty_args a) {
  penalty_step_row(a, a.repetition, a.presence, a.frequency);
}

// finite: the exponent field is not all ones (a bit test, whatever the compiler assumes about NaNs)
__device__ __forceinline__ bool pen_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// ti_penalty_step_rows: the values are block-uniform loads from rows[m].  A row that does not penalise, or whose
// entry ti_penalty_step would have refused, leaves before anything is read or written.
__global__ __launch_bounds__(kPenThreads) void penalty_step_rows_kernel(const ti_penalty_args a, const ti_row_params* rows) {
  const ti_row_params rp = rows[blockIdx.x];
  const float rep = rp.repetition, pres = rp.presence, freq = rp.frequency;
  if (rep == 1.0f && pres == 0.0f && freq == 0.0f) return;
  if (!(pen_finite(rep) && rep > 0.0f) || !pen_finite(pres) || !pen_finite(freq)) return;
  penalty_step_row(a, rep, pres, freq);
}

// counts / seen rows of the slot are zero and n_seen[m] is 0 on entry (the launcher's memsets)
__global__ __launch_bounds__(kPenResetThreads) void penalty_reset_kernel(ti_penalty_state st, int V, int m,
                                                                    const int32_t* __restrict__ tokens, int n) {
  const int i = blockIdx.x * kPenResetThreads + threadIdx.x;
  if (i >= n) return;
  const int tok = tokens[i];
  if (tok < 0 || tok >= V) return;
  int32_t* counts = st.counts + (size_t)m * V;
  if (atomicAdd(&counts[tok], 1) == 0) {   // exactly one occurrence sees 0: at most V appends
    const int at = atomicAdd(&st.n_seen[m], 1);
    if (at < V) st.seen[(size_t)m * V + at] = tok;
  }
}

}  // namespace ti

extern "C" int ti_penalty_reset(const ti_penalty_state* st, int V, int m, const int32_t* tokens_dev, int n,
                                ti_stream_t stream) {
  if (!st || !st->counts || !st->seen || !st->n_seen || V < 1 || m < 0 || n < 0 || (!tokens_dev && n > 0))
    return ti_set_error(TI_ERR_ARG, "ti_penalty_reset: bad arguments (V %d, m %d, n %d)", V, m, n);
  hipStream_t s = (hipStream_t)stream;
  TI_HIP_CHECK(hipMemsetAsync(st->counts + (size_t)m * V, 0, (size_t)V * 4, s), "hipMemsetAsync(penalty counts)");
  TI_HIP_CHECK(hipMemsetAsync(st->seen + (size_t)m * V, 0, (size_t)V * 4, s), "hipMemsetAsync(penalty seen)");
  TI_HIP_CHECK(hipMemsetAsync(st->n_seen + m, 0, 4, s), "hipMemsetAsync(penalty n_seen)");
  if (n == 0) return TI_OK;
  const int blocks = (n + ti::kPenResetThreads - 1) / ti::kPenResetThreads;
  hipLaunchKernelGGL(ti::penalty_reset_kernel, dim3(blocks), dim3(ti::kPenResetThreads), 0, s, *st, V, m, tokens_dev, n);
  TI_LAUNCH_CHECK("penalty_reset_kernel");
  return TI_OK;
}

extern "C" int ti_penalty_step_rows(const ti_penalty_args* a, const ti_row_params* rows, ti_stream_t stream) {
  if (!a || !rows || !a->logits || !a->state.counts || !a->state.seen || !a->state.n_seen || (a->step_ctr && !a->out_tokens))
    return ti_set_error(TI_ERR_ARG, "ti_penalty_step_rows: null");
  if (a->M < 1 || a->V < 1 || a->ldl < a->V || a->draw_stride < 1 || a->out_stride < 0)
    return ti_set_error(TI_ERR_ARG, "ti_penalty_step_rows: M %d V %d ldl %d draw_stride %d out_stride %d", a->M, a->V,
                        a->ldl, a->draw_stride, a->out_stride);
  hipLaunchKernelGGL(ti::penalty_step_rows_kernel, dim3(a->M), dim3(ti::kPenThreads), 0, (hipStream_t)stream, *a, rows);
  TI_LAUNCH_CHECK("penalty_step_rows_kernel");
  ti_stamp_next(ti::STAMP_OTHER, 0);   // (unstamped; keeps the stamped step's launch list whole)
  return TI_OK;
}

extern "C" int ti_penalty_step(const ti_penalty_args* a, ti_stream_t stream) {
  if (!a || !a->logits || !a->state.counts || !a->state.seen || !a->state.n_seen || (a->step_ctr && !a->out_tokens))
    return ti_set_error(TI_ERR_ARG, "ti_penalty_step: null");
  if (a->M < 1 || a->V < 1 || a->ldl < a->V || a->draw_stride < 1 || a->out_stride < 0)
    return ti_set_error(TI_ERR_ARG, "ti_penalty_step: M %d V %d ldl %d draw_stride %d out_stride %d", a->M, a->V, a->ldl,
                        a->draw_stride, a->out_stride);
  if (!(std::isfinite(a->repetition) && a->repetition > 0.0f) || !std::isfinite(a->presence) || !std::isfinite(a->frequency))
    return ti_set_error(TI_ERR_ARG, "ti_penalty_step: repetition %g (finite, > 0), presence %g, frequency %g (finite)",
                        (double)a->repetition, (double)a->presence, (double)a->frequency);
  hipLaunchKernelGGL(ti::penalty_step_kernel, dim3(a->M), dim3(ti::kPenThreads), 0, (hipStream_t)stream, *a);
  TI_LAUNCH_CHECK("penalty_step_kernel");
  ti_stamp_next(ti::STAMP_OTHER, 0);   // (unstamped; keeps the stamped step's launch list whole)
  return TI_OK;
}
