// guide.hip -- token-automaton guided decoding: one launch between the lm_head (and ti_penalty_step) and the
// sampler that advances each stream's automaton state by the token the step fed and sets every logit the new
// state does not allow to -inf (ti_hip.h ti_guide_step; the contract is ti_engine.h ti_guide's).
//
// One workgroup per stream.  One thread binary-searches the fed token in the state's sorted token list and
// publishes the new state through LDS; behind the barrier all threads stream the row once.  The allow-bitmask of
// the state (built on the host, ceil(V / 32) words) says what to do with each group of four columns without
// reading the row: all allowed -- nothing is touched; none allowed -- one 16-byte store of -inf; mixed -- load,
// select, store.  A constrained state allows few ids, so most of the row is written and never read.  The vector
// part starts at the row's first 16-byte aligned column and ends at the last whole group below V; the columns
// before and behind go one by one.  Nothing leaves the workgroup's own row and state word.
//
// ti_guide_step_rows is the same body with each row's guide its own: the row's handle (ti_row_params.reserved[0])
// picks a descriptor out of a device table, so a captured launch bakes in two pointers and never a guide.
#include "common.hpp"

namespace ti {

constexpr int kGuideThreads = 1024;
constexpr unsigned kGuideNegInf = 0xFF800000u;

// next state of `tok` in state s, or -1
__device__ __forceinline__ int guide_next(const ti_guide_dev& g, int s, int tok) {
  int64_t lo = g.row_ptr[s], hi = g.row_ptr[s + 1];
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int v = g.tokens[mid];
    if (v == tok) return g.next[mid];
    if (v < tok) lo = mid + 1;
    else hi = mid;
  }
  return -1;
}

// One row's step under descriptor g (a.guide is not read): the body of both kernels below.
__device__ __forceinline__ void guide_step_row(const ti_guide_args& a, const ti_guide_dev& g) {
  __shared__ int s_state;
  const int m = blockIdx.x, tid = threadIdx.x;
  int t = 0;   // the row's draw index, as sample_kernel computes it
  if (a.step_ctr) t = (*a.step_ctr - a.advance) - (a.n_in ? a.n_in[m] - 1 : 0);
  if (t < 0 || t >= a.draw_stride) return;   // a prompt step or past the budget: nothing moves
  if (tid == 0) {
    int s = a.state[m];
    if (s >= g.n_states) s = -1;   // (stale state of a slot nobody reset, or one of another row's larger guide)
    int tok = -1;   // the token this step fed, when it is a generated one
    if (t >= 1) {
      if (a.out_tokens && t - 1 < a.out_stride) tok = a.out_tokens[(size_t)m * a.out_stride + (t - 1)];
    } else if (a.carry) {
      tok = a.carry[m];
    }
    if (s >= 0 && tok >= 0) {
      s = guide_next(g, s, tok);
      if (s >= g.n_states) s = -1;
      a.state[m] = s;
    }
    s_state = s;
  }
  __syncthreads();   // thread 0's new state is visible to the walk
  const int s = s_state;
  if (s < 0) return;   // free or dead: the row keeps its bits
  const int V = a.V, W = g.mask_words;
  const uint32_t* __restrict__ mw = g.mask + (size_t)s * W;
  float* lg = a.logits + (size_t)m * a.ldl;
  const float ninf = __uint_as_float(kGuideNegInf);
  auto one = [&](int v) {
    if (!((mw[v >> 5] >> (v & 31)) & 1u)) lg[v] = ninf;
  };
  // columns [0, head) before the first 16-byte aligned one, groups of four in [head, vend), then [vend, V)
  const int head = min(V, (int)((4u - (unsigned)(((uintptr_t)lg >> 2) & 3u)) & 3u));
  const int vend = head + ((V - head) & ~3);
  if (tid < head) one(tid);
  for (int v = head + tid * 4; v < vend; v += kGuideThreads * 4) {
    // the four columns' bits: they may straddle two mask words when head is not 0
    const int w0 = v >> 5, w1 = min((v + 3) >> 5, W - 1);
    const unsigned long long ww = (unsigned long long)mw[w0] | ((unsigned long long)mw[w1] << 32);
    const unsigned bits = (unsigned)(ww >> (v & 31)) & 0xFu;
    if (bits == 0xFu) continue;
    float4* p = reinterpret_cast<float4*>(lg + v);
    float4 x = make_float4(ninf, ninf, ninf, ninf);
    if (bits != 0u) {
      const float4 old = *p;
      if (bits & 1u) x.x = old.x;
      if (bits & 2u) x.y = old.y;
      if (bits & 4u) x.z = old.z;
      if (bits & 8u) x.w = old.w;
    }
    *p = x;
  }
  if (vend + tid < V) one(vend + tid);
}

__global__ __launch_bounds__(kGuideThreads) void guide_step_kernel(const ti_guide_args a) { guide_step_row(a, a.guide); }

// ti_guide_step_rows: row m's descriptor is guides[rows[m].reserved[0] - 1], the handle and the descriptor both
// block-uniform loads.  The table is memory the launch cannot check: a handle outside [1, guide_cap], or an entry
// that is unused (all zero), has a null pointer, n_states < 1 or mask_words != ceil(V / 32), returns before the
// row's state or logits are touched.
__global__ __launch_bounds__(kGuideThreads) void guide_step_rows_kernel(const ti_guide_args a, const ti_guide_dev* guides,
                                                                        int guide_cap, const ti_row_params* rows) {
  const int h = rows[blockIdx.x].reserved[0];
  if (h < 1 || h > guide_cap) return;
  const ti_guide_dev g = guides[h - 1];
  if (g.n_states < 1 || g.mask_words != (a.V + 31) / 32 || !g.row_ptr || !g.tokens || !g.next || !g.mask) return;
  guide_step_row(a, g);
}

}  // namespace ti

extern "C" int ti_guide_reset(int32_t* state, int first, int count, int32_t value, ti_stream_t stream) {
  if (!state || first < 0 || count < 1 || value < -1)
    return ti_set_error(TI_ERR_ARG, "ti_guide_reset: bad arguments (first %d, count %d, value %d)", first, count, (int)value);
  TI_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(state + first), value, (size_t)count, (hipStream_t)stream),
               "hipMemsetD32Async(guide state)");
  return TI_OK;
}

extern "C" int ti_guide_step(const ti_guide_args* a, ti_stream_t stream) {
  if (!a || !a->logits || !a->state || !a->guide.row_ptr || !a->guide.tokens || !a->guide.next || !a->guide.mask ||
      (a->step_ctr && !a->out_tokens))
    return ti_set_error(TI_ERR_ARG, "ti_guide_step: null");
  if (a->M < 1 || a->V < 1 || a->ldl < a->V || a->draw_stride < 1 || a->out_stride < 0)
    return ti_set_error(TI_ERR_ARG, "ti_guide_step: M %d V %d ldl %d draw_stride %d out_stride %d", a->M, a->V, a->ldl,
                        a->draw_stride, a->out_stride);
  if (a->guide.n_states < 1 || a->guide.mask_words != (a->V + 31) / 32)
    return ti_set_error(TI_ERR_ARG, "ti_guide_step: n_states %d, mask_words %d for V %d (ceil(V / 32) = %d)",
                        a->guide.n_states, a->guide.mask_words, a->V, (a->V + 31) / 32);
  hipLaunchKernelGGL(ti::guide_step_kernel, dim3(a->M), dim3(ti::kGuideThreads), 0, (hipStream_t)stream, *a);
  TI_LAUNCH_CHECK("guide_step_kernel");
  ti_stamp_next(ti::STAMP_OTHER, 0);   // (unstamped; keeps the stamped step's launch list whole)
  return TI_OK;
}

extern "C" int ti_guide_step_rows(const ti_guide_args* a, const ti_guide_dev* guides, int guide_cap, const ti_row_params* rows,
                                  ti_stream_t stream) {
  if (!a || !guides || !rows || !a->logits || !a->state || (a->step_ctr && !a->out_tokens))
    return ti_set_error(TI_ERR_ARG, "ti_guide_step_rows: null");
  if (a->M < 1 || a->V < 1 || a->ldl < a->V || a->draw_stride < 1 || a->out_stride < 0 || guide_cap < 1)
    return ti_set_error(TI_ERR_ARG, "ti_guide_step_rows: M %d V %d ldl %d draw_stride %d out_stride %d guide_cap %d", a->M, a->V,
                        a->ldl, a->draw_stride, a->out_stride, guide_cap);
  hipLaunchKernelGGL(ti::guide_step_rows_kernel, dim3(a->M), dim3(ti::kGuideThreads), 0, (hipStream_t)stream, *a, guides,
                     guide_cap, rows);
  TI_LAUNCH_CHECK("guide_step_rows_kernel");
  ti_stamp_next(ti::STAMP_OTHER, 0);   // (unstamped, as ti_guide_step)
  return TI_OK;
}
