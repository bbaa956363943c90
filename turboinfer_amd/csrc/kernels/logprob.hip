// logprob.hip -- row log-softmax gather: [rows][vocab] fp32 logits -> one log-probability (and the
// greedy token) per row.
//
// InferenceEngine::compute_logprobs (src/model/inference_engine.cpp:921-942) per position:
//   max_r = max_v logits[r][v];  sum_r = sum_v exp(logits[r][v] - max_r)
//   logprob[r] = logits[r][target] - max_r - log(sum_r)
// The reference walks each row three times (max, sum, pick).  Here one workgroup walks its row
// once: every lane keeps a running (max, index of the max, sum rescaled to that max) over the
// elements it loads, and the lanes' triples are merged across the wave on the VALU (DPP /
// v_permlane swaps, common.hpp) and across the waves through LDS.  The merge is symmetric in
// its two inputs, bit for bit (fp add and max commute; the file compiles with -ffp-contract=off,
// so no operand is folded into an fma on one side only), so after each butterfly stage both
// partners hold the same triple -- what the mirrored DPP stages of common.hpp's group_sum need.
// Rows are read with 16-byte loads from the first 16-byte boundary on; the up to 3 elements
// before it and the up to 3 after the last whole vector are scalar loads, so any vocab >= 1 at
// any ld >= vocab works.  Differences to the reference: exp / log are the device's, and the sum
// is a tree over the lanes, not index order.
#include <math.h>

#include "common.hpp"

namespace ti {

constexpr int kLpThreads = 1024;
constexpr int kLpWaves = kLpThreads / kWave;
constexpr float kLpInvalidToken = -20.0f;   // the reference's LOGPROB_INVALID_TOKEN (:888)

// running softmax state: m = max so far, i = lowest index holding m, s = sum exp(x - m)
struct LpState {
  float m, s;
  int32_t i;
};

// exp(a - b) for a <= b, with a == b (both -inf: an empty lane) -> 1 instead of exp(nan)
__device__ __forceinline__ float lp_scale(float a, float b) { return a == b ? 1.0f : expf(a - b); }

__device__ __forceinline__ LpState lp_merge(const LpState a, const LpState b) {
  LpState r;
  r.m = fmaxf(a.m, b.m);
  r.s = a.s * lp_scale(a.m, r.m) + b.s * lp_scale(b.m, r.m);
  r.i = (b.m > a.m || (b.m == a.m && b.i < a.i)) ? b.i : a.i;
  return r;
}

// one element, indices ascending within a lane (a later equal value keeps the earlier index)
__device__ __forceinline__ void lp_push(LpState& st, float x, int32_t idx) {
  if (x > st.m) {
    st.s = st.s * expf(st.m - x) + 1.0f;   // (st.m = -inf: s = 0 * 0 + 1)
    st.m = x;
    st.i = idx;
  } else {
    st.s += lp_scale(x, st.m);
  }
}

// four consecutive elements: one rescale to their maximum, then four terms
__device__ __forceinline__ void lp_push4(LpState& st, const f32x4 v, int32_t idx) {
  float mx = v[0];
  int32_t mi = idx;
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (v[j] > mx) {
      mx = v[j];
      mi = idx + j;
    }
  if (mx > st.m) {
    st.s *= expf(st.m - mx);
    st.m = mx;
    st.i = mi;
  }
  st.s += (lp_scale(v[0], st.m) + lp_scale(v[1], st.m)) + (lp_scale(v[2], st.m) + lp_scale(v[3], st.m));
}

template <int CTRL>
__device__ __forceinline__ LpState lp_dpp(const LpState a) {
  return {dpp_f<CTRL>(a.m), dpp_f<CTRL>(a.s), __builtin_bit_cast(int32_t, dpp_f<CTRL>(__builtin_bit_cast(float, a.i)))};
}
template <int O>
__device__ __forceinline__ LpState lp_xor(const LpState a) {
  return {lane_xor<O>(a.m), lane_xor<O>(a.s), (int32_t)lane_xor_u32<O>((uint32_t)a.i)};
}

// all-reduce over the wave's 64 lanes (the stage order of group_sum<64>)
__device__ __forceinline__ LpState lp_wave_merge(LpState a) {
  a = lp_merge(a, lp_xor<1>(a));
  a = lp_merge(a, lp_xor<2>(a));
  a = lp_merge(a, lp_dpp<0x141>(a));   // row_half_mirror
  a = lp_merge(a, lp_dpp<0x140>(a));   // row_mirror
  a = lp_merge(a, lp_xor<16>(a));
  a = lp_merge(a, lp_xor<32>(a));
  return a;
}

__global__ __launch_bounds__(kLpThreads) void logprob_rows_kernel(const float* __restrict__ logits, int64_t ld,
                                                                  int vocab, const int32_t* __restrict__ targets,
                                                                  float* __restrict__ out_logprob,
                                                                  int32_t* __restrict__ out_top1) {
  __shared__ float s_m[kLpWaves], s_s[kLpWaves];
  __shared__ int32_t s_i[kLpWaves];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* row = logits + (size_t)r * ld;
  // elements before the first 16-byte boundary (the row base is 4-byte aligned), whole vectors, rest
  const int head = min(vocab, (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 2));
  const int nvec = (vocab - head) >> 2;
  const int tail0 = head + 4 * nvec;
  LpState st{-INFINITY, 0.0f, INT32_MAX};
  if (tid < head) lp_push(st, row[tid], tid);
  const f32x4* rv = reinterpret_cast<const f32x4*>(row + head);
  int j = tid;
  for (; j + kLpThreads < nvec; j += 2 * kLpThreads) {   // two loads in flight
    const f32x4 a = rv[j], b = rv[j + kLpThreads];
    lp_push4(st, a, head + 4 * j);
    lp_push4(st, b, head + 4 * (j + kLpThreads));
  }
  if (j < nvec) lp_push4(st, rv[j], head + 4 * j);
  if (tail0 + tid < vocab) lp_push(st, row[tail0 + tid], tail0 + tid);

  st = lp_wave_merge(st);
  const int lane = tid & 63, w = tid >> 6;
  if (lane == 0) {
    s_m[w] = st.m;
    s_s[w] = st.s;
    s_i[w] = st.i;
  }
  __syncthreads();
  if (w == 0) {
    LpState t{-INFINITY, 0.0f, INT32_MAX};
    if (lane < kLpWaves) t = {s_m[lane], s_s[lane], s_i[lane]};
    t = lp_wave_merge(t);
    if (lane == 0) {
      const int32_t tg = targets[r];
      float lp = 0.0f;                                   // -1: no target
      if (tg >= vocab || tg < -1) lp = kLpInvalidToken;
      else if (tg >= 0) lp = row[tg] - t.m - logf(t.s);
      out_logprob[r] = lp;
      if (out_top1) out_top1[r] = t.i;
    }
  }
}

}  // namespace ti

extern "C" int ti_logprob_rows(const float* logits, int ld, int rows, int vocab, const int32_t* targets,
                               float* out_logprob, int32_t* out_top1, ti_stream_t s) {
  if (!logits || !targets || !out_logprob || rows < 1 || vocab < 1 || ld < vocab)
    return ti_set_error(TI_ERR_ARG, "ti_logprob_rows: bad arguments rows=%d vocab=%d ld=%d", rows, vocab, ld);
  hipLaunchKernelGGL(ti::logprob_rows_kernel, dim3(rows), dim3(ti::kLpThreads), 0, (hipStream_t)s, logits, (int64_t)ld,
                     vocab, targets, out_logprob, out_top1);
  TI_LAUNCH_CHECK("logprob_rows_kernel");
  return TI_OK;
}
