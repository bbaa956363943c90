// lookahead.hip -- the device bookkeeping of lookahead greedy decoding (ti_hip.h): the n-gram draft lookup at
// the head of a verify step (ti_lookahead_begin, in ti_step_begin's place) and the accept / commit at its end
// (ti_lookahead_accept, after the lm_head).  With both on the device the replayed verify graph never returns
// to the host between steps.
#include <math.h>

#include "common.hpp"

namespace ti {

constexpr int kLaThreads = 1024;

// One workgroup per row j.  Every workgroup runs the same lookup over the history (it is read from L2 after
// the first), so no workgroup waits for another; workgroup 0 records nd.
//
// The draft rule as one reduction: for a candidate end e = i + g in [1, L - 1], let c(e) be the length of the
// common suffix of hist[0 .. e) and hist[0 .. L), capped at min(ngram, L - 1, e).  A match of length g ends at
// e exactly when c(e) >= g, so the longest g with any match is max c, and its largest i = e - g is the largest
// e with c(e) = max c: the maximum of the key (c(e) << 32 | e) over the candidates with c(e) >= 1.
__global__ __launch_bounds__(kLaThreads) void lookahead_begin_kernel(const ti_lookahead_args a) {
  __shared__ unsigned long long s_key[kLaThreads / 64];
  const int j = blockIdx.x, tid = threadIdx.x;
  const int cap = a.cfg[LA_CFG_CAP];
  const int L = min(max(a.state[LA_LEN], 1), cap), done = a.state[LA_DONE];
  const int keff = done ? 0 : min(a.k, a.cfg[LA_CFG_MAX_NEW] - a.state[LA_PRODUCED] - 1);
  unsigned long long key = 0ull;
  if (keff >= 1) {   // block-uniform
    const int gmax = min(min(a.cfg[LA_CFG_NGRAM], TI_LA_MAX_NGRAM), L - 1);
    for (int e = 1 + tid; e <= L - 1; e += kLaThreads) {
      const int lim = min(gmax, e);
      int c = 0;
      while (c < lim && a.hist[e - 1 - c] == a.hist[L - 1 - c]) ++c;
      if (c >= 1) key = max(key, ((unsigned long long)c << 32) | (unsigned)e);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(key, o, 64);
      key = other > key ? other : key;
    }
    if ((tid & 63) == 0) s_key[tid >> 6] = key;
    __syncthreads();
    key = 0ull;
#pragma unroll
    for (int w = 0; w < kLaThreads / 64; ++w) key = s_key[w] > key ? s_key[w] : key;
  }
  const int e = (int)(key & 0xFFFFFFFFull);            // first draft's index (0: no match)
  const int nd = key ? min(keff, L - e) : 0;
  int tok = j >= 1 && j <= nd ? a.hist[e + j - 1] : a.hist[L - 1];
  if (tok < 0 || tok >= a.vocab) tok = 0;              // never index outside the table
  if (tid == 0) {
    a.row_tok[j] = tok;
    a.pos[j] = min(a.state[LA_POS] + j, a.max_pos);
    if (j == 0 && !done) a.state[LA_ND] = nd;
  }
  if (tid < TI_ARGMAX_SLOTS) a.argmax[(size_t)j * TI_ARGMAX_SLOTS + tid] = 0ull;
  const uint16_t* er = a.emb + (size_t)tok * a.hidden;
  float* h = a.h + (size_t)j * a.hidden;
  if ((a.hidden & 7) == 0) {   // 16-byte pieces
    for (int i8 = tid; i8 < (a.hidden >> 3); i8 += kLaThreads) {
      const f16x8 v = *(const f16x8*)(er + 8 * i8);
      *(float4*)(h + 8 * i8) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
      *(float4*)(h + 8 * i8 + 4) = make_float4((float)v[4], (float)v[5], (float)v[6], (float)v[7]);
    }
  } else {
    for (int i = tid; i < a.hidden; i += kLaThreads) h[i] = h2f(er[i]);
  }
}

// One workgroup of 16 rows x 32 slots: lane group (row) folds its slots into the row's key, thread 0 commits.
__global__ __launch_bounds__(16 * TI_ARGMAX_SLOTS) void lookahead_accept_kernel(const ti_lookahead_args a) {
  static_assert(TI_ARGMAX_SLOTS == 32 && TI_LA_MAX_K + 1 == 16, "one half-wave per row");
  __shared__ int s_tok[TI_LA_MAX_K + 1];
  const int tid = threadIdx.x, row = tid >> 5, slot = tid & 31;
  if (a.state[LA_DONE]) return;   // block-uniform
  unsigned long long key = row <= a.k ? a.argmax[(size_t)row * TI_ARGMAX_SLOTS + slot] : 0ull;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if (slot == 0) s_tok[row] = (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
  __syncthreads();
  if (tid != 0) return;
  const int max_new = a.cfg[LA_CFG_MAX_NEW], stop = a.cfg[LA_CFG_STOP], cap = a.cfg[LA_CFG_CAP];
  const int L = a.state[LA_LEN], produced = a.state[LA_PRODUCED], nd = min(max(a.state[LA_ND], 0), a.k);
  int acc = 0;
  while (acc < nd && a.row_tok[acc + 1] == s_tok[acc]) ++acc;
  int n = 0, done = 0;
  while (n <= acc && produced + n < max_new && L + n < cap) {
    const int tok = s_tok[n];
    a.hist[L + n] = tok;
    a.out_tokens[produced + n] = tok;
    ++n;
    if (stop >= 0 && tok == stop) {
      done = 1;
      break;
    }
  }
  if (produced + n >= max_new || L + n >= cap) done = 1;
  a.state[LA_LEN] = L + n;
  a.state[LA_POS] += n;
  a.state[LA_PRODUCED] = produced + n;
  a.state[LA_DONE] = done;
  a.state[LA_STEPS] += 1;
  a.state[LA_DRAFTED] += nd;
  a.state[LA_ACCEPTED] += min(n, acc);
}

static int la_check(const char* name, const ti_lookahead_args* a) {
  if (!a || !a->state || !a->cfg || !a->hist || !a->emb || !a->h || !a->row_tok || !a->pos || !a->argmax || !a->out_tokens)
    return ti_set_error(TI_ERR_ARG, "%s: null pointer", name);
  if (a->k < 1 || a->k > TI_LA_MAX_K) return ti_set_error(TI_ERR_ARG, "%s: k %d outside [1, %d]", name, a->k, TI_LA_MAX_K);
  if (a->hidden < 1 || a->vocab < 1 || a->max_pos < 0)
    return ti_set_error(TI_ERR_ARG, "%s: hidden %d vocab %d max_pos %d", name, a->hidden, a->vocab, a->max_pos);
  return TI_OK;
}

}  // namespace ti

extern "C" int ti_lookahead_begin(const ti_lookahead_args* a, ti_stream_t stream) {
  if (const int rc = ti::la_check("ti_lookahead_begin", a)) return rc;
  hipLaunchKernelGGL(ti::lookahead_begin_kernel, dim3(a->k + 1), dim3(ti::kLaThreads), 0, (hipStream_t)stream, *a);
  TI_LAUNCH_CHECK("lookahead_begin_kernel");
  return TI_OK;
}

extern "C" int ti_lookahead_accept(const ti_lookahead_args* a, ti_stream_t stream) {
  if (const int rc = ti::la_check("ti_lookahead_accept", a)) return rc;
  hipLaunchKernelGGL(ti::lookahead_accept_kernel, dim3(1), dim3(16 * TI_ARGMAX_SLOTS), 0, (hipStream_t)stream, *a);
  TI_LAUNCH_CHECK("lookahead_accept_kernel");
  return TI_OK;
}
