// shared_attn.hip -- batched decode attention over a prompt prefix the streams share (ti_attn_decode_shared).
//
// Stream m attends keys [0, P) of STREAM 0's cache and keys [P, pos[m]] of its own.  When every stream's rows
// [0, P) hold stream 0's values this is ti_attn_decode's function, with the prefix read once per block of 16
// (stream, q-head) columns instead of once per stream.  Two dependent launches; the launch boundary is the only
// synchronisation (no tickets, no spin loops, nothing in the workspace to zero):
//
//  1. attn_shared_prefix_kernel: the per-wave prefill kernel's arithmetic (prefill_attn.hip: S^T = K Q^T and
//     O^T += V^T P^T on fp16 MFMA, the fp32 operands q and p as fp16 hi + lo, online softmax per column, a
//     register ring of K / V blocks through buffer loads).  The (stream, q-head) columns of a kv-head go in
//     blocks of 16 (column c of block b: stream (16 b + c) / G, q-head (16 b + c) % G of the group); the prefix's
//     key blocks are cut over gridDim.z waves per (column block, kv-head), split s taking blocks
//     [s n / S, (s + 1) n / S) of the n = ceil(P / 16): the last split is never empty.  Every column's limit is
//     P - 1, so only a step that reaches past the split's last key masks.  Each wave writes its unnormalised
//     accumulators and (m, l) per column; a split without blocks writes (-inf, 0, zeros).
//     Workspace, per (column block, kv-head, split): kShPart<HD> floats -- o [16 columns][HD], m [16], l [16].
//  2. attn_shared_own_kernel: per (stream, kv-head) the stream's own keys [P, pos[m]] with the decode kernel's
//     arithmetic (attention_body.hpp: hd / 8 lanes per key row, fp32 FMA, online softmax per lane group, lane
//     groups then waves merged), then the prefix splits merged in split order 0 .. S - 1 and the own part last,
//     normalised and stored fp16, row-major or TI_X_F16_PACKED.  The fixed order makes the result
//     bit-reproducible from run to run.
// K and V are read-only to both launches; rows [0, P) of streams >= 1 and rows past pos[m] are never read.
#include <math.h>

#include <algorithm>

#include "common.hpp"

namespace ti {

typedef uint32_t sh_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t sh_u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 sh_f16x4 __attribute__((ext_vector_type(4)));

template <int HD>
constexpr int kShPart = 16 * HD + 32;
constexpr int kShRing = 4;       // K / V blocks in flight per wave (one wave per SIMD: the deep ring of the prefill kernel)
constexpr int kShOwnWaves = 4;   // waves of an own-keys workgroup

__device__ __forceinline__ void sh_split(float x, _Float16& hi, _Float16& lo) {
  hi = (_Float16)x;
  lo = (_Float16)(x - (float)hi);
}

template <int HD>
__global__ __launch_bounds__(64, 1) void attn_shared_prefix_kernel(const float* __restrict__ q, const uint16_t* __restrict__ kc,
                                                               const uint16_t* __restrict__ vc, int max_seq, int M, int heads,
                                                               int gsh, int P, float scale, float* __restrict__ ws) {
  constexpr int DV = HD / 16, KW = HD / 32, RING = kShRing, NB = 2;
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int G = 1 << gsh, qpw = 16 >> gsh;
  const int blk = blockIdx.x, kvh = blockIdx.y, sp = blockIdx.z, S = gridDim.z;
  // (columns past the last stream repeat it: computed, stored into the block's own partial, never merged)
  const int qi = min(blk * qpw + (r >> gsh), M - 1), h = kvh * G + (r & (G - 1));
  // B operand of step c: dims 32c + 8g + e of this lane's column, fp16 hi + lo
  f16x8 qh[KW], ql[KW];
  {
    const float* qr = q + ((size_t)qi * heads + h) * HD + 8 * g;
#pragma unroll
    for (int c = 0; c < KW; ++c) {
      const float4 t0 = *(const float4*)(qr + 32 * c), t1 = *(const float4*)(qr + 32 * c + 4);
      const float v[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        _Float16 hi, lo;
        sh_split(v[e] * scale, hi, lo);
        qh[c][e] = hi;
        ql[c][e] = lo;
      }
    }
  }
  // stream 0's cache of this kv-head; rows past P - 1 may be unwritten: they read row P - 1 instead, finite,
  // which their p = 0 multiplies away exactly
  const auto krs = buffer_rsrc(kc + (size_t)kvh * max_seq * HD), vrs = buffer_rsrc(vc + (size_t)kvh * max_seq * HD);
  const int kl = P - 1;
  auto load = [&](int kb, sh_u32x4 (&k)[KW], sh_u32x4 (&v)[4]) {
    const int kk = min(kb * 16 + r, kl);
#pragma unroll
    for (int c = 0; c < KW; ++c)
      k[c] = __builtin_bit_cast(sh_u32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, (kk * HD + 8 * g + 32 * c) * 2, 0, 0));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int off = (min(kb * 16 + 4 * g + j, kl) * HD + r * DV) * 2;
      if constexpr (HD == 128) {
        v[j] = __builtin_bit_cast(sh_u32x4, __builtin_amdgcn_raw_buffer_load_b128(vrs, off, 0, 0));
      } else {
        const sh_u32x2 t = __builtin_bit_cast(sh_u32x2, __builtin_amdgcn_raw_buffer_load_b64(vrs, off, 0, 0));
        v[j] = (sh_u32x4){t[0], t[1], 0u, 0u};
      }
    }
  };
  f32x4 acc[DV];
#pragma unroll
  for (int t = 0; t < DV; ++t) acc[t] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
  float m_run = -INFINITY, l_run = 0.0f;
  const int nkb = (P - 1) / 16 + 1;
  const int b0 = __builtin_amdgcn_readfirstlane((int)((long)sp * nkb / S));
  const int b1 = __builtin_amdgcn_readfirstlane((int)((long)(sp + 1) * nkb / S));
  const int pe = min(P - 1, b1 * 16 - 1);   // the last key this split counts
  sh_u32x4 kr[RING][KW], vr[RING][4];
#pragma unroll
  for (int u = 0; u < RING; ++u) load(b0 + u, kr[u], vr[u]);
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the loop's own count sets its waits (prefill_attn.hip)
  constexpr float kSlack = 8.0f;        // O rescaled only when a column max moves by more than e^8
  for (int kb0 = b0; kb0 < b1; kb0 += RING) {
#pragma unroll
    for (int u = 0; u < RING; u += NB) {
      const int kb = kb0 + u;
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int c = 0; c < KW; ++c) asm volatile("" : "+v"(kr[u + b][c]));   // no S of a later step hoisted above
      f32x4 s[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) s[b] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int c = 0; c < KW; ++c)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const f16x8 kf = __builtin_bit_cast(f16x8, kr[u + b][c]);
          s[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qh[c], s[b], 0, 0, 0);
          s[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, ql[c], s[b], 0, 0, 0);
        }
      float pv[NB][4], bm = -INFINITY;
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) pv[b][i] = s[b][i];
      if ((kb + NB) * 16 - 1 > pe) {   // wave-uniform: the step reaches past the split's last key
        const int lim = pe - kb * 16 - 4 * g;
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (16 * b + i > lim) pv[b][i] = -INFINITY;
      }
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) bm = fmaxf(bm, pv[b][i]);
      bm = xor32_max(xor16_max(bm));
      const float mn = fmaxf(m_run, bm);
      if (__builtin_amdgcn_ballot_w64(mn > m_run + kSlack) != 0) {
        const float alpha = m_run == mn ? 1.0f : __expf(m_run - mn);
        l_run *= alpha;
        m_run = mn;
#pragma unroll
        for (int t = 0; t < DV; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[t][i] *= alpha;
      }
      float ps = 0.0f;
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          // (a pass's steps past b1 hold masked keys only; the first step of a split always has a key)
          pv[b][i] = m_run == -INFINITY ? 0.0f : __expf(pv[b][i] - m_run);
          ps += pv[b][i];
        }
      l_run += ps;
      asm volatile("" : "+v"(l_run));
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        sh_f16x4 ph, pl;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          _Float16 hi, lo;
          sh_split(pv[b][e], hi, lo);
          ph[e] = hi;
          pl[e] = lo;
        }
#pragma unroll
        for (int t = 0; t < DV; ++t) {
          const uint32_t sel = (t & 1) ? 0x07060302u : 0x05040100u;
          const uint32_t b01 = __builtin_amdgcn_perm(vr[u + b][1][t >> 1], vr[u + b][0][t >> 1], sel);
          const uint32_t b23 = __builtin_amdgcn_perm(vr[u + b][3][t >> 1], vr[u + b][2][t >> 1], sel);
          const sh_f16x4 bf = __builtin_bit_cast(sh_f16x4, ((unsigned long long)b23 << 32) | b01);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x16f16(bf, ph, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x16f16(bf, pl, acc[t], 0, 0, 0);
        }
        load(kb + b + RING, kr[u + b], vr[u + b]);   // unconditional refill (clamped rows past the prefix)
      }
    }
  }
  float lt = l_run + __shfl_xor(l_run, 16, 64);
  lt += __shfl_xor(lt, 32, 64);
  // lane (r, g) holds dims DV (4g + i) + t of column r in acc[t][i]: 4 DV contiguous floats of the column's row
  float* part = ws + ((size_t)(blk * gridDim.y + kvh) * S + sp) * kShPart<HD>;
  float* dst = part + r * HD + 4 * g * DV;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < DV; t += 4)
      *(f32x4*)(dst + i * DV + t) = (f32x4){acc[t][i], acc[t + 1][i], acc[t + 2][i], acc[t + 3][i]};
  if (g == 0) {
    part[16 * HD + r] = m_run;
    part[16 * HD + 16 + r] = lt;
  }
}

// the 8 fp16 of one 16-byte load as floats
__device__ __forceinline__ void sh_unpack8(const sh_u32x4 v, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t w = v[i];   // (copied out first: a bit_cast of a vector element expression reads element 0)
    const f16x2 h = __builtin_bit_cast(f16x2, w);
    f[2 * i] = (float)h[0];
    f[2 * i + 1] = (float)h[1];
  }
}

template <int O>
__device__ __forceinline__ float sh_groups_max(float v) {
  if constexpr (O < 64) return sh_groups_max<2 * O>(fmaxf(v, lane_xor<O>(v)));
  else return v;
}
template <int O>
__device__ __forceinline__ float sh_groups_sum(float v) {
  if constexpr (O < 64) return sh_groups_sum<2 * O>(v + lane_xor<O>(v));
  else return v;
}

template <int HD, int G>
__global__ __launch_bounds__(kShOwnWaves * 64) void attn_shared_own_kernel(const float* __restrict__ q, const uint16_t* __restrict__ kc,
                                                                     const uint16_t* __restrict__ vc, int64_t stride, int max_seq,
                                                                     const int32_t* __restrict__ pos, int heads, int P, int S,
                                                                     float scale, const float* __restrict__ ws, int out_kt,
                                                                     uint16_t* __restrict__ out) {
  constexpr int NW = kShOwnWaves, R = 2, LPK = HD / 8, KPW = 64 / LPK;
  __shared__ float s_m[NW][G], s_l[NW][G];
  __shared__ __attribute__((aligned(16))) float s_acc[NW][G][HD];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dl = lane % LPK, kg = lane / LPK;
  const int kvh = blockIdx.x, m = blockIdx.y, kv_heads = gridDim.x;
  // own keys [P, s1): none for a row at or below P - 1 (it attends the prefix only)
  const int s0 = P, s1 = min(max(pos[m] + 1, P), max_seq);
  const int nslot = (s1 - s0 + KPW - 1) / KPW;
  const int total = wave < nslot ? (nslot - wave + NW - 1) / NW : 0;   // this wave's slots
  const uint16_t* kb = kc + (int64_t)m * stride + (int64_t)kvh * max_seq * HD;
  const uint16_t* vb = vc + (int64_t)m * stride + (int64_t)kvh * max_seq * HD;
  float qs[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float* qr = q + ((size_t)m * heads + kvh * G + g) * HD + dl * 8;
    const float4 q0 = *(const float4*)qr, q1 = *(const float4*)(qr + 4);
    qs[g][0] = q0.x * scale; qs[g][1] = q0.y * scale; qs[g][2] = q0.z * scale; qs[g][3] = q0.w * scale;
    qs[g][4] = q1.x * scale; qs[g][5] = q1.y * scale; qs[g][6] = q1.z * scale; qs[g][7] = q1.w * scale;
  }
  float mrun[G], lrun[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    mrun[g] = -INFINITY;
    lrun[g] = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.0f;
  }
  if (total > 0) {   // wave-uniform
    auto slot_key = [&](int i) { return s0 + (wave + NW * i) * KPW + kg; };
    sh_u32x4 kr[R], vr[R];
    int rj = 0, ci = 0;
    auto refill = [&](int s) {   // past the wave's last slot, and past s1 - 1: a row that is read anyway
      const int key = min(slot_key(min(rj, total - 1)), s1 - 1);
      ++rj;
      kr[s] = __builtin_nontemporal_load((const sh_u32x4*)(kb + (int64_t)key * HD + dl * 8));
      vr[s] = __builtin_nontemporal_load((const sh_u32x4*)(vb + (int64_t)key * HD + dl * 8));
    };
    auto consume = [&](const sh_u32x4& kv, const sh_u32x4& vv) {
      const bool valid = slot_key(ci) < s1;
      ++ci;
      float kf[8], vf[8];
      sh_unpack8(kv, kf);
      sh_unpack8(vv, vf);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float d = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d = fmaf(qs[g][e], kf[e], d);
        d = group_sum<LPK>(d);
        const float sc = valid ? d : -INFINITY;
        const float mn = fmaxf(mrun[g], sc);
        const float alpha = mrun[g] == mn ? 1.0f : __expf(mrun[g] - mn);
        const float p = valid ? __expf(sc - mn) : 0.0f;
        lrun[g] = fmaf(lrun[g], alpha, p);
        mrun[g] = mn;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] = fmaf(p, vf[e], acc[g][e] * alpha);
      }
    };
#pragma unroll
    for (int s = 0; s < R; ++s) refill(s);
    int j0 = 0;
    for (; j0 + R <= total; j0 += R) {
#pragma unroll
      for (int s = 0; s < R; ++s) {
        consume(kr[s], vr[s]);
        refill(s);
      }
    }
#pragma unroll
    for (int s = 0; s < R; ++s)
      if (j0 + s < total) consume(kr[s], vr[s]);
    // merge the wave's lane groups (each holds its own max / sum / o)
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float mx = sh_groups_max<LPK>(mrun[g]);
      const float f = mrun[g] == -INFINITY ? 0.0f : __expf(mrun[g] - mx);
      const float l = sh_groups_sum<LPK>(lrun[g] * f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[g][e] = sh_groups_sum<LPK>(acc[g][e] * f);
      mrun[g] = mx;
      lrun[g] = l;
    }
  }
  if (lane < LPK) {
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) s_acc[wave][g][dl * 8 + e] = acc[g][e];
  }
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      s_m[wave][g] = mrun[g];
      s_l[wave][g] = lrun[g];
    }
  }
  __syncthreads();
  // one thread per (q-head of the group, pair of dims): the waves' own part, then the merge with the prefix
  for (int idx = tid; idx < G * HD / 2; idx += NW * 64) {
    const int g = idx / (HD / 2), d = 2 * (idx - g * (HD / 2));
    float mo = s_m[0][g];
#pragma unroll
    for (int w = 1; w < NW; ++w) mo = fmaxf(mo, s_m[w][g]);
    float o0 = 0.0f, o1 = 0.0f, lo = 0.0f;
    if (mo != -INFINITY) {
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const float f = s_m[w][g] == -INFINITY ? 0.0f : __expf(s_m[w][g] - mo);
        o0 = fmaf(f, s_acc[w][g][d], o0);
        o1 = fmaf(f, s_acc[w][g][d + 1], o1);
        lo = fmaf(f, s_l[w][g], lo);
      }
    }
    const int col = m * G + g, blk = col >> 4, r = col & 15;
    const float* part = ws + (size_t)(blk * kv_heads + kvh) * S * kShPart<HD>;
    float mx = mo;   // finite after the loop: the prefix's last split is never empty
    for (int sp = 0; sp < S; ++sp) mx = fmaxf(mx, part[(size_t)sp * kShPart<HD> + 16 * HD + r]);
    float n0 = 0.0f, n1 = 0.0f, den = 0.0f;
    for (int sp = 0; sp < S; ++sp) {   // split order 0 .. S - 1
      const float* ps = part + (size_t)sp * kShPart<HD>;
      const float ms = ps[16 * HD + r];
      const float f = ms == -INFINITY ? 0.0f : __expf(ms - mx);
      const float2 o = *(const float2*)(ps + r * HD + d);
      den = fmaf(f, ps[16 * HD + 16 + r], den);
      n0 = fmaf(f, o.x, n0);
      n1 = fmaf(f, o.y, n1);
    }
    {   // the own part last
      const float f = mo == -INFINITY ? 0.0f : __expf(mo - mx);
      den = fmaf(f, lo, den);
      n0 = fmaf(f, o0, n0);
      n1 = fmaf(f, o1, n1);
    }
    const int K = heads * HD, k = (kvh * G + g) * HD + d;
    const size_t at = out_kt > 0 ? TI_PACKED_INDEX(m, k, out_kt) : (size_t)m * K + k;   // (k even: the pair is adjacent)
    *(uint32_t*)(out + at) = (uint32_t)f2h(n0 / den) | ((uint32_t)f2h(n1 / den) << 16);
  }
}

template <int HD>
static int launch_own(int G, dim3 grid, hipStream_t s, const float* q, const uint16_t* kc, const uint16_t* vc, int64_t stride,
                      int max_seq, const int32_t* pos, int heads, int P, int S, float scale, const float* ws, int out_kt,
                      uint16_t* out) {
  const dim3 block(kShOwnWaves * 64);
#define TI_SH_OWN(GG)                                                                                                       \
  hipLaunchKernelGGL((attn_shared_own_kernel<HD, GG>), grid, block, 0, s, q, kc, vc, stride, max_seq, pos, heads, P, S, scale, \
                     ws, out_kt, out)
  switch (G) {
    case 1: TI_SH_OWN(1); break;
    case 2: TI_SH_OWN(2); break;
    case 4: TI_SH_OWN(4); break;
    default: TI_SH_OWN(8); break;
  }
#undef TI_SH_OWN
  TI_LAUNCH_CHECK("attn_shared_own_kernel");
  return TI_OK;
}

// column blocks x kv-heads of M streams, the largest over the group sizes the entry point takes
static size_t sh_blocks(int M, int heads) {
  size_t nb = 0;
  for (int G = 1; G <= 8; G <<= 1)
    if (heads % G == 0) nb = std::max(nb, (size_t)((M * G + 15) / 16) * (size_t)(heads / G));
  return nb;
}

}  // namespace ti

extern "C" size_t ti_attn_shared_workspace_bytes(int M, int heads, int head_dim, int splits) {
  if (M < 1 || M > TI_ATTN_MAX_M || heads < 1 || heads > 65535 || (head_dim != 64 && head_dim != 128) || splits < 1 ||
      splits > 32)
    return 0;
  return ti::sh_blocks(M, heads) * (size_t)splits * (size_t)(16 * head_dim + 32) * sizeof(float);
}

extern "C" int ti_attn_decode_shared(const float* q, const uint16_t* k_cache, const uint16_t* v_cache, int64_t kv_stream_stride,
                                     int max_seq, const int32_t* pos, int M, int heads, int kv_heads, int head_dim,
                                     int prefix_len, int splits, int packed, float* workspace, uint16_t* out,
                                     ti_stream_t stream) {
  const char* name = "ti_attn_decode_shared";
  if (!q || !k_cache || !v_cache || !pos || !workspace || !out) return ti_set_error(TI_ERR_ARG, "%s: null pointer", name);
  if (M < 1 || M > TI_ATTN_MAX_M || heads < 1 || heads > 65535 || kv_heads < 1 || heads % kv_heads || max_seq < 1)
    return ti_set_error(TI_ERR_ARG, "%s: bad sizes M=%d (1..%d) heads=%d kv_heads=%d max_seq=%d", name, M, TI_ATTN_MAX_M, heads,
                        kv_heads, max_seq);
  if (head_dim != 64 && head_dim != 128) return ti_set_error(TI_ERR_ARG, "%s: head_dim %d not in {64,128}", name, head_dim);
  const int G = heads / kv_heads;
  if (G != 1 && G != 2 && G != 4 && G != 8) return ti_set_error(TI_ERR_ARG, "%s: heads / kv_heads %d not in {1,2,4,8}", name, G);
  if (prefix_len < 1 || prefix_len >= max_seq)
    return ti_set_error(TI_ERR_ARG, "%s: prefix_len %d outside [1, max_seq %d)", name, prefix_len, max_seq);
  if (splits < 1 || splits > 32) return ti_set_error(TI_ERR_ARG, "%s: splits %d outside [1, 32]", name, splits);
  if (packed && ((heads * head_dim) & 127))
    return ti_set_error(TI_ERR_ARG, "%s: packed needs heads * head_dim %d a multiple of 128", name, heads * head_dim);
  if (kv_stream_stride <= 0) return ti_set_error(TI_ERR_ARG, "%s: kv_stream_stride must be positive", name);
  // (a kv-head's cache sits behind one 2 GiB buffer resource)
  if ((int64_t)max_seq * head_dim * 2 > 0x7fffffffLL) return ti_set_error(TI_ERR_ARG, "%s: max_seq %d too large", name, max_seq);
  const int gsh = __builtin_ctz(G);
  const float scale = 1.0f / sqrtf((float)head_dim);
  hipStream_t s = (hipStream_t)stream;
  const dim3 g1((M * G + 15) / 16, kv_heads, splits);
  if (head_dim == 128)
    hipLaunchKernelGGL((ti::attn_shared_prefix_kernel<128>), g1, dim3(64), 0, s, q, k_cache, v_cache, max_seq, M, heads, gsh,
                       prefix_len, scale, workspace);
  else
    hipLaunchKernelGGL((ti::attn_shared_prefix_kernel<64>), g1, dim3(64), 0, s, q, k_cache, v_cache, max_seq, M, heads, gsh,
                       prefix_len, scale, workspace);
  TI_LAUNCH_CHECK("attn_shared_prefix_kernel");
  const dim3 g2(kv_heads, M);
  const int out_kt = packed ? heads * head_dim / 128 : 0;
  return head_dim == 128 ? ti::launch_own<128>(G, g2, s, q, k_cache, v_cache, kv_stream_stride, max_seq, pos, heads, prefix_len,
                                               splits, scale, workspace, out_kt, out)
                         : ti::launch_own<64>(G, g2, s, q, k_cache, v_cache, kv_stream_stride, max_seq, pos, heads, prefix_len,
                                              splits, scale, workspace, out_kt, out);
}
