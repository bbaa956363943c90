// wsynth_kq.hip -- seeded random Q4_K super-blocks generated straight into device tiles (TI_BITS_KQ):
// ti_wsynth_device's branch for bits 4 | TI_BITS_G32 | TI_BITS_KQ (misc.hip holds the other formats).  A timing
// model's weights, not a quantization of the synthetic fp32 model: ggml's Q4_K quantizer is a search.
#include <math.h>

#include "common.hpp"

namespace ti {

// One thread per (source column c, super-block sb).  With u(i) the seeded uniform stream of the tensor:
//   q(k)  = floor(8 (u(k N_src + c) + 1)) in 0..15,
//   sc_j  = 8 + floor(8 (u(K N_src + (8 sb + j) N_src + c) + 1)) in 8..23, m_j the same from the next K/32 N_src
//           indices (both halves of the 6-bit packing carry bits),
//   d     = fp16(amp / 120), dmin = fp16(7.5 amp / 120): weight = d sc_j q - dmin m_j is about amp (sc_j (q - 7.5)
//           + 7.5 (sc_j - m_j)) / 120, zero-centred with a spread near amp = sqrt(3 / K).
// The entry's layout is ti_hip.h's: d | dmin << 16, then field 2 j + (0: sc, 1: m) at bit 6 (2 j + ..) of 96.
__global__ __launch_bounds__(128) void wsynth_kq_kernel(uint64_t stream, int K, int N_src, int row_map, int row_offset,
                                                        float amp, uint8_t* tiles, uint32_t* scales) {
  const int KT = K >> 7, KS = K >> 8;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)N_src * KS) return;
  const int c = (int)(t % N_src), sb = (int)(t / N_src);
  const int n = row_map == TI_ROWS_INTERLEAVE8 ? 16 * (c >> 3) + (c & 7) + row_offset : row_offset + c;
  const int nt = n >> 4, r = n & 15;
  auto u16 = [&](uint64_t i, int lo, int span) {   // lo + floor(span (u + 1) / 2), clamped
    const int v = lo + (int)floorf((synth_unit(stream, i) + 1.0f) * (0.5f * (float)span));
    return (uint32_t)min(lo + span - 1, max(lo, v));
  };
  uint32_t w[4] = {(uint32_t)f2h_soft(amp / 120.0f) | ((uint32_t)f2h_soft(amp * (7.5f / 120.0f)) << 16), 0u, 0u, 0u};
  const uint64_t kn = (uint64_t)K * (uint64_t)N_src, bn = (uint64_t)(K >> 5) * (uint64_t)N_src;
#pragma unroll
  for (int f = 0; f < 16; ++f) {
    const uint32_t v = u16(kn + (f & 1 ? bn : 0) + (uint64_t)(8 * sb + (f >> 1)) * (uint64_t)N_src + (uint64_t)c, 8, 16);
    const int bit = 6 * f;
    w[1 + (bit >> 5)] |= v << (bit & 31);
    if ((bit & 31) > 26) w[2 + (bit >> 5)] |= v >> (32 - (bit & 31));
  }
  *(uint4*)(scales + (((size_t)nt * KS + sb) * 16 + r) * 4) = make_uint4(w[0], w[1], w[2], w[3]);
  for (int g = 2 * sb; g < 2 * sb + 2; ++g) {   // lane kq's word s4 holds k = 32 s4 + 8 kq + e (the group-32 order)
    uint8_t* tile = tiles + ((size_t)nt * KT + g) * 1024;
    for (int kq = 0; kq < 4; ++kq) {
      uint32_t words[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        uint32_t wd = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t nib = u16((uint64_t)(g * 128 + 32 * s4 + 8 * kq + e) * (uint64_t)N_src + (uint64_t)c, 0, 16);
          wd |= nib << ((e & 1) ? (16 + 4 * (e >> 1)) : (4 * (e >> 1)));
        }
        words[s4] = wd;
      }
      *(uint4*)(tile + (kq * 16 + r) * 16) = make_uint4(words[0], words[1], words[2], words[3]);
    }
  }
}

// (arguments checked by ti_wsynth_device; K % 256 == 0)
int launch_wsynth_kq(uint64_t stream_id, int K, int N_src, int row_map, int row_offset, float amp, void* tiles,
                     void* scales, hipStream_t s) {
  const int64_t n = (int64_t)N_src * (K >> 8);
  hipLaunchKernelGGL(wsynth_kq_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, s, stream_id, K, N_src, row_map,
                     row_offset, amp, (uint8_t*)tiles, (uint32_t*)scales);
  TI_LAUNCH_CHECK("wsynth_kq_kernel");
  return TI_OK;
}

}  // namespace ti
