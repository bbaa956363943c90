// wsynth_mx.hip -- the synthetic model's linear weights generated straight into MXFP4 tiles (TI_BITS_MX):
// ti_wsynth_device's branch for bits 4 | TI_BITS_G32 | TI_BITS_MX (misc.hip holds the other formats).
// Built without packed fp32 operations (Makefile): the quantization below is scalar fp32 arithmetic that has to
// agree bit for bit with ti_wpack_host's on the host.
#include <math.h>

#include "common.hpp"

namespace ti {

// ti_wpack_host's rule (ti_hip.h): e2m1 code of v, round-to-nearest-even onto {0, .5, 1, 1.5, 2, 3, 4, 6} (a tie
// goes to the even code), saturating at 6; bit 3 is the sign of v < 0.
__device__ __forceinline__ uint32_t mx_code(float v) {
  const float a = fabsf(v);
  // the midpoints between neighbouring codes; a tie moves up only from an odd code
  const uint32_t c = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
  return c | (v < 0.0f ? 8u : 0u);
}

// One thread per (source column c, k-group g): 128 seeded values; per 32-block e = floor(log2(absmax)) - 2 + 127
// clamped to [1, 254] (127 for an all-zero block) and the 32 codes of w * 2^(127 - e); lane kq's word s4 of the
// tile holds k = 32 s4 + 8 kq + e8 (the group-32 order), element 2p at bits 4p and 2p + 1 at bits 16 + 4p.
__global__ __launch_bounds__(128) void wsynth_mx_kernel(uint64_t stream, int K, int N_src, int row_map, int row_offset,
                                                        float amp, uint8_t* tiles, uint8_t* scales) {
  const int KT = K >> 7;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)N_src * KT) return;
  const int c = (int)(t % N_src), g = (int)(t / N_src);
  const int n = row_map == TI_ROWS_INTERLEAVE8 ? 16 * (c >> 3) + (c & 7) + row_offset : row_offset + c;
  const int nt = n >> 4, r = n & 15;
  uint8_t* tile = tiles + ((size_t)nt * KT + g) * 1024;
  uint32_t words[4][4];   // [kq][s4]
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) {
    float w[32];
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      w[i] = synth_unit(stream, (uint64_t)(g * 128 + s4 * 32 + i) * (uint64_t)N_src + (uint64_t)c) * amp;
      amax = fmaxf(amax, fabsf(w[i]));
    }
    // (the biased exponent of a normal fp32 is floor(log2) + 127; a subnormal absmax clamps to 1 either way)
    const int be = (int)((__builtin_bit_cast(uint32_t, amax) >> 23) & 0xffu);
    const int eb = amax > 0.0f ? min(254, max(1, be - 2)) : 127;
    scales[(((size_t)nt * KT + g) * 4 + s4) * 16 + r] = (uint8_t)eb;
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      uint32_t wd = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t nib = mx_code(ldexpf(w[8 * kq + e], 127 - eb));
        wd |= nib << ((e & 1) ? (16 + 4 * (e >> 1)) : (4 * (e >> 1)));
      }
      words[kq][s4] = wd;
    }
  }
#pragma unroll
  for (int kq = 0; kq < 4; ++kq)
    *(uint4*)(tile + (kq * 16 + r) * 16) = make_uint4(words[kq][0], words[kq][1], words[kq][2], words[kq][3]);
}

// (arguments checked by ti_wsynth_device)
int launch_wsynth_mx(uint64_t stream_id, int K, int N_src, int row_map, int row_offset, float amp, void* tiles,
                     void* scales, hipStream_t s) {
  const int64_t n = (int64_t)N_src * (K >> 7);
  hipLaunchKernelGGL(wsynth_mx_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, s, stream_id, K, N_src, row_map,
                     row_offset, amp, (uint8_t*)tiles, (uint8_t*)scales);
  TI_LAUNCH_CHECK("wsynth_mx_kernel");
  return TI_OK;
}

}  // namespace ti
