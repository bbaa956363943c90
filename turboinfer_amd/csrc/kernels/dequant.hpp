// dequant.hpp -- packed INT4 / INT8 weight words -> fp16 MFMA B fragments (gfx950), shared by
// the decode GEMV (gemv.hip) and the persistent decode-layers kernel (pds.hip).
#pragma once
#include "common.hpp"

namespace ti {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------- dequant
// int4: word of 8 nibbles, nibble p holds element 2p, nibble p+4 element 2p+1, value q+8.
// int8: 4 signed bytes in k order; (b ^ 0x80) = b + 128 -> fp16 1024 + b + 128 - 1152.
__device__ __forceinline__ f16x2 deq_int8_pair(uint32_t t, uint32_t sel) {
  const uint32_t v = __builtin_amdgcn_perm(0x64646464u, t, sel);
  return __builtin_bit_cast(f16x2, v) - (f16x2){(f16)1152.0f, (f16)1152.0f};
}
__device__ __forceinline__ void deq_int8_word(uint32_t w, f16x8& r, int o) {
  const uint32_t t = w ^ 0x80808080u;
  const f16x2 lo = deq_int8_pair(t, 0x04010400u), hi = deq_int8_pair(t, 0x04030402u);
  r[o + 0] = lo[0];
  r[o + 1] = lo[1];
  r[o + 2] = hi[0];
  r[o + 3] = hi[1];
}

// int4, offset folded (5 VALU ops per 8 weights): fp16 lanes hold 1024 + n for the low
// nibble of each byte and 1024 + 16 n for the high one -- the raw bit patterns after one
// v_and_or_b32 each.  The activations are staged so that this is exact arithmetic: x at
// k % 8 in {2,3,6,7} (high-nibble slots) is pre-scaled by 1/16, making a_k * (1024 + 16 n)
// = 64 x_k + x_k n, and the MFMA sum t of one 128-k group then equals
//   sum_k x_k (n_k - 8) + D,   D = 1032 * sum_lo a_k + 1152 * sum_hi a_k,
// with D depending only on the activation row and the group: it is precomputed once per
// workgroup (corr table) and subtracted before the group scale is applied.
__device__ __forceinline__ f16x8 deq_int4_raw(uint32_t w, uint32_t magic) {
  const uint32_t w8 = w >> 8;
  u32x4 r;
  r[0] = (w & 0x000F000Fu) | magic;
  r[1] = (w & 0x00F000F0u) | magic;
  r[2] = (w8 & 0x000F000Fu) | magic;
  r[3] = (w8 & 0x00F000F0u) | magic;
  return __builtin_bit_cast(f16x8, r);
}

// MXFP4 (TI_BITS_MX): the same word layout with the raw e2m1 code per nibble.  v_cvt_scalef32_pk_f16_fp4 at scale
// 1 widens the two nibbles of one byte exactly (every e2m1 value is an fp16 value): byte b holds nibbles 2b and
// 2b + 1, i.e. the element pairs (0, 2), (4, 6), (1, 3), (5, 7) for b = 0..3; four half-word picks
// put them back in k order (4 conversions + 4 v_perm / v_pack per 8 weights, no offset to remove afterwards).
__device__ __forceinline__ f16x8 deq_mxfp4(uint32_t w) {
  const uint32_t c0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 0));
  const uint32_t c1 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 1));
  const uint32_t c2 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 2));
  const uint32_t c3 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 3));
  u32x4 r;   // (v_perm_b32: selector bytes 0-3 pick from the second operand, 4-7 from the first)
  r[0] = __builtin_amdgcn_perm(c2, c0, 0x05040100u);   // elements 0, 1
  r[1] = __builtin_amdgcn_perm(c2, c0, 0x07060302u);   // elements 2, 3
  r[2] = __builtin_amdgcn_perm(c3, c1, 0x05040100u);   // elements 4, 5
  r[3] = __builtin_amdgcn_perm(c3, c1, 0x07060302u);   // elements 6, 7
  return __builtin_bit_cast(f16x8, r);
}
// The e8m0 block scale as fp32: 2^(e - 127) for 1 <= e <= 254.
__device__ __forceinline__ float e8m0_to_f32(uint32_t e) { return __builtin_bit_cast(float, e << 23); }

// Q4_K (TI_BITS_KQ): the same word layout with the raw q (0..15) per nibble, widened exactly: (w & 0x000F000F) |
// 0x64006400 is fp16 1024 + q and (w & 0x00F000F0) | 0x54005400 is fp16 64 + q (one ulp at 64 is 1/16, the nibble
// sits 4 bits up); a packed subtract of 1024 / 64 leaves q (gemm_w4a.hip's deq_q4_exact without the offset 8).
__device__ __forceinline__ f16x8 deq_q4k(uint32_t w) {
  const f16x2 k1024 = {(f16)1024.0f, (f16)1024.0f}, k64 = {(f16)64.0f, (f16)64.0f};
  const uint32_t w8 = w >> 8;
  const f16x2 e01 = __builtin_bit_cast(f16x2, (w & 0x000F000Fu) | 0x64006400u) - k1024;
  const f16x2 e23 = __builtin_bit_cast(f16x2, (w & 0x00F000F0u) | 0x54005400u) - k64;
  const f16x2 e45 = __builtin_bit_cast(f16x2, (w8 & 0x000F000Fu) | 0x64006400u) - k1024;
  const f16x2 e67 = __builtin_bit_cast(f16x2, (w8 & 0x00F000F0u) | 0x54005400u) - k64;
  return (f16x8){e01[0], e01[1], e23[0], e23[1], e45[0], e45[1], e67[0], e67[1]};
}

template <int BITS>
__device__ __forceinline__ f16x8 dequant_step(const u32x4 (&w)[BITS / 4], int s4, uint32_t magic) {
  if constexpr (BITS == 4) {
    return deq_int4_raw(w[0][s4], magic);
  } else if constexpr (BITS == 8) {
    f16x8 r;
    const u32x4 c = w[s4 >> 1];
    deq_int8_word(c[(s4 & 1) * 2 + 0], r, 0);
    deq_int8_word(c[(s4 & 1) * 2 + 1], r, 4);
    return r;
  } else {
    return __builtin_bit_cast(f16x8, w[s4]);
  }
}

}  // namespace ti
