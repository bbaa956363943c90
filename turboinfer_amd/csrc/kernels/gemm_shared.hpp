// gemm_shared.hpp -- what the GEMM kernels of gemv.hip (int4 tile kernel), gemm_w8.hip (INT8 rows
// kernel), gemm_w16.hip (fp16-weight rows kernel), gemm_w4a.hip (Q4_1 rows kernel) and gemm_mx.hip (MXFP4 rows
// kernel) have in common and is independent of the weight format: the launch arguments, the swizzled
// activation image in LDS, the staged epilogue of a 64 x 16 output block.
#pragma once
#include "common.hpp"
#include "dequant.hpp"

namespace ti {

constexpr int kGemvWaves = 8;
constexpr int kGemvThreads = kGemvWaves * kWave;

struct GemvArgs {
  const u32x4* tiles;
  const uint16_t* scales;
  const void* x;
  const float* norm_w;
  float eps;
  int32_t x_kind, ldx, M, N, K;
  ti_epilogue epi;
  unsigned long long* stamp;   // in-step launch stamps (common.hpp stamp_end), NULL in product launches
};

__host__ __device__ constexpr int align16(int b) { return (b + 15) & ~15; }

__device__ __forceinline__ uint32_t float_order_key(float v) {
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// LDS barrier that leaves the wave's outstanding global loads in flight (a plain
// __syncthreads() may drain vmcnt): LDS writes retired, then s_barrier.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

constexpr int kTileEpiStride = 20;   // floats per row of a wave's 64 x 16 staging block (padded: no bank conflicts)
__host__ __device__ constexpr int tile_epi_lds_bytes() { return kGemvWaves * 64 * kTileEpiStride * 4; }

// Epilogue of weight tile tn (16 outputs) for rows mb .. mb + 63 of one wave, from its LDS block
// stg[row][col] (row stride kTileEpiStride).  Same arithmetic as epilogue_mb, element for element.
//   STORE_F32 / RESID_F32 / QKV_ROPE_KV: lane l owns columns 4 (l & 3) .. + 3 of rows 16 it + l / 4
//   SILU_MUL_F16: lane l owns outputs 4 (l & 1) .. + 3 (gate columns, up = column + 8) of rows 32 it + l / 2
template <int RB = 4>   // the wave's rows: 16 RB
__device__ __forceinline__ void tile_epilogue_lds(const GemvArgs& a, int tn, int mb, const float* stg, int lane) {
  const ti_epilogue& e = a.epi;
  if (e.kind == TI_EPI_SILU_MUL_F16) {
    const int h = 4 * (lane & 1);
#pragma unroll
    for (int it = 0; it < RB / 2; ++it) {
      const int row = 32 * it + (lane >> 1), m = mb + row;
      const float4 g = *(const float4*)(stg + row * kTileEpiStride + h);
      const float4 u = *(const float4*)(stg + row * kTileEpiStride + 8 + h);
      if (m >= a.M) continue;
      auto sm = [](float v, float up) { return f2h(up * (v / (1.0f + expf(-v)))); };
      const uint32_t lo = sm(g.x, u.x) | ((uint32_t)sm(g.y, u.y) << 16), hi = sm(g.z, u.z) | ((uint32_t)sm(g.w, u.w) << 16);
      *(uint2*)((uint16_t*)e.out + (size_t)m * e.ldo + tn * 8 + h) = make_uint2(lo, hi);
    }
    return;
  }
  const int c4 = 4 * (lane & 3), ng = tn * 16 + c4;
  // QKV: the tile lies in one of q / k / v and one head (head_dim % 16 == 0)
  const int hd = e.head_dim;
  const bool in_q = ng < e.q_dim, in_k = !in_q && ng < e.q_dim + e.kv_dim;
  const int c = in_q ? ng : in_k ? ng - e.q_dim : ng - e.q_dim - e.kv_dim;
  const int kvh = e.kind == TI_EPI_QKV_ROPE_KV ? c / hd : 0, d = c - kvh * hd;
#pragma unroll
  for (int it = 0; it < RB; ++it) {
    const int row = 16 * it + (lane >> 2), m = mb + row;
    const float4 v = *(const float4*)(stg + row * kTileEpiStride + c4);
    if (m >= a.M) continue;
    if (e.kind == TI_EPI_STORE_F32) {
      *(float4*)((float*)e.out + (size_t)m * e.ldo + ng) = v;
    } else if (e.kind == TI_EPI_RESID_F32) {
      float4* o = (float4*)((float*)e.out + (size_t)m * e.ldo + ng);
      const float4 h = *o;
      *o = make_float4(h.x + v.x, h.y + v.y, h.z + v.z, h.w + v.w);
    } else {   // TI_EPI_QKV_ROPE_KV
      const int p = e.pos[m];
      if (in_q || in_k) {
        // (cos, sin) of pairs d / 2 and d / 2 + 1: even output fmaf(-odd, sin, even * cos), odd
        // output fmaf(odd, cos, even * sin) (epilogue_mb with partner = the other of the pair)
        const float4 cs = *(const float4*)(e.rope_cs + (size_t)p * hd + d);
        const float r0 = fmaf(-v.y, cs.y, v.x * cs.x), r1 = fmaf(v.y, cs.x, v.x * cs.y);
        const float r2 = fmaf(-v.w, cs.w, v.z * cs.z), r3 = fmaf(v.w, cs.z, v.z * cs.w);
        if (in_q) {
          *(float4*)((float*)e.out + (size_t)m * e.ldo + ng) = make_float4(r0, r1, r2, r3);
        } else {
          const size_t ci = (size_t)m * e.kv_stream_stride + ((size_t)kvh * e.max_seq + p) * hd + d;
          if (e.kv_fp8)   // 4 elements -> one 32-bit store
            *(uint32_t*)((uint8_t*)e.k_cache + ci) = f2e4m3x4(r0, r1, r2, r3);
          else
            *(uint2*)(e.k_cache + ci) =
                make_uint2(f2h(r0) | ((uint32_t)f2h(r1) << 16), f2h(r2) | ((uint32_t)f2h(r3) << 16));
        }
      } else {
        const size_t ci = (size_t)m * e.kv_stream_stride + ((size_t)kvh * e.max_seq + p) * hd + d;
        if (e.kv_fp8)
          *(uint32_t*)((uint8_t*)e.v_cache + ci) = f2e4m3x4(v.x, v.y, v.z, v.w);
        else
          *(uint2*)(e.v_cache + ci) =
              make_uint2(f2h(v.x) | ((uint32_t)f2h(v.y) << 16), f2h(v.z) | ((uint32_t)f2h(v.w) << 16));
      }
    }
  }
}

// STORE_F16 and LOGITS_ARGMAX of weight tile tn from the wave's staging block (the layout of
// tile_epilogue_lds: lane l owns columns 4 (l & 3) .. + 3 of rows 16 it + l / 4).  best[it]: the lane's
// running argmax key of its rows (epilogue_mb's keys: the value's order key above, the lowest index wins).
template <int RB>
__device__ __forceinline__ void tile_epilogue_extra(const GemvArgs& a, int tn, int mb, const float* stg, int lane,
                                                    unsigned long long (&best)[RB]) {
  const ti_epilogue& e = a.epi;
  const int c4 = 4 * (lane & 3), ng = tn * 16 + c4;
#pragma unroll
  for (int it = 0; it < RB; ++it) {
    const int row = 16 * it + (lane >> 2), m = mb + row;
    const float4 v = *(const float4*)(stg + row * kTileEpiStride + c4);
    if (m >= a.M) continue;
    if (e.kind == TI_EPI_STORE_F16) {
      *(uint2*)((uint16_t*)e.out + (size_t)m * e.ldo + ng) =
          make_uint2(f2h(v.x) | ((uint32_t)f2h(v.y) << 16), f2h(v.z) | ((uint32_t)f2h(v.w) << 16));
    } else {   // TI_EPI_LOGITS_ARGMAX
      *(float4*)((float*)e.out + (size_t)m * e.ldo + ng) = v;
      const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned long long key = ((unsigned long long)float_order_key(vv[j]) << 32) |
                                       (unsigned long long)(0xFFFFFFFFu - (uint32_t)(ng + j));
        best[it] = key > best[it] ? key : best[it];
      }
    }
  }
}

// Physical 16-byte chunk of logical chunk c in activation row `row` of the tile kernel's LDS image:
// c ^ tile_swz(row).  An A-fragment read (ds_read_b128, lane l: row l & 15, chunk 4 (l >> 4) + s, or
// 4 s + (l >> 4) with group-32 weights) is serviced in the lane groups {0-3,12-15,20-27},
// {4-11,16-19,28-31}, {32-35,44-47,52-59}, {36-43,48-51,60-63} (MI355X_MICROARCH.md, LDS); each
// holds the 16 rows once, rows {0-3,12-15} at one chunk column and rows {4-11} at the next.  With
// (row + 4) & 15 the first set lands in chunks 0-7 and the second in 8-15 of a row, so the 16 lanes
// of a group hit 16 different chunks (64 banks): conflict-free.  (row & 15 put both sets on the
// same 8 chunks: 2-way conflicts in every group, SQ_LDS_BANK_CONFLICT 3.3 cycles per read.)
#ifndef TI_TILE_SWZ4
#define TI_TILE_SWZ4 1
#endif
__device__ __forceinline__ int tile_swz(int row) { return TI_TILE_SWZ4 ? (row + 4) & 15 : row & 15; }

// ------------------------------------------------------------- gemm_w8.hip (INT8 rows kernel), host side
// The instance of gemm_w8_kernel a call takes: 16 rb rows per workgroup, tpw tiles per wave, kw k-waves
// (8 / kw column-waves), n_cb column blocks x n_rb row blocks in `grid` workgroups, `lds` bytes of LDS.
struct W8Plan {
  int rb, tpw, kw, n_cb, n_rb, grid, lds;
  bool g32;   // the group-32 instance (Q8_0 blocks, 8 | TI_BITS_G32)
};
bool w8_rows_on();   // TI_GEMM_W8_ROWS (0: the route is off)
W8Plan w8_plan(int M, int N, int K, int cus, bool g32 = false);
int w8_prepare();    // dynamic-LDS cap of every instance (ti_gemm_prepare)
int launch_w8(const GemvArgs& a, const W8Plan& p, hipStream_t s);

// ------------------------------------------------------------ gemm_w16.hip (fp16-weight rows kernel), host side
// The instance of gemm_w16_kernel a call takes, in W8Plan's terms.
struct W16Plan {
  int rb, tpw, kw, n_cb, n_rb, grid, lds;
};
bool w16_rows_on();   // TI_GEMM_W16_ROWS (0: the route is off)
W16Plan w16_plan(int M, int N, int K, int cus);
int w16_prepare();    // dynamic-LDS cap of every instance (ti_gemm_prepare)
int launch_w16(const GemvArgs& a, const W16Plan& p, hipStream_t s);

// ------------------------------------------------------------ gemm_w4a.hip (Q4_1 rows kernel), host side
// The instance of gemm_w4a_kernel a call takes, in W8Plan's terms.
struct W4aPlan {
  int rb, tpw, kw, n_cb, n_rb, grid, lds;
};
bool w4a_rows_on();   // TI_GEMM_W4A_ROWS (0: the route is off)
W4aPlan w4a_plan(int M, int N, int K, int cus);
int w4a_prepare();    // dynamic-LDS cap of every instance (ti_gemm_prepare)
int launch_w4a(const GemvArgs& a, const W4aPlan& p, hipStream_t s);

// ------------------------------------------------------------ gemm_mx.hip (MXFP4 rows kernel), host side
// The instance of gemm_mx_kernel a call takes, in W8Plan's terms.
struct MxPlan {
  int rb, tpw, kw, n_cb, n_rb, grid, lds;
};
bool mx_rows_on();        // the route's switch: TI_GEMM_MX_ROWS at first use (default 0: off), then mx_rows_set
int mx_rows_set(int on);  // ti_gemm_set_mx_rows: sets the switch, returns its previous value
MxPlan mx_plan(int M, int N, int K, int cus);
int mx_prepare();         // dynamic-LDS cap of every instance (ti_gemm_prepare)
int launch_mx(const GemvArgs& a, const MxPlan& p, hipStream_t s);

}  // namespace ti
