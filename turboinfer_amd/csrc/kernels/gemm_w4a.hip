// gemm_w4a.hip -- GGUF Q4_1 weights (affine group-32 int4, bits 4 | TI_BITS_G32 | TI_BITS_AFF) x fp16 rows on MFMA
// for 17 .. TI_GEMM_MAX_ROWS rows (gfx950): batched decode above 16 streams and prompt chunks of affine engines
// (ti_gemm_wq_a16 with TI_X_F16 rows, M >= 17).  The fused gemv_wq_kernel<4, .., G32, AFF> stays the
// Q4_1 kernel up to 16 rows.
//
// y[M][N] = x[M][K] . W, W = d q + m per 32-weight block, in the tiles, scales and minimums of ti_wpack_q1_host as
// they are: a tile is 16 outputs x 128 k in 1 KiB, lane l = 16 kq + r holds one dwordx4 whose word s4 is
// k = 32 s4 + 8 kq + e of output r (element 2p at bits 4p, element 2p + 1 at bits 16 + 4p, the nibble ggml's q in
// 0 .. 15); the 64 fp16 block scales d of a tile and group are [s4][output], the 64 block minimums m have the same
// layout ti_wpack_scale_bytes(4 | TI_BITS_G32, K, N) bytes behind the scales.  The arithmetic is the fused
// kernel's decomposition, weight = d (q - 8) + (8 d + m): one v_mfma_f32_16x16x32_f16 from zero sums x (q - 8) over
// one block, then acc = fmaf(d, block_sum, acc) and acc = fmaf(fmaf(8, d, m), sx, acc) per block in k order, sx the
// fp32 sum of the row's 32 activations of the block.
//
// Shape of the work (a sibling of gemm_w8_kernel and gemm_w16_kernel; the stream is what differs):
//   * a workgroup of 8 waves owns one row block of 16 RB rows (RB 2: at most 32 rows, else 4) and one column block
//     of WC TPW tiles; its waves are WC = 8 / KW column-waves x KW k-waves, k-wave q takes group j KW + q of step
//     j: K is split INSIDE the workgroup only.
//   * weights: HBM -> VGPRs, per lane, tile and group one dwordx4 of nibbles and one coalesced 4-byte load of the
//     tile's scales (lanes 0 .. 31: entries 2 l, 2 l + 1) or minimums (lanes 32 .. 63), in a ring w4a_ring(TPW)
//     steps deep: a tile costs a quarter of fp16's registers, so the ring is 7 / 5 deep where fp16's is 4 / 3 (a
//     register decision; 2-byte loads of entry `lane` made the compiler wait on them a step early).
//   * dequantization is exact and in registers (deq_q4_exact: 9 VALU per B fragment, which feeds RB MFMAs); the x
//     image is the family's plain swizzled fp16 image (tile_swz) -- no pre-scaled slots, no corr table.  The A
//     fragment of step s4 is chunk 4 s4 + kq (group-32 order, compute32 of gemm_w8.hip).
//   * sx: where x is staged, the thread holding piece (row, chunk c) sums its 8 values in fp32 in a fixed order,
//     two cross-lane adds over the 4 adjacent lanes of block c >> 2 follow, one lane writes
//     bsum[buffer][k-wave][s4][row]; the table is double-buffered with the x image behind it and shares its
//     barrier.  Lane (r, kq) reads rows 16 b + 4 kq .. + 3 of a block with one ds_read_b128: the MFMA C layout.
//   * d and m of (block s4, output r) reach lane (r, kq) from lanes 8 s4 + r / 2 and 32 + 8 s4 + r / 2, which
//     loaded their dwords: one ds_bpermute each per block and tile, then a shift by 16 (r & 1).
//   * after the stream the k-waves' accumulators are summed through LDS in k-wave order (fixed: a second launch
//     gives the same bits; no split-K between workgroups, no tickets, no atomics on sums); the column-waves of
//     k-wave 0 run the staged epilogues of gemm_shared.hpp, one tile at a time.
#include <stdlib.h>

#include "gemm_shared.hpp"

namespace ti {

// Weight ring depth (steps): a step holds 5 TPW VGPRs (4 of nibbles, one of scales / minimums).  7 / 5 keep
// 7.5 / 10 KiB of weight loads in flight per wave (the INT8 kernel: 6 / 8 KiB) with no instance in scratch --
// DESIGN 4.34, the resource table.  The depth is a register decision; no depth was measured against another.
__host__ __device__ constexpr int w4a_ring(int tpw) { return tpw == 1 ? 7 : 5; }
__host__ __device__ constexpr int w4a_x_bytes(int rb, int kw) { return 2 * kw * 16 * rb * 256; }
__host__ __device__ constexpr int w4a_bsum_bytes(int rb, int kw) { return 2 * kw * 4 * 16 * rb * 4; }   // <= 8 KiB
__host__ __device__ constexpr int w4a_lds_bytes(int rb, int kw) {
  const int stream = w4a_x_bytes(rb, kw) + w4a_bsum_bytes(rb, kw);
  return stream > tile_epi_lds_bytes() ? stream : tile_epi_lds_bytes();
}

// One word of 8 nibbles -> the B fragment q - 8, exactly: (w & 0x000F000F) | 0x64006400 is fp16 1024 + q and
// (w & 0x00F000F0) | 0x54005400 is fp16 64 + q (one ulp at 64 is 1/16, the nibble sits 4 bits up); a packed
// subtract of 1032 / 72 leaves q - 8.  The same two for w >> 8.
__device__ __forceinline__ f16x8 deq_q4_exact(uint32_t w) {
  const f16x2 k1032 = {(f16)1032.0f, (f16)1032.0f}, k72 = {(f16)72.0f, (f16)72.0f};
  const uint32_t w8 = w >> 8;
  const f16x2 e01 = __builtin_bit_cast(f16x2, (w & 0x000F000Fu) | 0x64006400u) - k1032;
  const f16x2 e23 = __builtin_bit_cast(f16x2, (w & 0x00F000F0u) | 0x54005400u) - k72;
  const f16x2 e45 = __builtin_bit_cast(f16x2, (w8 & 0x000F000Fu) | 0x64006400u) - k1032;
  const f16x2 e67 = __builtin_bit_cast(f16x2, (w8 & 0x00F000F0u) | 0x54005400u) - k72;
  return (f16x8){e01[0], e01[1], e23[0], e23[1], e45[0], e45[1], e67[0], e67[1]};
}

template <int RB, int TPW, int KW>
__global__ __launch_bounds__(kGemvThreads, 1) void gemm_w4a_kernel(const GemvArgs a, int n_cb, int n_rb) {
  const unsigned long long t_entry = stamp_now();
  constexpr int WC = kGemvWaves / KW, BM = 16 * RB;   // column-waves, rows per workgroup
  constexpr int NX = BM * KW * 16 / kGemvThreads;     // 16-byte pieces of a step's x block per thread
  constexpr int D = w4a_ring(TPW);
  constexpr int XB = KW * BM * 128, BS = KW * 4 * BM;   // elements of one x buffer (fp16) / one bsum buffer (fp32)
  static_assert(NX >= 1 && RB * KW <= 16 && (KW - 1) * TPW <= KW * KW, "x block / k-wave slabs within the LDS image");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int KT = a.K >> 7, NT = a.N >> 4;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wn = wave % WC, q = wave / WC;
  // blockIdx -> (row block, column block): the n_rb row blocks of a column block share an XCD
  const int b8 = blockIdx.x & 7, rest = blockIdx.x >> 3;
  const int rb = rest % n_rb, cb = (rest / n_rb) * 8 + b8;
  if (cb >= n_cb) return;
  const int m0 = rb * BM, t0 = cb * WC * TPW;
  const int nsteps = (KT + KW - 1) / KW;
  f16* xb = (f16*)smem;                                 // [2][KW][BM rows][128 k], 16-byte chunks swizzled by tile_swz(row)
  float* bsum = (float*)(smem + w4a_x_bytes(RB, KW));   // [2][KW][4 blocks][BM rows]: sums of x per 32-k block

  // ---- x block of step j: global -> xr (rows and groups clamped into the call) -> LDS buffer j & 1, with the
  // block sums: piece i is (row, chunk c), the 4 lanes c & ~3 .. + 3 hold block c >> 2 of the row
  const f16* xsrc[NX];
  int xdst[NX], xq[NX], bdst[NX];
#pragma unroll
  for (int u = 0; u < NX; ++u) {
    const int i = tid + u * kGemvThreads, row = (i >> 4) % BM, c = i & 15;
    xq[u] = i / (BM * 16);
    xsrc[u] = (const f16*)a.x + (size_t)min(m0 + row, a.M - 1) * a.ldx + c * 8;
    xdst[u] = (xq[u] * BM + row) * 128 + ((c ^ tile_swz(row)) * 8);
    bdst[u] = (xq[u] * 4 + (c >> 2)) * BM + row;
  }
  u32x4 xr[NX];
  auto load_x = [&](int j) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NX; ++u) xr[u] = *(const u32x4*)(xsrc[u] + min(j * KW + xq[u], KT - 1) * 128);
  };
  auto store_x = [&](int j) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NX; ++u) {
      *(u32x4*)(xb + (j & 1) * XB + xdst[u]) = xr[u];
      const f16x8 h = __builtin_bit_cast(f16x8, xr[u]);
      float s = (((float)h[0] + (float)h[1]) + ((float)h[2] + (float)h[3])) +
                (((float)h[4] + (float)h[5]) + ((float)h[6] + (float)h[7]));
      s = group_sum<4>(s);
      if ((lane & 3) == 0) bsum[(j & 1) * BS + bdst[u]] = s;
    }
  };

  // ---- the wave's weight tiles, scales and minimums (tiles past N clamped, never stored): per tile and group
  // kWave u32x4 of nibbles and 64 + 64 fp16 [block s4][output] = 32 + 32 dwords; lane l < 32 loads dword l of the
  // scales, lane l >= 32 dword l - 32 of the minimums (one coalesced 4-byte load per lane: entry pairs 2 l, 2 l + 1)
  const u32x4* wt[TPW];
  const uint32_t* st[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tn = min(t0 + wn * TPW + t, NT - 1);
    wt[t] = a.tiles + (size_t)tn * KT * kWave + lane;
    // (the minimums follow all N / 16 tiles' scales)
    st[t] = (const uint32_t*)(a.scales + (lane < 32 ? (size_t)0 : (size_t)NT * KT * 64) + (size_t)tn * KT * 64) + (lane & 31);
  }
  u32x4 W[D][TPW];
  uint32_t S[D][TPW];
  auto load_w = [&](int slot, int j) __attribute__((always_inline)) {
    const int kg = min(min(j, nsteps - 1) * KW + q, KT - 1);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      W[slot][t] = wt[t][(size_t)kg * kWave];
      S[slot][t] = st[t][kg * 32];
    }
  };

  f32x4 acc[TPW][RB];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int b = 0; b < RB; ++b) acc[t][b] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

  // lane (r, kq): A fragment of block s4 and row block b = row b 16 + r, chunk 4 s4 + kq (k = 32 s4 + 8 kq .. + 7);
  // B fragment = the lane's word s4 of the tile, the same k of output r: one MFMA from zero is the block's sum of
  // x (q - 8) for rows b 16 + 4 kq .. + 3 (C layout), and bs[b] holds those rows' sx.  The TPW x 4 (block, tile)
  // units run as one software pipeline (compute32 of gemm_w8.hip): the loads, the bpermute and the MFMAs of unit
  // u + 1 ahead of the FMAs of unit u, so only two units' sums (2 RB f32x4) are live beside the accumulators.
  auto compute = [&](int slot, int j) __attribute__((always_inline)) {
    const f16* xrow = xb + (j & 1) * XB + (q * BM + r) * 128;
    const float* bsq = bsum + (j & 1) * BS + q * 4 * BM + 4 * kq;
    constexpr int NU = 4 * TPW;   // unit u: block s4 = u / TPW of tile t = u % TPW
    const int half = 16 * (r & 1);   // entry 16 s4 + r is half r & 1 of dword 8 s4 + r / 2
    f16x8 xf[RB];
    f32x4 bs[2][RB], sum[2][RB];   // bs by block parity: unit u's FMAs run after block s4 + 1's loads
    float d[2], mt[2];
    auto mfmas = [&](int u) __attribute__((always_inline)) {
      const int s4 = u / TPW, t = u % TPW;
      if (t == 0) {
#pragma unroll
        for (int b = 0; b < RB; ++b) {
          xf[b] = *(const f16x8*)(xrow + b * 16 * 128 + (((s4 * 4 + kq) ^ tile_swz(r)) * 8));
          bs[s4 & 1][b] = *(const f32x4*)(bsq + s4 * BM + b * 16);
        }
      }
      const int src = 4 * (8 * s4 + (r >> 1));   // (byte address of the source lane; + 32 lanes: the minimums)
      const uint32_t de = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)S[slot][t]) >> half;
      const uint32_t me = (uint32_t)__builtin_amdgcn_ds_bpermute(src + 128, (int)S[slot][t]) >> half;
      d[u & 1] = h2f((uint16_t)de);
      mt[u & 1] = fmaf(8.0f, d[u & 1], h2f((uint16_t)me));
      const f16x8 bf = deq_q4_exact(W[slot][t][s4]);
#pragma unroll
      for (int b = 0; b < RB; ++b)
        sum[u & 1][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xf[b], bf, (f32x4){0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
    };
    mfmas(0);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      if (u + 1 < NU) mfmas(u + 1);
#pragma unroll
      for (int b = 0; b < RB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[u % TPW][b][i] = fmaf(d[u & 1], sum[u & 1][b][i], acc[u % TPW][b][i]);
          acc[u % TPW][b][i] = fmaf(mt[u & 1], bs[(u / TPW) & 1][b][i], acc[u % TPW][b][i]);
        }
    }
  };

  // ---- the stream.  Step j: x(j + 1) -> registers, W(j + D - 1) -> ring (x first: the wait for x at the
  // step's end then leaves the younger weight loads in flight), compute j from buffer j & 1, x(j + 1) and its
  // block sums -> buffer (j + 1) & 1 (last read in step j - 1, which every wave left at the previous barrier),
  // barrier.
  load_x(0);
#pragma unroll
  for (int u = 0; u < D - 1; ++u) load_w(u, u);
  store_x(0);
  lds_barrier();
  for (int j0 = 0; j0 < nsteps; j0 += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int j = j0 + u;
      if (j < nsteps) {   // (uniform over the workgroup)
        if (j + 1 < nsteps) load_x(j + 1);
        load_w((u + D - 1) % D, j + D - 1);
        if (j * KW + q < KT) compute(u, j);   // (uniform over the wave: K / 128 need not divide by KW)
        if (j + 1 < nsteps) store_x(j + 1);
        lds_barrier();
      }
    }
  }

  // ---- k-waves: slabs [k-wave 1 .. KW - 1][column-wave][TPW RB][64 lanes] f32x4 over the x image (every
  // wave is past its last read of it), summed by k-wave 0 in k-wave order
  if constexpr (KW > 1) {
    f32x4* red = (f32x4*)smem;
    if (q > 0) {
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int b = 0; b < RB; ++b) red[(((q - 1) * WC + wn) * (TPW * RB) + t * RB + b) * kWave + lane] = acc[t][b];
    }
    lds_barrier();
    if (q == 0) {
#pragma unroll
      for (int qq = 1; qq < KW; ++qq)
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
          for (int b = 0; b < RB; ++b) {
            const f32x4 p = red[(((qq - 1) * WC + wn) * (TPW * RB) + t * RB + b) * kWave + lane];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t][b][i] += p[i];
          }
    }
    lds_barrier();   // the staging blocks below overlay the slabs
  }
  if (q == 0) {
    // ---- epilogue, one weight tile at a time through the wave's own staging block: lane (r, kq) holds
    // rows b 16 + 4 kq + i of column r (LDS program order within the wave orders the block's writes and reads)
    const int ek = a.epi.kind;
    const bool extra = ek == TI_EPI_STORE_F16 || ek == TI_EPI_LOGITS_ARGMAX;
    float* stg = (float*)smem + wn * (64 * kTileEpiStride);
    unsigned long long best[RB];
#pragma unroll
    for (int b = 0; b < RB; ++b) best[b] = 0ull;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int tn = t0 + wn * TPW + t;
#pragma unroll
      for (int b = 0; b < RB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) stg[(b * 16 + 4 * kq + i) * kTileEpiStride + r] = acc[t][b][i];
      if (tn < NT) {
        if (extra) tile_epilogue_extra<RB>(a, tn, m0, stg, lane, best);
        else tile_epilogue_lds<RB>(a, tn, m0, stg, lane);
      }
    }
    if (ek == TI_EPI_LOGITS_ARGMAX) {
      // one key per row and wave: the 4 lanes of a row, then one atomicMax into the workgroup's slot
#pragma unroll
      for (int it = 0; it < RB; ++it) {
        unsigned long long key = best[it];
#pragma unroll
        for (int o = 1; o < 4; o <<= 1) {
          const unsigned long long other = __shfl_xor(key, o, kWave);
          key = other > key ? other : key;
        }
        const int m = m0 + 16 * it + (lane >> 2);
        if ((lane & 3) == 0 && key && m < a.M)
          atomicMax(a.epi.argmax + (size_t)m * TI_ARGMAX_SLOTS + (blockIdx.x & (TI_ARGMAX_SLOTS - 1)), key);
      }
      if (a.epi.step_ctr && blockIdx.x == 0 && tid == 0) *a.epi.step_ctr += a.epi.advance;
    }
  }
  stamp_end(a.stamp, t_entry);
}

// ------------------------------------------------------------------------------------------------ host
// TI_GEMM_W4A_ROWS=0: Q4_1 rows above 16 are cut into 16-row fused pieces by ti_gemm_wq_a16 and by the engine, as
// before this kernel (A/B knob, read once per process).
bool w4a_rows_on() {
  static const bool on = [] {
    const char* e = getenv("TI_GEMM_W4A_ROWS");
    return e ? atoi(e) != 0 : true;
  }();
  return on;
}

// Instances: two tiles per wave only without a k-wave split (TPW 2 with KW k-waves has the column block of TPW 1
// with KW / 2 and a larger slab trip: the plan below never picks it), 8 k-waves only at RB 2 (the LDS image).
#define TI_W4A_FNS_RB(RB)                                                                   \
  (const void*)gemm_w4a_kernel<RB, 1, 1>, (const void*)gemm_w4a_kernel<RB, 1, 2>,           \
      (const void*)gemm_w4a_kernel<RB, 1, 4>, (const void*)gemm_w4a_kernel<RB, 2, 1>
static const void* const g_w4a_fns[] = {TI_W4A_FNS_RB(2), TI_W4A_FNS_RB(4), (const void*)gemm_w4a_kernel<2, 1, 8>};
static const void* w4a_fn(int rb, int tpw, int kw) {
  if (kw == 8) return g_w4a_fns[8];
  return g_w4a_fns[(rb == 4 ? 4 : 0) + (tpw == 2 ? 3 : kw == 1 ? 0 : kw == 2 ? 1 : 2)];
}

// The plan: w8_plan's per-CU byte model with 1024 + 256 B per tile and group (nibbles, scales and minimums).  RB 2
// up to 32 rows, else 4; over tiles per wave TPW in {1, 2} and k-waves KW in {1, 2, 4, 8 (RB 2)} with
// KW <= K / 128, the launch takes ceil(workgroups of an XCD / its CUs) rounds, a workgroup moves per 128-k group
// its x rows (16 RB x 256 B) and its (8 / KW) TPW tiles, and a k-wave split adds its slabs' trip through LDS
// once; the cheapest shape wins, ties to fewer k-waves and then to more tiles per wave.  (TPW 2 with KW > 1 always
// loses that comparison to TPW 1 with KW / 2, which has the same column block: not a candidate, not instantiated.)
W4aPlan w4a_plan(int M, int N, int K, int cus) {
  const int NT = N >> 4, KT = K >> 7, rb = M <= 32 ? 2 : 4, bm = 16 * rb;
  const int n_rb = (M + bm - 1) / bm, xcd_cus = cus >= 8 ? cus / 8 : 1;
  W4aPlan best{};
  long best_cost = -1;
  for (int kw : {1, 2, 4, 8}) {
    if (kw > KT || rb * kw > 16) continue;
    for (int tpw : {2, 1}) {
      if (tpw == 2 && kw > 1) continue;
      const int cols = (8 / kw) * tpw, n_cb = (NT + cols - 1) / cols;
      const long per_xcd = (long)(n_cb + 7) / 8 * n_rb, rounds = (per_xcd + xcd_cus - 1) / xcd_cus;
      const long cost = rounds * ((long)KT * (bm * 256 + cols * 1280) + (kw > 1 ? (long)(kw - 1) * cols * rb * 1024 : 0));
      if (best_cost < 0 || cost < best_cost) {
        best_cost = cost;
        best.rb = rb; best.tpw = tpw; best.kw = kw; best.n_cb = n_cb; best.n_rb = n_rb;
        best.grid = (n_cb + 7) / 8 * 8 * n_rb;
        best.lds = w4a_lds_bytes(rb, kw);
      }
    }
  }
  return best;
}

int w4a_prepare() {
  for (const void* f : g_w4a_fns)
    TI_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                 "hipFuncSetAttribute(gemm_w4a_kernel)");
  return TI_OK;
}

int launch_w4a(const GemvArgs& a, const W4aPlan& p, hipStream_t s) {
  GemvArgs args = a;
  int n_cb = p.n_cb, n_rb = p.n_rb;
  void* kargs[] = {&args, &n_cb, &n_rb};
  TI_HIP_CHECK(hipLaunchKernel(w4a_fn(p.rb, p.tpw, p.kw), dim3(p.grid), dim3(kGemvThreads), kargs, p.lds, s),
               "hipLaunchKernel(gemm_w4a_kernel)");
  TI_LAUNCH_CHECK("gemm_w4a_kernel");
  return TI_OK;
}

}  // namespace ti
