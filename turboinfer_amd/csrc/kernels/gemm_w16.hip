// gemm_w16.hip -- fp16 weights x fp16 rows on MFMA for 17 .. TI_GEMM_MAX_ROWS rows (gfx950): batched decode
// above 16 streams and prompt chunks of fp16 engines (ti_gemm_wq_a16 with bits 16, TI_X_F16 rows, M >= 17;
// DESIGN 4.33).  The fused gemv_wq_kernel<16, ..> stays the fp16 kernel up to 16 rows.
//
// y[M][N] = x[M][K] . W with W in the fp16 tiles of ti_wpack_host(.., 16): a tile is 16 outputs x 128 k (4 KiB,
// four 1 KiB chunks; lane l of chunk c: 8 fp16 of output l & 15 at k = 32 (l >> 4) + 8 c).  Chunk c IS the B
// fragment of MFMA step s4 = c, so the stream is load -> MFMA: no widening, no scale, no correction.  The
// arithmetic is the fused kernel's fp16 path: one fp32 accumulator per (tile, 16-row block) threaded through
// v_mfma_f32_16x16x32_f16 over all of the k-wave's groups in k order (no per-group zero start).
//
// Shape of the work (a sibling of gemm_w8_kernel; what differs is the weight stream and the accumulation):
//   * a workgroup of 8 waves owns one row block of 16 RB rows (RB 2: at most 32 rows, else 4)
//     and one column block of WC TPW tiles; its waves are WC = 8 / KW column-waves x KW k-waves, k-wave q takes
//     group j KW + q of step j: K is split INSIDE the workgroup only.
//   * weights: HBM -> VGPRs, four dwordx4 per lane, tile and group (twice INT8's), in a ring w16_ring(TPW)
//     steps deep (the depth is a register decision of its own); with one row block every weight byte is
//     read once per launch, above that the row blocks of a column block sit on one XCD and re-read from its L2.
//   * x: per step the 16 RB x (128 KW) fp16 block goes global -> VGPRs -> LDS (double-buffered, one barrier per
//     step) into the swizzled image of the tile kernels (tile_swz); the A fragment of step s4 is chunk
//     4 kq + s4 (group-128 order), one ds_read_b128 per 16-row block, and each B fragment feeds RB MFMAs.  The
//     only VALU work of the stream is address arithmetic.
//   * after the stream the k-waves' accumulators are summed through LDS in k-wave order (fixed: a second launch
//     gives the same bits; no split-K between workgroups, no tickets, no atomics on sums); the column-waves of
//     k-wave 0 run the staged epilogues of gemm_w8_kernel (gemm_shared.hpp), one tile at a time.
#include <stdlib.h>

#include "gemm_shared.hpp"

namespace ti {

// Weight ring depth (steps): a step holds 16 TPW VGPRs of weights.  4 / 3 keep 12 / 16 KiB of weight loads in
// flight per wave, no instance in scratch (at most 173 VGPRs) and the RB 2 / narrow RB 4 instances within the
// 128 VGPRs at which two workgroups share a CU.  Deeper rings compile without scratch too (TPW 1 at 6 steps: up
// to 192 VGPRs, TPW 2 at 5: 237) and were not measured -- DESIGN 4.33, the resource table.
__host__ __device__ constexpr int w16_ring(int tpw) { return tpw == 1 ? 4 : 3; }
__host__ __device__ constexpr int w16_x_bytes(int rb, int kw) { return 2 * kw * 16 * rb * 256; }
__host__ __device__ constexpr int w16_lds_bytes(int rb, int kw) {
  return w16_x_bytes(rb, kw) > tile_epi_lds_bytes() ? w16_x_bytes(rb, kw) : tile_epi_lds_bytes();
}

template <int RB, int TPW, int KW>
__global__ __launch_bounds__(kGemvThreads, 1) void gemm_w16_kernel(const GemvArgs a, int n_cb, int n_rb) {
  const unsigned long long t_entry = stamp_now();
  constexpr int WC = kGemvWaves / KW, BM = 16 * RB;   // column-waves, rows per workgroup
  constexpr int NX = BM * KW * 16 / kGemvThreads;     // 16-byte pieces of a step's x block per thread
  constexpr int D = w16_ring(TPW);
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
  f16* xb = (f16*)smem;   // [2][KW][BM rows][128 k], 16-byte chunks swizzled by tile_swz(row)

  // ---- x block of step j: global -> xr (rows and groups clamped into the call) -> LDS buffer j & 1
  const f16* xsrc[NX];
  int xdst[NX], xq[NX];
#pragma unroll
  for (int u = 0; u < NX; ++u) {
    const int i = tid + u * kGemvThreads, row = (i >> 4) % BM, c = i & 15;
    xq[u] = i / (BM * 16);
    xsrc[u] = (const f16*)a.x + (size_t)min(m0 + row, a.M - 1) * a.ldx + c * 8;
    xdst[u] = (xq[u] * BM + row) * 128 + ((c ^ tile_swz(row)) * 8);
  }
  u32x4 xr[NX];
  auto load_x = [&](int j) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NX; ++u) xr[u] = *(const u32x4*)(xsrc[u] + min(j * KW + xq[u], KT - 1) * 128);
  };
  auto store_x = [&](int j) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NX; ++u) *(u32x4*)(xb + (j & 1) * (KW * BM * 128) + xdst[u]) = xr[u];
  };

  // ---- the wave's weight tiles (tiles past N clamped, never stored): 4 kWave u32x4 per tile and group
  const u32x4* wt[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) wt[t] = a.tiles + (size_t)min(t0 + wn * TPW + t, NT - 1) * KT * (4 * kWave) + lane;
  u32x4 W[D][TPW][4];
  auto load_w = [&](int slot, int j) __attribute__((always_inline)) {
    const int kg = min(min(j, nsteps - 1) * KW + q, KT - 1);
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) W[slot][t][c] = wt[t][(size_t)kg * (4 * kWave) + c * kWave];
  };

  f32x4 acc[TPW][RB];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int b = 0; b < RB; ++b) acc[t][b] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

  // lane (r, kq): A fragment s4 of row block b = row b 16 + r, k = 32 kq + 8 s4 .. + 7 (chunk 4 kq + s4);
  // B fragment s4 = the lane's chunk s4 of the tile, the same k of output r.  TPW RB accumulator chains.
  auto compute = [&](int slot, int j) __attribute__((always_inline)) {
    const f16* xrow = xb + (j & 1) * (KW * BM * 128) + (q * BM + r) * 128;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      f16x8 xf[RB];
#pragma unroll
      for (int b = 0; b < RB; ++b) xf[b] = *(const f16x8*)(xrow + b * 16 * 128 + (((kq * 4 + s4) ^ tile_swz(r)) * 8));
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const f16x8 bf = __builtin_bit_cast(f16x8, W[slot][t][s4]);
#pragma unroll
        for (int b = 0; b < RB; ++b) acc[t][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xf[b], bf, acc[t][b], 0, 0, 0);
      }
    }
  };

  // ---- the stream.  Step j: x(j + 1) -> registers, W(j + D - 1) -> ring (x first: the wait for x at the
  // step's end then leaves the younger weight loads in flight), compute j from buffer j & 1, x(j + 1) ->
  // buffer (j + 1) & 1 (last read in step j - 1, which every wave left at the previous barrier), barrier.
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
// TI_GEMM_W16_ROWS=0: fp16-weight rows above 16 are refused by ti_gemm_wq_a16 and cut into 16-row fused pieces
// by the engine, as before this kernel (A/B knob, read once per process).
bool w16_rows_on() {
  static const bool on = [] {
    const char* e = getenv("TI_GEMM_W16_ROWS");
    return e ? atoi(e) != 0 : true;
  }();
  return on;
}

// Instances: two tiles per wave only without a k-wave split (TPW 2 with KW k-waves has the column block of TPW 1
// with KW / 2 and a larger slab trip: the plan below never picks it), 8 k-waves only at RB 2 (the LDS image).
#define TI_W16_FNS_RB(RB)                                                                   \
  (const void*)gemm_w16_kernel<RB, 1, 1>, (const void*)gemm_w16_kernel<RB, 1, 2>,           \
      (const void*)gemm_w16_kernel<RB, 1, 4>, (const void*)gemm_w16_kernel<RB, 2, 1>
static const void* const g_w16_fns[] = {TI_W16_FNS_RB(2), TI_W16_FNS_RB(4), (const void*)gemm_w16_kernel<2, 1, 8>};
static const void* w16_fn(int rb, int tpw, int kw) {
  if (kw == 8) return g_w16_fns[8];
  return g_w16_fns[(rb == 4 ? 4 : 0) + (tpw == 2 ? 3 : kw == 1 ? 0 : kw == 2 ? 1 : 2)];
}

// The plan, by the per-CU byte model of w8_plan: RB 2 up to 32 rows, else 4; over tiles per wave TPW in {1, 2}
// and k-waves KW in {1, 2, 4, 8 (RB 2)} with KW <= K / 128, the launch takes ceil(workgroups of an XCD / its
// CUs) rounds, a workgroup moves per 128-k group its x rows (16 RB x 256 B) and its (8 / KW) TPW tiles of
// 4 KiB, and a k-wave split adds its slabs' trip through LDS once; the cheapest shape wins, ties to fewer
// k-waves and then to more tiles per wave.  (TPW 2 with KW > 1 always loses that comparison to TPW 1 with
// KW / 2, which has the same column block: not a candidate, not instantiated.)
W16Plan w16_plan(int M, int N, int K, int cus) {
  const int NT = N >> 4, KT = K >> 7, rb = M <= 32 ? 2 : 4, bm = 16 * rb;
  const int n_rb = (M + bm - 1) / bm, xcd_cus = cus >= 8 ? cus / 8 : 1;
  W16Plan best{};
  long best_cost = -1;
  for (int kw : {1, 2, 4, 8}) {
    if (kw > KT || rb * kw > 16) continue;
    for (int tpw : {2, 1}) {
      if (tpw == 2 && kw > 1) continue;
      const int cols = (8 / kw) * tpw, n_cb = (NT + cols - 1) / cols;
      const long per_xcd = (long)(n_cb + 7) / 8 * n_rb, rounds = (per_xcd + xcd_cus - 1) / xcd_cus;
      const long cost = rounds * ((long)KT * (bm * 256 + cols * 4096) + (kw > 1 ? (long)(kw - 1) * cols * rb * 1024 : 0));
      if (best_cost < 0 || cost < best_cost) {
        best_cost = cost;
        best.rb = rb; best.tpw = tpw; best.kw = kw; best.n_cb = n_cb; best.n_rb = n_rb;
        best.grid = (n_cb + 7) / 8 * 8 * n_rb;
        best.lds = w16_lds_bytes(rb, kw);
      }
    }
  }
  return best;
}

int w16_prepare() {
  for (const void* f : g_w16_fns)
    TI_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                 "hipFuncSetAttribute(gemm_w16_kernel)");
  return TI_OK;
}

int launch_w16(const GemvArgs& a, const W16Plan& p, hipStream_t s) {
  GemvArgs args = a;
  int n_cb = p.n_cb, n_rb = p.n_rb;
  void* kargs[] = {&args, &n_cb, &n_rb};
  TI_HIP_CHECK(hipLaunchKernel(w16_fn(p.rb, p.tpw, p.kw), dim3(p.grid), dim3(kGemvThreads), kargs, p.lds, s),
               "hipLaunchKernel(gemm_w16_kernel)");
  TI_LAUNCH_CHECK("gemm_w16_kernel");
  return TI_OK;
}

}  // namespace ti
