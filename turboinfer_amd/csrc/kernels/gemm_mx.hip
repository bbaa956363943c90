// gemm_mx.hip -- MXFP4 weights (OCP e2m1 blocks of 32 with one e8m0 scale, bits 4 | TI_BITS_G32 | TI_BITS_MX) x fp16
// rows on MFMA for 17 .. TI_GEMM_MAX_ROWS rows (gfx950): batched decode above 16 streams and prompt chunks of MX
// engines (ti_gemm_wq_a16 with TI_X_F16 rows, M >= 17, once ti_gemm_set_mx_rows / TI_GEMM_MX_ROWS turned the route
// on).  The fused gemv_mx_kernel stays the MX kernel up to 16 rows, and above them while the route is off.
//
// y[M][N] = x[M][K] . W, W = 2^(e - 127) v per 32-weight block, in the tiles and scale bytes of ti_wpack_mx_host as
// they are: a tile is 16 outputs x 128 k in 1 KiB, lane l = 16 kq + r holds one dwordx4 whose word s4 is
// k = 32 s4 + 8 kq + e of output r (element 2p at bits 4p, element 2p + 1 at bits 16 + 4p, the nibble the raw e2m1
// code); the 64 e8m0 bytes of a tile and group are [block s4][output], i.e. the scale of (s4, r) is byte r & 3 of
// dword 4 s4 + (r >> 2).  The arithmetic is the fused kernel's: one v_mfma_f32_16x16x32_f16 from zero sums x v over
// one block (v widened exactly by deq_mxfp4), then acc = fmaf(bit_cast<float>(e << 23), block_sum, acc) per block in
// k order.  The block scale is not folded into the conversion: with e down to 100 the product leaves fp16's range.
//
// Shape of the work (the fourth sibling of gemm_w8_kernel / gemm_w16_kernel / gemm_w4a_kernel; the stream differs):
//   * a workgroup of 8 waves owns one row block of 16 RB rows (RB 2: at most 32 rows, else 4) and one column block
//     of WC TPW tiles; its waves are WC = 8 / KW column-waves x KW k-waves, k-wave q takes group j KW + q of step
//     j: K is split INSIDE the workgroup only.
//   * weights: HBM -> VGPRs, per lane, tile and group one dwordx4 of nibbles and one 4-byte load of dword lane & 15
//     of the tile's 64 scale bytes (every dword arrives four times over the wave: one coalesced 64-byte request,
//     no byte loads in the ring), in a ring mx_ring(TPW) steps deep.
//   * nothing else per block: no block sums of x, no minimums, no correction table, no pre-scaled x slots.  The x
//     image is the family's plain swizzled fp16 image (tile_swz), double-buffered, one barrier per step; the A
//     fragment of block s4 is chunk 4 s4 + kq.  The dynamic LDS is that image alone (or the epilogue staging).
//   * the scale of (block s4, output r) reaches lane (r, kq) from lane 4 s4 + (r >> 2), which loaded its dword:
//     one ds_bpermute per block and tile, then a shift by 8 (r & 3) and the move into the exponent field.
//   * the TPW x 4 (block, tile) units run as one software pipeline: the bpermute, the conversion and the MFMAs of
//     unit u + 1 ahead of the FMAs of unit u.
//   * after the stream the k-waves' accumulators are summed through LDS in k-wave order (fixed: a second launch
//     gives the same bits; no split-K between workgroups, no tickets, no atomics on sums); the column-waves of
//     k-wave 0 run the staged epilogues of gemm_shared.hpp, one tile at a time.
#include <stdlib.h>

#include <atomic>

#include "gemm_shared.hpp"

namespace ti {

// Weight ring depth (steps): a step holds 5 TPW VGPRs (4 of nibbles, one of scale bytes).  Without Q4_1's block
// sums and minimum terms the kernel has the registers for one step more than gemm_w4a_kernel's 7 / 5: 8 / 6 keep
// 7.4 / 10.6 KiB of weight loads in flight per wave with no instance in scratch -- DESIGN 4.36, the resource
// table.  The depth is a register decision; no depth was measured against another.
__host__ __device__ constexpr int mx_ring(int tpw) { return tpw == 1 ? 8 : 6; }
__host__ __device__ constexpr int mx_x_bytes(int rb, int kw) { return 2 * kw * 16 * rb * 256; }
__host__ __device__ constexpr int mx_lds_bytes(int rb, int kw) {
  return mx_x_bytes(rb, kw) > tile_epi_lds_bytes() ? mx_x_bytes(rb, kw) : tile_epi_lds_bytes();
}

template <int RB, int TPW, int KW>
__global__ __launch_bounds__(kGemvThreads, 1) void gemm_mx_kernel(const GemvArgs a, int n_cb, int n_rb) {
  const unsigned long long t_entry = stamp_now();
  constexpr int WC = kGemvWaves / KW, BM = 16 * RB;   // column-waves, rows per workgroup
  constexpr int NX = BM * KW * 16 / kGemvThreads;     // 16-byte pieces of a step's x block per thread
  constexpr int D = mx_ring(TPW);
  constexpr int XB = KW * BM * 128;                   // elements of one x buffer
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
    for (int u = 0; u < NX; ++u) *(u32x4*)(xb + (j & 1) * XB + xdst[u]) = xr[u];
  };

  // ---- the wave's weight tiles and scale bytes (tiles past N clamped, never stored): per tile and group kWave
  // u32x4 of nibbles and 64 e8m0 bytes [block s4][output] = 16 dwords, lane l loads dword l & 15
  const u32x4* wt[TPW];
  const uint32_t* st[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tn = min(t0 + wn * TPW + t, NT - 1);
    wt[t] = a.tiles + (size_t)tn * KT * kWave + lane;
    st[t] = (const uint32_t*)((const uint8_t*)a.scales + (size_t)tn * KT * 64) + (lane & 15);
  }
  u32x4 W[D][TPW];
  uint32_t S[D][TPW];
  auto load_w = [&](int slot, int j) __attribute__((always_inline)) {
    const int kg = min(min(j, nsteps - 1) * KW + q, KT - 1);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      W[slot][t] = wt[t][(size_t)kg * kWave];
      S[slot][t] = st[t][kg * 16];
    }
  };

  f32x4 acc[TPW][RB];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int b = 0; b < RB; ++b) acc[t][b] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

  // lane (r, kq): A fragment of block s4 and row block b = row b 16 + r, chunk 4 s4 + kq (k = 32 s4 + 8 kq .. + 7);
  // B fragment = the lane's word s4 of the tile, the same k of output r: one MFMA from zero is the block's sum of
  // x v for rows b 16 + 4 kq .. + 3 (C layout).  Unit u is block s4 = u / TPW of tile t = u % TPW; only two units'
  // sums (2 RB f32x4) and scales are live beside the accumulators.
  const int ssrc = 4 * (r >> 2), ssh = 8 * (r & 3);   // (byte address of source lane r >> 2 of block 0; the byte's shift)
  auto compute = [&](int slot, int j) __attribute__((always_inline)) {
    const f16* xrow = xb + (j & 1) * XB + (q * BM + r) * 128;
    constexpr int NU = 4 * TPW;
    f16x8 xf[RB];
    f32x4 sum[2][RB];
    float d[2];
    auto mfmas = [&](int u) __attribute__((always_inline)) {
      const int s4 = u / TPW, t = u % TPW;
      if (t == 0) {
#pragma unroll
        for (int b = 0; b < RB; ++b) xf[b] = *(const f16x8*)(xrow + b * 16 * 128 + (((s4 * 4 + kq) ^ tile_swz(r)) * 8));
      }
      const uint32_t sw = (uint32_t)__builtin_amdgcn_ds_bpermute(ssrc + 16 * s4, (int)S[slot][t]);
      d[u & 1] = e8m0_to_f32((sw >> ssh) & 0xffu);
      const f16x8 bf = deq_mxfp4(W[slot][t][s4]);
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
        for (int i = 0; i < 4; ++i) acc[u % TPW][b][i] = fmaf(d[u & 1], sum[u & 1][b][i], acc[u % TPW][b][i]);
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
// The route's process-wide switch (ti_gemm_set_mx_rows): off unless TI_GEMM_MX_ROWS (read once) or a
// call turns it on.  While it is off MX rows above 16 are cut into 16-row fused pieces by ti_gemm_wq_a16 and by
// the engine, as before this kernel.
static std::atomic<int>& mx_rows_flag() {
  static std::atomic<int> on{[] {
    const char* e = getenv("TI_GEMM_MX_ROWS");
    return e && atoi(e) != 0 ? 1 : 0;
  }()};
  return on;
}
bool mx_rows_on() { return mx_rows_flag().load(std::memory_order_relaxed) != 0; }
int mx_rows_set(int on) { return mx_rows_flag().exchange(on ? 1 : 0, std::memory_order_relaxed); }

// Instances: gemm_w4a_kernel's nine -- two tiles per wave only without a k-wave split (TPW 2 with KW k-waves has the
// column block of TPW 1 with KW / 2 and a larger slab trip: the plan below never picks it), 8 k-waves only at RB 2
// (the LDS image).
#define TI_MX_FNS_RB(RB)                                                                  \
  (const void*)gemm_mx_kernel<RB, 1, 1>, (const void*)gemm_mx_kernel<RB, 1, 2>,           \
      (const void*)gemm_mx_kernel<RB, 1, 4>, (const void*)gemm_mx_kernel<RB, 2, 1>
static const void* const g_mx_fns[] = {TI_MX_FNS_RB(2), TI_MX_FNS_RB(4), (const void*)gemm_mx_kernel<2, 1, 8>};
static const void* mx_fn(int rb, int tpw, int kw) {
  if (kw == 8) return g_mx_fns[8];
  return g_mx_fns[(rb == 4 ? 4 : 0) + (tpw == 2 ? 3 : kw == 1 ? 0 : kw == 2 ? 1 : 2)];
}

// The plan: w8_plan's per-CU byte model with 1024 + 64 B per tile and group (nibbles and scale bytes).  RB 2 up to
// 32 rows, else 4; over tiles per wave TPW in {1, 2} and k-waves KW in {1, 2, 4, 8 (RB 2)} with KW <= K / 128, the
// launch takes ceil(workgroups of an XCD / its CUs) rounds, a workgroup moves per 128-k group its x rows
// (16 RB x 256 B) and its (8 / KW) TPW tiles, and a k-wave split adds its slabs' trip through LDS once; the
// cheapest shape wins, ties to fewer k-waves and then to more tiles per wave.  (TPW 2 with KW > 1 always loses that
// comparison to TPW 1 with KW / 2, which has the same column block: not a candidate, not instantiated.)
MxPlan mx_plan(int M, int N, int K, int cus) {
  const int NT = N >> 4, KT = K >> 7, rb = M <= 32 ? 2 : 4, bm = 16 * rb;
  const int n_rb = (M + bm - 1) / bm, xcd_cus = cus >= 8 ? cus / 8 : 1;
  MxPlan best{};
  long best_cost = -1;
  for (int kw : {1, 2, 4, 8}) {
    if (kw > KT || rb * kw > 16) continue;
    for (int tpw : {2, 1}) {
      if (tpw == 2 && kw > 1) continue;
      const int cols = (8 / kw) * tpw, n_cb = (NT + cols - 1) / cols;
      const long per_xcd = (long)(n_cb + 7) / 8 * n_rb, rounds = (per_xcd + xcd_cus - 1) / xcd_cus;
      const long cost = rounds * ((long)KT * (bm * 256 + cols * 1088) + (kw > 1 ? (long)(kw - 1) * cols * rb * 1024 : 0));
      if (best_cost < 0 || cost < best_cost) {
        best_cost = cost;
        best.rb = rb; best.tpw = tpw; best.kw = kw; best.n_cb = n_cb; best.n_rb = n_rb;
        best.grid = (n_cb + 7) / 8 * 8 * n_rb;
        best.lds = mx_lds_bytes(rb, kw);
      }
    }
  }
  return best;
}

int mx_prepare() {
  for (const void* f : g_mx_fns)
    TI_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                 "hipFuncSetAttribute(gemm_mx_kernel)");
  return TI_OK;
}

int launch_mx(const GemvArgs& a, const MxPlan& p, hipStream_t s) {
  GemvArgs args = a;
  int n_cb = p.n_cb, n_rb = p.n_rb;
  void* kargs[] = {&args, &n_cb, &n_rb};
  TI_HIP_CHECK(hipLaunchKernel(mx_fn(p.rb, p.tpw, p.kw), dim3(p.grid), dim3(kGemvThreads), kargs, p.lds, s),
               "hipLaunchKernel(gemm_mx_kernel)");
  TI_LAUNCH_CHECK("gemm_mx_kernel");
  return TI_OK;
}

}  // namespace ti
