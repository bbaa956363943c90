// gemm_w8.hip -- INT8 weights (group-128, and group-32 Q8_0 blocks) x fp16 rows on MFMA for 17 ..
// TI_GEMM_MAX_ROWS rows (gfx950): batched decode above 16 streams and prompt chunks of INT8 engines
// (ti_gemm_wq_a16 with bits 8 or 8 | TI_BITS_G32, TI_X_F16 rows, M >= 17).  The fused
// gemv_wq_kernel stays the INT8 kernel up to 16 rows.  Group-128 first:
//
// y[M][N] = x[M][K] . W with W in the INT8 tiles and fp16 group scales of ti_wpack_host(.., 8): a tile is
// 16 outputs x 128 k (2 KiB, two 1 KiB chunks; lane l of chunk c: 16 bytes of output l & 15 from
// k = 32 (l >> 4) + 16 c), scales [N/16][K/128][16].  The arithmetic is the fused kernel's (dequant.hpp,
// dequant_step<8>): bytes widen exactly to fp16, v_mfma_f32_16x16x32_f16 sums one 128-k group in fp32 from
// zero, acc = fmaf(scale, group_sum, acc).
//
// Shape of the work:
//   * a workgroup of 8 waves owns one row block of 16 RB rows (RB 2: at most 32 rows, else 4) and one
//     column block of WC TPW tiles; its waves are WC = 8 / KW column-waves x KW k-waves.  Step j covers
//     the KW consecutive groups j KW .. j KW + KW - 1, k-wave q takes group j KW + q: narrow outputs
//     (TinyLlama's O and down: 128 tiles) still fill the chip, K being split INSIDE the workgroup.
//   * weights: HBM -> VGPRs, two dwordx4 per lane, tile and group, in a ring 4 steps deep (3 at TPW 2); with one
//     row block (M <= 64) every weight byte is read once per launch, above that the row blocks of a column
//     block sit next to each other on one XCD and re-read the tiles from its L2.
//   * x: per step the 16 RB x (128 KW) fp16 block goes global -> VGPRs -> LDS (double-buffered, one
//     barrier per step) into the swizzled image the int4 tile kernel uses (tile_swz: conflict-free
//     ds_read_b128 A fragments); each dequantised B fragment feeds RB MFMAs.
//   * after the stream the k-waves' fp32 accumulators are summed through LDS in k-wave order (fixed, so
//     the result is bit-reproducible: no split-K between workgroups, no tickets, no atomics on the sums);
//     the column-waves of k-wave 0 run the staged epilogue (tile_epilogue_lds; STORE_F16 and
//     LOGITS_ARGMAX are staged the same way here).
//
// G32 instances (bits 8 | TI_BITS_G32, GGUF Q8_0 blocks): the same work split on group-32 tiles
// (lane l's bytes 8 s4 .. + 7 are k = 32 s4 + 8 (l >> 4) .. + 7, scales [N/16][K/128][4][16]).  One MFMA from
// zero sums one 32-k block and acc = fmaf(block scale, block sum, acc) runs per block in k order, the fused
// kernel's group-32 arithmetic.  The 64 scales of a tile and group ride in the ring as one coalesced 2-byte
// load per lane; a ds_bpermute per block hands lane (r, kq) the scale of (block, output r).  See compute32.
#include <stdlib.h>

#include "gemm_shared.hpp"

namespace ti {

constexpr int w8_ring(int tpw) { return tpw == 1 ? 4 : 3; }   // weight ring depth (steps)
__host__ __device__ constexpr int w8_x_bytes(int rb, int kw) { return 2 * kw * 16 * rb * 256; }
__host__ __device__ constexpr int w8_lds_bytes(int rb, int kw) {
  return w8_x_bytes(rb, kw) > tile_epi_lds_bytes() ? w8_x_bytes(rb, kw) : tile_epi_lds_bytes();
}

template <int RB, int TPW, int KW, bool G32 = false>
__global__ __launch_bounds__(kGemvThreads, 1) void gemm_w8_kernel(const GemvArgs a, int n_cb, int n_rb) {
  const unsigned long long t_entry = stamp_now();
  constexpr int WC = kGemvWaves / KW, BM = 16 * RB;   // column-waves, rows per workgroup
  constexpr int NX = BM * KW * 16 / kGemvThreads;     // 16-byte pieces of a step's x block per thread
  constexpr int D = w8_ring(TPW);
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

  // ---- the wave's weight tiles and scales (tiles past N clamped, never stored)
  const u32x4* wt[TPW];
  const uint16_t* st[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tn = min(t0 + wn * TPW + t, NT - 1);
    wt[t] = a.tiles + (size_t)tn * KT * (2 * kWave) + lane;
    // group-32: the 64 scales of a tile and group are [block s4][output], lane l loads entry l
    st[t] = a.scales + (size_t)tn * KT * (G32 ? 64 : 16) + (G32 ? lane : r);
  }
  u32x4 W[D][TPW][2];
  uint16_t S[D][TPW];
  auto load_w = [&](int slot, int j) __attribute__((always_inline)) {
    const int kg = min(min(j, nsteps - 1) * KW + q, KT - 1);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      W[slot][t][0] = wt[t][(size_t)kg * (2 * kWave)];
      W[slot][t][1] = wt[t][(size_t)kg * (2 * kWave) + kWave];
      S[slot][t] = st[t][kg * (G32 ? 64 : 16)];
    }
  };

  f32x4 acc[TPW][RB];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int b = 0; b < RB; ++b) acc[t][b] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

  // lane (r, kq): A fragment s4 of row block b = row b 16 + r, k = 32 kq + 8 s4 .. + 7 (chunk 4 kq + s4);
  // B fragment s4 = the lane's bytes 8 s4 .. + 7 of the tile row r, the same k
  auto compute128 = [&](int slot, int j) __attribute__((always_inline)) {
    const f16* xrow = xb + (j & 1) * (KW * BM * 128) + (q * BM + r) * 128;
    f32x4 tmp[TPW][RB];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int b = 0; b < RB; ++b) tmp[t][b] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      f16x8 xf[RB];
#pragma unroll
      for (int b = 0; b < RB; ++b) xf[b] = *(const f16x8*)(xrow + b * 16 * 128 + (((kq * 4 + s4) ^ tile_swz(r)) * 8));
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const f16x8 bf = dequant_step<8>(W[slot][t], s4, 0u);
#pragma unroll
        for (int b = 0; b < RB; ++b) tmp[t][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xf[b], bf, tmp[t][b], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const float sc = h2f(S[slot][t]);
#pragma unroll
      for (int b = 0; b < RB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[t][b][i] = fmaf(sc, tmp[t][b][i], acc[t][b][i]);
    }
  };

  // Group-32 tiles (Q8_0 blocks): the lane's bytes 8 s4 .. + 7 are k = 32 s4 + 8 kq .. + 7, so the A fragment
  // of step s4 is chunk 4 s4 + kq and one MFMA from zero is one block's sum; acc = fmaf(scale(block s4,
  // output r), sum, acc) for s4 = 0 .. 3 in that order (gemv_body<8, .., G32>).  Lane 16 s4 + r loaded that
  // scale (load_w): one ds_bpermute per block and tile hands it to the four lanes (r, kq).  The TPW x 4
  // (block, tile) units run as one software pipeline, the MFMAs of unit u + 1 ahead of the FMAs of unit
  // u, so only two units' sums (2 RB f32x4) are live beside the accumulators.
  auto compute32 = [&](int slot, int j) __attribute__((always_inline)) {
    const f16* xrow = xb + (j & 1) * (KW * BM * 128) + (q * BM + r) * 128;
    constexpr int NU = 4 * TPW;   // unit u: block s4 = u / TPW of tile t = u % TPW
    float sc[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u)
      sc[u] = h2f((uint16_t)__builtin_amdgcn_ds_bpermute(4 * (16 * (u / TPW) + r), (int)S[slot][u % TPW]));
    f16x8 xf[RB];
    f32x4 sum[2][RB];
    auto mfmas = [&](int u) __attribute__((always_inline)) {
      const int s4 = u / TPW, t = u % TPW;
      if (t == 0) {
#pragma unroll
        for (int b = 0; b < RB; ++b) xf[b] = *(const f16x8*)(xrow + b * 16 * 128 + (((s4 * 4 + kq) ^ tile_swz(r)) * 8));
      }
      const f16x8 bf = dequant_step<8>(W[slot][t], s4, 0u);
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
        for (int i = 0; i < 4; ++i) acc[u % TPW][b][i] = fmaf(sc[u], sum[u & 1][b][i], acc[u % TPW][b][i]);
    }
  };
  auto compute = [&](int slot, int j) __attribute__((always_inline)) {
    if constexpr (G32) compute32(slot, j);
    else compute128(slot, j);
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
// TI_GEMM_W8_ROWS=0: INT8 rows above 16 are refused by ti_gemm_wq_a16 (group-32: cut into 16-row fused pieces
// there) and cut into 16-row fused pieces by the engine, as before this kernel (A/B knob, read once per
// process).
bool w8_rows_on() {
  static const bool on = [] {
    const char* e = getenv("TI_GEMM_W8_ROWS");
    return e ? atoi(e) != 0 : true;
  }();
  return on;
}

#define TI_W8_FNS_RB(RB, G)                                                                           \
  (const void*)gemm_w8_kernel<RB, 1, 1, G>, (const void*)gemm_w8_kernel<RB, 1, 2, G>,                  \
      (const void*)gemm_w8_kernel<RB, 1, 4, G>, (const void*)gemm_w8_kernel<RB, 2, 1, G>,              \
      (const void*)gemm_w8_kernel<RB, 2, 2, G>, (const void*)gemm_w8_kernel<RB, 2, 4, G>
#define TI_W8_FNS(G)                                                                        \
  TI_W8_FNS_RB(2, G), TI_W8_FNS_RB(4, G), (const void*)gemm_w8_kernel<2, 1, 8, G>,          \
      (const void*)gemm_w8_kernel<2, 2, 8, G>
static const void* const g_w8_fns[] = {TI_W8_FNS(false), TI_W8_FNS(true)};   // 14 group-128, 14 group-32
static const void* w8_fn(int rb, int tpw, int kw, bool g32) {
  const int i = kw == 8 ? 12 + tpw - 1 : (rb == 4 ? 6 : 0) + (tpw - 1) * 3 + (kw == 1 ? 0 : kw == 2 ? 1 : 2);
  return g_w8_fns[(g32 ? 14 : 0) + i];
}

// The plan, by a per-CU byte model (as tile_shape): RB 2 up to 32 rows, else 4; over tiles per wave TPW in
// {1, 2} and k-waves KW in {1, 2, 4, 8 (RB 2)} with KW <= K / 128, the launch takes
// ceil(workgroups of an XCD / its CUs) rounds, a workgroup moves per 128-k group its x rows (16 RB x 256 B)
// and its (8 / KW) TPW tiles of 2 KiB (group-32: + 128 B of block scales each), and a k-wave split adds its
// slabs' trip through LDS once; the cheapest shape wins, ties to fewer k-waves and then to more tiles per
// wave.  Every (RB, TPW, KW) is a candidate for both group sizes: no group-32 instance uses scratch.
W8Plan w8_plan(int M, int N, int K, int cus, bool g32) {
  const int NT = N >> 4, KT = K >> 7, rb = M <= 32 ? 2 : 4, bm = 16 * rb;
  const int n_rb = (M + bm - 1) / bm, xcd_cus = cus >= 8 ? cus / 8 : 1;
  const int tile_bytes = 2048 + (g32 ? 128 : 0);   // (the 32 B of group-128 scales were never counted)
  W8Plan best{};
  best.g32 = g32;
  long best_cost = -1;
  for (int kw : {1, 2, 4, 8}) {
    if (kw > KT || rb * kw > 16) continue;
    for (int tpw : {2, 1}) {
      const int cols = (8 / kw) * tpw, n_cb = (NT + cols - 1) / cols;
      const long per_xcd = (long)(n_cb + 7) / 8 * n_rb, rounds = (per_xcd + xcd_cus - 1) / xcd_cus;
      const long cost = rounds * ((long)KT * (bm * 256 + cols * tile_bytes) + (kw > 1 ? (long)(kw - 1) * cols * rb * 1024 : 0));
      if (best_cost < 0 || cost < best_cost) {
        best_cost = cost;
        best.rb = rb; best.tpw = tpw; best.kw = kw; best.n_cb = n_cb; best.n_rb = n_rb;
        best.grid = (n_cb + 7) / 8 * 8 * n_rb;
        best.lds = w8_lds_bytes(rb, kw);
      }
    }
  }
  return best;
}

int w8_prepare() {
  for (const void* f : g_w8_fns)
    TI_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                 "hipFuncSetAttribute(gemm_w8_kernel)");
  return TI_OK;
}

int launch_w8(const GemvArgs& a, const W8Plan& p, hipStream_t s) {
  GemvArgs args = a;
  int n_cb = p.n_cb, n_rb = p.n_rb;
  void* kargs[] = {&args, &n_cb, &n_rb};
  TI_HIP_CHECK(hipLaunchKernel(w8_fn(p.rb, p.tpw, p.kw, p.g32),dim3(p.grid), dim3(kGemvThreads), kargs, p.lds, s),
               "hipLaunchKernel(gemm_w8_kernel)");
  TI_LAUNCH_CHECK("gemm_w8_kernel");
  return TI_OK;
}

}  // namespace ti
