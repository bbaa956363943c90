// gemv_wq_body.inc -- the body of gemv_wq_kernel / gemv_mx_kernel / gemv_kq_kernel (gemv.hip, which documents it): included inside
// a function that has BITS, XM, G32, AFF, EPI, MX, KQ as compile-time constants and the kernel's parameters.
  const unsigned long long t_entry = stamp_now();
  const unsigned bid = blockIdx.x;
  a.tiles = p_tiles;
  a.scales = p_scales;
  a.x = p_x;
  a.norm_w = p_aux;
  a.M = p_mgk & 63;
  // p_N = q | r << 8: NT = q * grid + r 16-row tiles, workgroup b takes q (+1 for b < r) of them from
  // t0 = b q + min(b, r) (scalar arithmetic only; launch_gemv packs it)
  const int nt_q = p_N & 0xff, nt_r = (int)((unsigned)p_N >> 8);
  a.K = p_kx & 0xffff;
  a.ldx = XM == XM_F16F || XM == XM_ATTN ? a.K : (int)((unsigned)p_kx >> 16);
  const int p_grid = (p_mgk >> 6) & 0xfff;
  a.N = 16 * (nt_q * p_grid + nt_r);
  constexpr int C = TileFmt<BITS>::kChunks;
  constexpr int R = TI_GEMV_RING_VGPRS / (4 * C) > 2 ? TI_GEMV_RING_VGPRS / (4 * C) : 2;   // ring depth (items)
  constexpr int XPF = 3;                           // fp16 x: 16-byte pieces prefetched per thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  GEMV_TS(0);
  const int KT = a.K >> 7, xs = a.K + 8, NT = a.N >> 4, K8 = a.K >> 3;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: counters live in SGPRs
  const int t0 = (int)bid * nt_q + ((int)bid < nt_r ? (int)bid : nt_r);
  const int ntl = nt_q + ((int)bid < nt_r ? 1 : 0);
  constexpr bool kOneRow = XM == XM_F16F || XM == XM_ATTN || XM == XM_NORM1;   // (M == 1 by construction)
  const int KW = wave < KT ? (KT - wave + kGemvWaves - 1) / kGemvWaves : 0;   // k-tiles per tile, this wave
  const int total = ntl * KW;
  static_assert(!G32 || BITS != 16, "group-32 weights: int4 / int8");
  static_assert(!AFF || (G32 && BITS == 4), "affine blocks: group-32 int4");
  static_assert(!MX || (G32 && BITS == 4 && !AFF), "MXFP4 blocks: group-32 nibbles");
  static_assert(!KQ || (G32 && BITS == 4 && !AFF && !MX && XM != XM_F16F), "Q4_K super-blocks: group-32 nibbles");
  const GemvLds L = KQ ? gemv_lds_layout_kq(a.M, a.K, ntl)
                    : MX ? gemv_lds_layout_mx(a.M, a.K, ntl) : gemv_lds_layout(a.M, a.K, ntl, G32, AFF);
  uint16_t* ml = (uint16_t*)(smem + L.mins);       // AFF: block minimums, as sl; KQ: the d | dmin words
  float* bsum = (float*)(smem + L.bsum);           // AFF, KQ: [K/32][16] sums of x per block and row
  f16* xl = (f16*)(smem + L.x);
  uint16_t* sl = (uint16_t*)(smem + L.sc);
  float* corr = (float*)(smem + L.corr);           // [K/128][16] (int4 only)
  f32x4* slab = (f32x4*)(smem + L.slab);           // [ntl + 1][8][64]
  float* es = (float*)(smem + L.es);
  unsigned long long* best_l = (unsigned long long*)(smem + L.best);
  float* red = (float*)(smem + L.slab);            // norm reduction scratch (before the stream)

  // ---- 1. small inputs into registers, ahead of the ring
  const int n_sc = BITS == 16 ? 0 : ntl * KT * (MX ? 4 : G32 ? 8 : 2);  // u32x4 pieces of scales
  const u32x4* sg = (const u32x4*)(a.scales + (size_t)t0 * KT * (MX ? 32 : G32 ? 64 : 16));
  u32x4 sc_reg = {0u, 0u, 0u, 0u};
#if TI_GEMV_EXP & 8   // diagnostic: no dependency on x / scales (constants instead of loads)
  const int nx16 = a.M * K8;
  float4 v0 = {1.0f, 1.0f, 1.0f, 1.0f}, v1 = v0, w0 = v0, w1 = v0;
  u32x4 xr16[XPF];
  for (int q = 0; q < XPF; ++q) xr16[q] = (u32x4){0x3c003c00u, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u};
  sc_reg = xr16[0];
  auto load_x = [&]() {};
  if (false) {
#else
  if constexpr (BITS != 16) sc_reg = ld_w(sg + (tid < n_sc ? tid : 0));

  const int nx16 = a.M * K8;
  float4 v0, v1, w0, w1;
  u32x4 xr16[XPF];
  // x rows and the epilogue input depend on the previous launch
  // XM_ATTN: this thread's 8 dims (one head) of every split, and the splits' (max, sum)
  constexpr int kPS = TI_ATTN_MAX_PART_SPLITS;
  u32x4 po[XM == XM_ATTN ? kPS : 1];
  float2 pml[XM == XM_ATTN ? kPS : 1];
  auto load_x = [&]() {
    if constexpr (XM == XM_ATTN) {
      const int S = (int)((unsigned)p_kx >> 16), hsh = ((p_mgk >> 21) & 3) == 2 ? 7 : 6;
      const int i = tid < K8 ? tid : K8 - 1, h = (8 * i) >> hsh, d = (8 * i) & ((1 << hsh) - 1);
#pragma unroll
      for (int sp = 0; sp < kPS; ++sp) {
        const int r = h * S + (sp < S ? sp : S - 1);
        po[sp] = *(const u32x4*)((const f16*)a.x + ((size_t)r << hsh) + d);
        pml[sp] = *(const float2*)(p_aux + 2 * r);
      }
    } else if constexpr (XM == XM_NORM1) {
      const int k8 = tid < K8 ? tid : K8 - 1;
      const float* xr = (const float*)a.x;
      v0 = *(const float4*)(xr + 8 * k8);
      v1 = *(const float4*)(xr + 8 * k8 + 4);
    } else if constexpr (XM == XM_F16 || XM == XM_F16F) {
#pragma unroll
      for (int q = 0; q < XPF; ++q) {
        const int i = tid + q * kGemvThreads < nx16 ? tid + q * kGemvThreads : nx16 - 1;
        const int m = kOneRow ? 0 : i / K8, k8 = i - m * K8;
        xr16[q] = *(const u32x4*)((const f16*)a.x + (size_t)m * a.ldx + 8 * k8);
      }
    }
  };
  if constexpr (XM == XM_NORM1) {
#endif
    const int k8 = tid < K8 ? tid : K8 - 1;
    w0 = *(const float4*)(a.norm_w + 8 * k8);
    w1 = *(const float4*)(a.norm_w + 8 * k8 + 4);
  }
  load_x();
  // Epilogue input, one word per thread, loaded unconditionally (a branch here would make
  // the compiler wait at the join): a residual element of our tiles, this step's position
  // of row tid, or a dummy word of x.
  // (p_pre / kind / ldo are preloaded: epi.out for RESID, epi.pos for QKV, else x)
  const int kind = EPI >= 0 ? EPI : (p_mgk >> 18) & 7, ldo = p_ldo;
  const int n_res = kind == TI_EPI_RESID_F32 ? ntl * a.M * 16 : 0;
  const float* pre_p;
  {
    const int idx = tid < n_res ? tid : 0;
    const int tl = kOneRow || EPI >= 0 ? idx >> 4 : idx / (a.M * 16), rem = idx - tl * a.M * 16, m = rem >> 4, n = rem & 15;
    pre_p = kind == TI_EPI_RESID_F32 ? p_pre + (size_t)m * ldo + (t0 + tl) * 16 + n
            : kind == TI_EPI_QKV_ROPE_KV ? p_pre + (tid < a.M ? tid : 0) : p_pre;
  }
  const float pre = *pre_p;
  // RESID with fold_x: the fold weight of the same output (one row), consumed by the epilogue
  // (its pointer comes from the kernarg struct: loaded after the ring is issued, below)
  float fw_pre = 0.0f;
  // XM_F16F: this lane's share of the producer's partial sums of squares (up to 256 of them),
  // clamped loads; masked and summed after the stream
  float ss4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const int n_ss = (int)((unsigned)p_kx >> 16);
  if constexpr (XM == XM_F16F) {
#pragma unroll
    for (int j = 0; j < 4; ++j) ss4[j] = p_aux[lane + 64 * j < n_ss ? lane + 64 * j : 0];
  }

  // ---- 2. the weight ring.  Item j of this wave = (tile j / KW, k-tile wave + 8 * (j % KW));
  // items past the end re-load the last item (no branch around loads); coordinates advance
  // by counters (no integer division in the stream).
  const u32x4* tb = a.tiles + (size_t)t0 * KT * (kWave * C) + lane;
  const size_t last_off = total > 0 ? ((size_t)(ntl - 1) * KT + wave + kGemvWaves * (KW - 1)) * (kWave * C) : 0;
  int rt = 0, rk = 0, rj = 0;                      // refill cursor: tile, k index, item
  auto refill_off = [&]() -> size_t {
    const size_t o = rj < total ? ((size_t)rt * KT + wave + kGemvWaves * rk) * (kWave * C) : last_off;
    ++rj;
    if (++rk == KW) { rk = 0; ++rt; }
    return o;
  };
  // Only the first R0 slots go out before the staging barrier: a CU's memory pipe accepts a
  // limited number of outstanding loads, so a wave issuing all R slots blocks in issue for
  // microseconds, and the barrier (hence the first MFMA) would wait for the slowest wave's
  // whole burst.  The rest of the ring is issued right after the barrier.
  constexpr int R0 = R >= 8 ? 4 : R;
  u32x4 ring[R][C];
#if TI_GEMV_RING_DELAY > 0   // A/B knob: hold the ring back (x 64 clocks) behind the small loads
  __builtin_amdgcn_s_sleep(TI_GEMV_RING_DELAY);
#endif
#pragma unroll
  for (int s = 0; s < R0; ++s) {
    const size_t o = refill_off();
#pragma unroll
    for (int c = 0; c < C; ++c) ring[s][c] = ld_w(tb + o + c * kWave);
  }
  const bool fold = (XM == XM_F16 || XM == XM_ATTN) && kind == TI_EPI_RESID_F32 && a.epi.fold_x != nullptr;
  if constexpr (XM == XM_F16 || XM == XM_ATTN) {   // fold weight (consumed by the epilogue)
    const float* fw_p = fold ? a.epi.fold_w + (size_t)t0 * 16 + (tid < n_res ? tid : 0) : pre_p;
    fw_pre = *fw_p;
  }

  GEMV_TS(1);
  STAMP_MARK(ph_issued);
  // ---- 3. stage scales and x in LDS (waits only for the loads of step 1)
  if constexpr (KQ) {   // (entry tid of the workgroup's [ntl][K/256][16 rows]: decoded, kq_stage_entry)
    if (tid < n_sc) kq_stage_entry(sc_reg, tid, sl, (uint32_t*)ml);
  } else if constexpr (BITS != 16) {
    if (tid < n_sc) ((u32x4*)sl)[tid] = sc_reg;
  }
  // int4 (group 128): the x pieces staged from registers get their 1/16 scaling and offset correction
  // here, before the staging barrier (no second LDS pass and barrier in front of the stream); every
  // piece of x must come from registers for that (rare long shapes take the pass below)
  constexpr bool kRegPrep = BITS == 4 && !G32 && (XM == XM_NORM1 || XM == XM_ATTN || XM == XM_F16 || XM == XM_F16F);
  const bool reg_prep = kRegPrep && (XM == XM_NORM1 || XM == XM_ATTN || nx16 <= XPF * kGemvThreads);
  if constexpr (XM == XM_NORM1) {
    // rms_norm (tensor_engine.cpp:1488-1505) of the single row, x and w held in registers.
    float ss = 0.0f;
    if (tid < K8) {
      ss = fmaf(v0.x, v0.x, ss); ss = fmaf(v0.y, v0.y, ss); ss = fmaf(v0.z, v0.z, ss); ss = fmaf(v0.w, v0.w, ss);
      ss = fmaf(v1.x, v1.x, ss); ss = fmaf(v1.y, v1.y, ss); ss = fmaf(v1.z, v1.z, ss); ss = fmaf(v1.w, v1.w, ss);
    }
    ss = group_sum<kWave>(ss);
    if (lane == 0) red[wave] = ss;
    lds_barrier();
    float tot = 0.0f;
#pragma unroll
    for (int w = 0; w < kGemvWaves; ++w) tot += red[w];
    const float rms = sqrtf(tot / (float)a.K + a.eps);
    float part = 0.0f;
    if (tid < K8) {
      f16x8 h;
      h[0] = (f16)((v0.x / rms) * w0.x); h[1] = (f16)((v0.y / rms) * w0.y);
      h[2] = (f16)((v0.z / rms) * w0.z); h[3] = (f16)((v0.w / rms) * w0.w);
      h[4] = (f16)((v1.x / rms) * w1.x); h[5] = (f16)((v1.y / rms) * w1.y);
      h[6] = (f16)((v1.z / rms) * w1.z); h[7] = (f16)((v1.w / rms) * w1.w);
      if constexpr (kRegPrep) part = int4_x_prep(h);
      *(f16x8*)(xl + 8 * tid) = h;
      if constexpr (KQ) put_bsum(bsum, h, 0, tid);
    }
    if constexpr (kRegPrep) {
      part = group_sum<16>(part);
      if (tid < K8 && (lane & 15) == 0) corr[(tid >> 4) * 16] = part;
    }
  } else if constexpr (XM == XM_ATTN) {
    // the attention's split merge (attention.hip last-arriver merge): weights
    // l_s * exp(m_s - max), normalised rows o_s, empty splits (m = -inf) weigh 0
    const int S = (int)((unsigned)p_kx >> 16);
    float mx = -INFINITY;
#pragma unroll
    for (int sp = 0; sp < kPS; ++sp) mx = sp < S ? fmaxf(mx, pml[sp].x) : mx;
    float num[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, den = 0.0f;
#pragma unroll
    for (int sp = 0; sp < kPS; ++sp) {
      const float f = sp < S && pml[sp].x != -INFINITY ? pml[sp].y * __expf(pml[sp].x - mx) : 0.0f;
      den += f;
      const f16x8 o = __builtin_bit_cast(f16x8, po[sp]);
#pragma unroll
      for (int e = 0; e < 8; ++e) num[e] = fmaf(f, (float)o[e], num[e]);
    }
    float part = 0.0f;
    if (tid < K8) {
      f16x8 hx;
#pragma unroll
      for (int e = 0; e < 8; ++e) hx[e] = (f16)(den > 0.0f ? num[e] / den : 0.0f);
      if constexpr (kRegPrep) part = int4_x_prep(hx);
      *(f16x8*)(xl + 8 * tid) = hx;
      if constexpr (KQ) put_bsum(bsum, hx, 0, tid);
    }
    if constexpr (kRegPrep) {
      part = group_sum<16>(part);
      if (tid < K8 && (lane & 15) == 0) corr[(tid >> 4) * 16] = part;
    }
  } else if constexpr (XM == XM_F16 || XM == XM_F16F) {
#pragma unroll
    for (int q = 0; q < XPF; ++q) {
      const int i = tid + q * kGemvThreads;
      const int m = kOneRow || i >= nx16 ? 0 : i / K8, k8 = i - m * K8;
      float part = 0.0f;
      if (i < nx16) {
        if (kRegPrep && reg_prep) {
          f16x8 h = __builtin_bit_cast(f16x8, xr16[q]);
          part = int4_x_prep(h);
          *(f16x8*)(xl + m * xs + 8 * k8) = h;
        } else {
          *(u32x4*)(xl + m * xs + 8 * k8) = xr16[q];
          if constexpr (KQ) put_bsum(bsum, __builtin_bit_cast(f16x8, xr16[q]), m, k8);
        }
      }
      if (kRegPrep && reg_prep) {   // (uniform: every lane of a 16-lane group has the same q)
        part = group_sum<16>(part);
        if (i < nx16 && (lane & 15) == 0) corr[(k8 >> 4) * 16 + m] = part;
      }
    }
  }
  // rare shapes: what the register prefetch did not cover (these loads wait behind the ring)
  if constexpr (KQ) {
    for (int i = tid + kGemvThreads; i < n_sc; i += kGemvThreads) kq_stage_entry(sg[i], i, sl, (uint32_t*)ml);
  } else if constexpr (BITS != 16) {
    for (int i = tid + kGemvThreads; i < n_sc; i += kGemvThreads) ((u32x4*)sl)[i] = sg[i];
  }
  if constexpr (AFF) {   // the minimums follow all N/16 tiles' scales in the same buffer
    const u32x4* mg = (const u32x4*)(a.scales + (size_t)NT * KT * 64 + (size_t)t0 * KT * 64);
    for (int i = tid; i < n_sc; i += kGemvThreads) ((u32x4*)ml)[i] = mg[i];
  }
  if constexpr (XM == XM_F16 || XM == XM_F16F) {
    if (nx16 > XPF * kGemvThreads) stage_x_generic<XM, KQ>(a, xl, red, XPF * kGemvThreads, bsum);
  } else if constexpr (XM != XM_NORM1 && XM != XM_ATTN) {
    stage_x_generic<XM, KQ>(a, xl, red, 0, bsum);
  }
  if ((EPI >= 0 ? kind : a.epi.kind) == TI_EPI_QKV_ROPE_KV && tid < a.M) ((int*)(es + a.M * a.epi.head_dim))[tid] = __builtin_bit_cast(int, pre);
  if (tid < 16) best_l[tid] = 0ull;
  lds_barrier();
  STAMP_MARK(ph_staged);
#pragma unroll
  for (int s = R0; s < R; ++s) {
    const size_t o = refill_off();
#pragma unroll
    for (int c = 0; c < C; ++c) ring[s][c] = ld_w(tb + o + c * kWave);
  }
  if constexpr (BITS == 4 && !MX && !KQ) if (!reg_prep) {
    // Offset-folded int4 (deq_int4_raw): scale the high-nibble slots of x by 1/16 (exact in
    // fp16) and build corr[g][m] = 1032 * sum_lo a + 1152 * sum_hi a per 128-k group.  A
    // group is 16 consecutive k8 pieces, i.e. 16 consecutive lanes (K8 % 16 == 0).
    const f16 s16 = (f16)0.0625f;
    for (int i0 = 0; i0 < a.M * K8; i0 += kGemvThreads) {
      const int idx = i0 + tid;
      float part = 0.0f, sx = 0.0f;
      int m = 0, k8 = 0;
      if (idx < a.M * K8) {
        m = idx / K8;
        k8 = idx - m * K8;
        f16x8 h = *(const f16x8*)(xl + m * xs + 8 * k8);
        h[2] *= s16; h[3] *= s16; h[6] *= s16; h[7] *= s16;
        *(f16x8*)(xl + m * xs + 8 * k8) = h;
        const float lo = ((float)h[0] + (float)h[1]) + ((float)h[4] + (float)h[5]);
        const float hi = ((float)h[2] + (float)h[3]) + ((float)h[6] + (float)h[7]);
        part = 1032.0f * lo + 1152.0f * hi;
        if constexpr (AFF) sx = lo + 16.0f * hi;   // the piece's sum of x (high slots were scaled by 1/16)
      }
      if constexpr (G32) {   // one 32-k block = 4 consecutive pieces
        part = group_sum<4>(part);
        if (idx < a.M * K8 && (lane & 3) == 0) corr[(k8 >> 2) * 16 + m] = part;
        if constexpr (AFF) {
          sx = group_sum<4>(sx);
          if (idx < a.M * K8 && (lane & 3) == 0) bsum[(k8 >> 2) * 16 + m] = sx;
        }
      } else {
        part = group_sum<16>(part);
        if (idx < a.M * K8 && (lane & 15) == 0) corr[(k8 >> 4) * 16 + m] = part;
      }
    }
    lds_barrier();
  }

  // RoPE (cos, sin) of each row's position: issued now, consumed after the stream.
  float cs_reg = 0.0f;
  const int n_cs = EPI < 0 && a.epi.kind == TI_EPI_QKV_ROPE_KV ? a.M * a.epi.head_dim : 0;
  if (n_cs > 0) {
    const int hd = a.epi.head_dim, idx = tid < n_cs ? tid : 0, m = idx / hd, j = idx - m * hd;
    cs_reg = a.epi.rope_cs[(size_t)((const int*)(es + a.M * hd))[m] * hd + j];
  }

  // One-row instances (EPI >= 0): everything the tail needs that does not depend on the stream is worked
  // out here, where the waves wait for the ring anyway.  Thread tid owns output (tile tid >> 4,
  // n = tid & 15) -- the generic M <= 4 epilogue's assignment of outputs to waves and lanes, which
  // the fold's per-wave sums of h^2 depend on; the launcher guarantees ntl * 16 <= kGemvThreads.
  const bool o_ok = tid < ntl * 16;
  const int o_tl = o_ok ? tid >> 4 : 0, o_ng = (t0 + o_tl) * 16 + (lane & 15);
  [[maybe_unused]] float o_rms = 1.0f;            // XM_F16F: the row's rms (same sum in every wave)
  [[maybe_unused]] void* o_out = nullptr;         // this thread's output element
  [[maybe_unused]] uint16_t* o_fx = nullptr;      // RESID with fold: its fold_x element
  [[maybe_unused]] float2 o_cs = {1.0f, 0.0f};    // ROPE: (cos, sin) of the pair at the row's position
  [[maybe_unused]] int o_rot = 0;                 // ROPE: 0 = no rotation (v rows), 1 = even dim, 2 = odd dim
  [[maybe_unused]] uint32_t o_ci = 0;             // ROPE: element index into the K / V cache
  if constexpr (EPI >= 0) {
    if constexpr (XM == XM_F16F && TI_GEMV_ONEROW_RMS_EARLY) {
      float t = 0.0f;
#pragma unroll
      for (int j = 0; j < 4; ++j) t += lane + 64 * j < n_ss ? ss4[j] : 0.0f;
      t = group_sum<kWave>(t);
      o_rms = sqrtf(t / (float)a.K + a.eps);
    }
    if constexpr (EPI == TI_EPI_RESID_F32) {
      o_out = (void*)pre_p;                        // (p_pre is epi.out: the residual is updated in place)
      if (fold) o_fx = a.epi.fold_x + o_ng;
    } else if constexpr (EPI == TI_EPI_SILU_MUL_F16) {
      o_out = (uint16_t*)a.epi.out + (t0 + o_tl) * 8 + (lane & 7);
    } else if constexpr (EPI == TI_EPI_LOGITS_ARGMAX) {
      o_out = (float*)a.epi.out + o_ng;
    } else if constexpr (EPI == TI_EPI_QKV_ROPE_KV) {
      const ti_epilogue& e = a.epi;
      const int hd = e.head_dim, p = ((const int*)(es + hd))[0];   // (staged before the barrier above)
      const bool is_q = o_ng < e.q_dim, qk = o_ng < e.q_dim + e.kv_dim;
      const int c = o_ng - (is_q ? 0 : e.q_dim) - (qk ? 0 : e.kv_dim);
      const int kvh = c / hd, d = c - kvh * hd;
      if (qk) {
        o_rot = 1 + (d & 1);
        o_cs = *(const float2*)(e.rope_cs + (size_t)p * hd + (d & ~1));
      }
      if (is_q) {
        o_out = (float*)e.out + o_ng;
      } else {
        o_out = qk ? e.k_cache : e.v_cache;
        o_ci = (uint32_t)((kvh * e.max_seq + p) * hd + d);
      }
    }
  }

  GEMV_TS(2);
  STAMP_MARK(ph_stream);
  // ---- 4. the stream: branch-free, R items per block
  const int r = lane & 15, kq = lane >> 4;
  const f16* xrow = xl + (r < a.M ? r : a.M - 1) * xs + kq * 32;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t magic;   // 0x64006400 in a VGPR (see deq_int4_raw)
  asm volatile("v_mov_b32 %0, 0x64006400" : "=v"(magic));
  f32x4* my_slab = slab + wave * kWave + lane;     // + tile * 8 * 64
  constexpr int kSlabStride = kGemvWaves * kWave;
  int ct = 0, ck = 0;                              // compute cursor: tile, k index
  auto item = [&](const u32x4 (&w)[C]) {
    const int kt = wave + kGemvWaves * ck;
    f32x4 t = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (BITS == 16) t = acc;
    if constexpr (KQ) {
      const f16* xr32 = xrow - kq * 32 + kq * 8;   // this lane's 8 k of each 32-k block
      const uint32_t ddw = ((const uint32_t*)ml)[(ct * (KT >> 1) + (kt >> 1)) * 16 + r];   // the super-block's d | dmin
      const float fd = h2f((uint16_t)ddw), fnm = -h2f((uint16_t)(ddw >> 16));
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const f16x8 bf = deq_q4k(w[0][s4]);
        const f16x8 af = *(const f16x8*)(xr32 + kt * 128 + s4 * 32);
        const f32x4 tb = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, (f32x4){0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
        const uint32_t scm = sl[((ct * KT + kt) * 4 + s4) * 16 + r];   // sc | m << 8 of the block
        const float dsc = fd * (float)(scm & 0xffu), nm = fnm * (float)(scm >> 8);   // (both exact in fp32)
        const f32x4 bs = *(const f32x4*)(bsum + (kt * 4 + s4) * 16 + 4 * kq);
        acc[0] = fmaf(dsc, tb[0], acc[0]);
        acc[1] = fmaf(dsc, tb[1], acc[1]);
        acc[2] = fmaf(dsc, tb[2], acc[2]);
        acc[3] = fmaf(dsc, tb[3], acc[3]);
        acc[0] = fmaf(nm, bs[0], acc[0]);
        acc[1] = fmaf(nm, bs[1], acc[1]);
        acc[2] = fmaf(nm, bs[2], acc[2]);
        acc[3] = fmaf(nm, bs[3], acc[3]);
      }
    } else if constexpr (G32) {
      const f16* xr32 = xrow - kq * 32 + kq * 8;   // this lane's 8 k of each 32-k block
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        f16x8 bf;
        if constexpr (MX) bf = deq_mxfp4(w[0][s4]);
        else bf = dequant_step<BITS>(w, s4, magic);
        const f16x8 af = *(const f16x8*)(xr32 + kt * 128 + s4 * 32);
        f32x4 tb = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, (f32x4){0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
        if constexpr (BITS == 4 && !MX) tb -= *(const f32x4*)(corr + (kt * 4 + s4) * 16 + 4 * kq);
        float sc;
        if constexpr (MX) sc = e8m0_to_f32(((const uint8_t*)sl)[((ct * KT + kt) * 4 + s4) * 16 + r]);
        else sc = h2f(sl[((ct * KT + kt) * 4 + s4) * 16 + r]);
        acc[0] = fmaf(sc, tb[0], acc[0]);
        acc[1] = fmaf(sc, tb[1], acc[1]);
        acc[2] = fmaf(sc, tb[2], acc[2]);
        acc[3] = fmaf(sc, tb[3], acc[3]);
        if constexpr (AFF) {   // weight = d (q - 8) + (8 d + m): the offset term times the block's sum of x
          const float mt = fmaf(8.0f, sc, h2f(ml[((ct * KT + kt) * 4 + s4) * 16 + r]));
          const f32x4 bs = *(const f32x4*)(bsum + (kt * 4 + s4) * 16 + 4 * kq);
          acc[0] = fmaf(mt, bs[0], acc[0]);
          acc[1] = fmaf(mt, bs[1], acc[1]);
          acc[2] = fmaf(mt, bs[2], acc[2]);
          acc[3] = fmaf(mt, bs[3], acc[3]);
        }
      }
    } else {
#if TI_GEMV_EXP & 1   // diagnostic build (tools/probe_gemv.hip): stream only, no dequant / MFMA
    t[0] += __builtin_bit_cast(float, w[0][0] ^ w[0][1] ^ w[0][2] ^ w[0][3]) + (float)xrow[kt];
#else
    (void)t;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const f16x8 bf = dequant_step<BITS>(w, s4, magic);
      const f16x8 af = *(const f16x8*)(xrow + kt * 128 + s4 * 8);
      t = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, t, 0, 0, 0);
    }
#endif
    if constexpr (BITS == 16) {
      acc = t;
    } else {
      if constexpr (BITS == 4) {   // remove the folded offsets of this group (deq_int4_raw)
        const f32x4 cr = *(const f32x4*)(corr + kt * 16 + 4 * kq);
        t -= cr;
      }
      const float sc = h2f(sl[(ct * KT + kt) * 16 + r]);
      acc[0] = fmaf(sc, t[0], acc[0]);
      acc[1] = fmaf(sc, t[1], acc[1]);
      acc[2] = fmaf(sc, t[2], acc[2]);
      acc[3] = fmaf(sc, t[3], acc[3]);
    }
    }   // !KQ && !G32
    // the tile's last item lands in its slab, every other item in the dummy slab
    const bool last = ++ck == KW;
    my_slab[(last ? ct : ntl) * kSlabStride] = acc;
    if (last) acc = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    ck = last ? 0 : ck;
    ct += last ? 1 : 0;
  };
  int j0 = 0;
#if TI_GEMV_SYNC > 0
  // Waves of a CU drift apart (the oldest wins issue arbitration); a workgroup barrier every
  // TI_GEMV_SYNC blocks keeps them together while every wave still has blocks left (the
  // count of barriers is the same for all waves: blocks below the smallest wave total).
  const int common = ntl * (KT / kGemvWaves);
  int blk = 0;
  for (; j0 + R <= common; j0 += R) {
#pragma unroll
    for (int s = 0; s < R; ++s) {
      item(ring[s]);
      const size_t o = refill_off();
#pragma unroll
      for (int c = 0; c < C; ++c) ring[s][c] = ld_w(tb + o + c * kWave);
    }
    if (++blk == TI_GEMV_SYNC) {
      blk = 0;
      __builtin_amdgcn_s_barrier();
    }
  }
#endif
  for (; j0 + R <= total; j0 += R) {   // full blocks: no branches, R items scheduled together
#pragma unroll
    for (int s = 0; s < R; ++s) {
      item(ring[s]);
      const size_t o = refill_off();   // refill this slot R items ahead (clamped past the end)
#pragma unroll
      for (int c = 0; c < C; ++c) ring[s][c] = ld_w(tb + o + c * kWave);
    }
  }
#pragma unroll
  for (int s = 0; s < R; ++s)          // tail: the last total % R items, nothing refilled
    if (j0 + s < total) item(ring[s]);
  if (KW == 0)   // K < 8*128: this wave owns no k-tiles; its partials are zero
    for (int tl = 0; tl < ntl; ++tl) my_slab[tl * kSlabStride] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

  GEMV_TS(3);
  GEMV_WTS();
  STAMP_MARK(ph_streamed);
  if constexpr (EPI >= 0) {
    // ---- 5'. the one-row tail: nothing but the barrier between a wave's last item and the reduction.
    // The residual and the fold weight of output tid are this thread's own prefetched words (the generic
    // tail passes them through es[tid]); the 8 partials are read as the m = 0 component alone, all
    // reads issued together, and summed in the generic order; the kind's arithmetic is epilogue()'s.
    if constexpr (XM == XM_F16F && !TI_GEMV_ONEROW_RMS_EARLY) {   // (A/B form: the rms where the generic tail has it)
      float t = 0.0f;
#pragma unroll
      for (int j = 0; j < 4; ++j) t += lane + 64 * j < n_ss ? ss4[j] : 0.0f;
      t = group_sum<kWave>(t);
      o_rms = sqrtf(t / (float)a.K + a.eps);
    }
    lds_barrier();
    STAMP_MARK(ph_reduce);
    float ssacc = 0.0f;
    if (wave * kWave < ntl * 16) {   // (wave-uniform) the waves that own outputs
      const float* sp = (const float*)(slab + o_tl * kSlabStride + (lane & 15));
      float pw[kGemvWaves];
#pragma unroll
      for (int w = 0; w < kGemvWaves; ++w) pw[w] = sp[w * kWave * 4];
      float v = pw[0];
#pragma unroll
      for (int w = 1; w < kGemvWaves; ++w) v += pw[w];
      if constexpr (XM == XM_F16F) v = v / o_rms;
      if constexpr (EPI == TI_EPI_RESID_F32) {
        if (o_ok) {
          const float r = pre + v;
          *(float*)o_out = r;
          if (fold) {
            *o_fx = f2h(r * fw_pre);
            ssacc = fmaf(r, r, ssacc);
          }
        }
      } else if constexpr (EPI == TI_EPI_SILU_MUL_F16) {
        const float up = lane_xor<8>(v);   // lanes n < 8: the up row n + 8 of the same tile
        const float s = v / (1.0f + expf(-v));
        if (o_ok && (lane & 8) == 0) *(uint16_t*)o_out = f2h(up * s);
      } else if constexpr (EPI == TI_EPI_QKV_ROPE_KV) {
        const float partner = lane_xor<1>(v);
        float r = v;
        if (o_rot == 1) r = fmaf(-partner, o_cs.y, v * o_cs.x);
        else if (o_rot == 2) r = fmaf(v, o_cs.x, partner * o_cs.y);
        if (o_ok) {
          if (o_ng < a.epi.q_dim) *(float*)o_out = r;
          else if (a.epi.kv_fp8) ((uint8_t*)o_out)[o_ci] = f2e4m3(r);
          else ((uint16_t*)o_out)[o_ci] = f2h(r);
        }
      } else if constexpr (EPI == TI_EPI_LOGITS_ARGMAX) {
        // the workgroup's key: a maximum, so any order of merging gives the generic tail's bits; each
        // wave that owns outputs merges its own into the slot (no LDS pass, no second barrier)
        unsigned long long best = 0ull;
        if (o_ok) {
          *(float*)o_out = v;
          best = ((unsigned long long)float_order_key(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)o_ng);
        }
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
          const unsigned long long other = __shfl_xor(best, o, kWave);
          best = other > best ? other : best;
        }
        if (lane == 0 && best) atomicMax(a.epi.argmax + (bid & (TI_ARGMAX_SLOTS - 1)), best);
      }
    }
    STAMP_MARK(ph_epi);
    if constexpr (EPI == TI_EPI_LOGITS_ARGMAX) {
      if (a.epi.step_ctr && bid == 0 && tid == 0) *a.epi.step_ctr += a.epi.advance;
    }
    if constexpr (EPI == TI_EPI_RESID_F32) {   // the workgroup's sum of h^2: the generic tail's two forms
      if (fold && ntl * 16 <= kWave) {
        if (wave == 0) {
          const float sw = group_sum<kWave>(ssacc);
          if (lane == 0) a.epi.fold_ss[bid] = sw;
        }
      } else if (fold) {
        float* red2 = (float*)best_l;
        const float sw = group_sum<kWave>(ssacc);
        if (lane == 0) red2[wave] = sw;
        lds_barrier();
        if (tid == 0) {
          float t = 0.0f;
#pragma unroll
          for (int w = 0; w < kGemvWaves; ++w) t += red2[w];
          a.epi.fold_ss[bid] = t;
        }
      }
    }
    GEMV_TS(4);
    stamp_end(a.stamp, t_entry, ph_issued, ph_staged, ph_stream, ph_streamed, ph_reduce, ph_epi, ph_streamed);
    return;
  }
  // ---- 5. epilogue inputs into LDS, reduce the 8 partials per tile, epilogue
  if (tid < n_res) es[tid] = pre;
  if (fold && tid < n_res) es[n_res + tid] = fw_pre;
  if (tid < n_cs) es[tid] = cs_reg;
  // inputs past the one-per-thread prefetch (ntl * M * 16 or M * head_dim > 512): loaded now
  for (int i = tid + kGemvThreads; i < n_res; i += kGemvThreads) {
    const int tl = i / (a.M * 16), rem = i - tl * a.M * 16, m = rem >> 4, n = rem & 15;
    es[i] = p_pre[(size_t)m * ldo + (t0 + tl) * 16 + n];
    if (fold) es[n_res + i] = a.epi.fold_w[(size_t)t0 * 16 + i];
  }
  // XM_F16F: rms of the row from the producer's partials, the same fixed-order sum in every
  // wave (rms_norm, tensor_engine.cpp:1488-1505, with the division moved behind the GEMM)
  float rms = 1.0f;
  if constexpr (XM == XM_F16F) {
    float t = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) t += lane + 64 * j < n_ss ? ss4[j] : 0.0f;
    t = group_sum<kWave>(t);
    rms = sqrtf(t / (float)a.K + a.eps);
  }
  float ssacc = 0.0f;
  const float* fw_l = es + n_res;
  for (int i = tid + kGemvThreads; i < n_cs; i += kGemvThreads) {
    const int hd = a.epi.head_dim, m = i / hd, j = i - m * hd;
    es[i] = a.epi.rope_cs[(size_t)((const int*)(es + a.M * hd))[m] * hd + j];
  }
  lds_barrier();
  GEMV_TS(5);
  STAMP_MARK(ph_reduce);
  unsigned long long best[4] = {0ull, 0ull, 0ull, 0ull};
  if (a.M <= 4) {
    // rows m < 4 live in lanes 0-15 of each partial (C layout m = 4*(l>>4) + i): one thread per
    // (tile, n), all tiles in one pass over the workgroup, the M components of its f32x4.
    for (int tb0 = wave * kWave; tb0 < ntl * 16; tb0 += kGemvThreads) {
      const int t = tb0 + lane, ok = t < ntl * 16, tl = ok ? t >> 4 : 0, n = lane & 15;
      const f32x4* sp = slab + tl * kSlabStride + n;
      f32x4 v = sp[0];
#pragma unroll
      for (int w = 1; w < kGemvWaves; ++w) v += sp[w * kWave];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < a.M) epilogue(a, t0 + tl, tl, n, i, XM == XM_F16F ? v[i] / rms : v[i], es, best[i], ok, fw_l, ssacc);
    }
  } else {
    const int i4 = wave & 3;
    for (int tl = wave >> 2; tl < ntl; tl += 2) {
      const float* sp = (const float*)(slab + tl * kSlabStride + lane) + i4;
      float v = 0.0f;
#pragma unroll
      for (int w = 0; w < kGemvWaves; ++w) v += sp[w * kWave * 4];
      epilogue(a, t0 + tl, tl, lane, i4, v, es, best[0], true, fw_l, ssacc);
    }
  }
  STAMP_MARK(ph_epi);
  if (a.epi.kind == TI_EPI_LOGITS_ARGMAX) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const unsigned long long other = __shfl_xor(best[i], o, kWave);
        best[i] = other > best[i] ? other : best[i];
      }
    }
    if (a.M <= 4) {
      if ((lane & 15) == 0)
#pragma unroll
        for (int i = 0; i < 4; ++i)   // constant bounds: best[] stays in registers
          if (i < a.M && best[i]) atomicMax(best_l + i, best[i]);
    } else {
      const int m = 4 * (lane >> 4) + (wave & 3);
      if ((lane & 15) == 0 && m < a.M && best[0]) atomicMax(best_l + m, best[0]);
    }
    lds_barrier();
    if (tid < a.M && best_l[tid])
      atomicMax(a.epi.argmax + (size_t)tid * TI_ARGMAX_SLOTS + (bid & (TI_ARGMAX_SLOTS - 1)), best_l[tid]);
    if (a.epi.step_ctr && bid == 0 && tid == 0) *a.epi.step_ctr += a.epi.advance;
  }
  if (fold && a.M <= 4 && ntl * 16 <= kWave) {
    // every output of the workgroup was wave 0's (the M <= 4 epilogue above): its sum alone, no
    // barrier -- the same value as the general form below, whose other terms are exact zeros
    if (wave == 0) {
      const float sw = group_sum<kWave>(ssacc);
      if (lane == 0) a.epi.fold_ss[bid] = sw;
    }
  } else if (fold) {   // this workgroup's sum of h^2, waves in a fixed order (best_l: unused by RESID)
    float* red2 = (float*)best_l;
    const float sw = group_sum<kWave>(ssacc);
    if (lane == 0) red2[wave] = sw;
    lds_barrier();
    if (tid == 0) {
      float t = 0.0f;
#pragma unroll
      for (int w = 0; w < kGemvWaves; ++w) t += red2[w];
      a.epi.fold_ss[bid] = t;
    }
  }
  GEMV_TS(4);
  stamp_end(a.stamp, t_entry, ph_issued, ph_staged, ph_stream, ph_streamed, ph_reduce, ph_epi, ph_streamed);
