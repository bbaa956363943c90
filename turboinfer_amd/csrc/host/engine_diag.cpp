// engine_diag.cpp -- the diagnostics bench.py --full builds on: one launch class timed alone
// (ti_engine_time_kernel) and the in-step launch stamps (ti_engine_stamp_steps).
#include "engine_impl.hpp"

using namespace ti_eng;

thread_local StampCtx ti_eng::g_stamp;

namespace {
struct OwnedExec {   // a graph of this file's own, outside the engine's cache: destroyed on every path
  hipGraphExec_t g = nullptr;
  ~OwnedExec() {
    if (g) hipGraphExecDestroy(g);
  }
};
}  // namespace

extern "C" {

int ti_engine_time_kernel(ti_engine* e, int which, int n, int kv_len, int reps, double* avg_us, double* bytes) {
  if (!e || e->c.compat || !avg_us || !bytes || reps < 1 || n < 1 || n > e->c.max_batch || e->c.layers < 1)
    return ti_set_error(TI_ERR_ARG, "ti_engine_time_kernel: bad arguments");
  DeviceScope bind_(e);
  TI_TRY(share_clear(e));   // (the timed QKV launches append at whatever positions the last call left)
  const ti_engine_config& c = e->c;
  const int H = c.hidden, I = c.inter, qd = e->qd(), kvd = e->kvd();
  // the step's own plan, epilogues and fold wiring (engine_step.cpp), but never its fused QKV + attention route
  const StepPlan p = plan_step(e, n);
  // Launch r uses layer r % layers, so (as in a real step) its weights are not still in
  // the 256 MB Infinity Cache from the previous launch.
  int cur = 0;
  auto setup = [&](DevLayer& L, const DevLinear*& W, const void*& x, int& xk, int& ldx, const float*& nw,
                     ti_epilogue& ep) -> int {
    W = nullptr; x = nullptr; xk = TI_X_F16; ldx = 0; nw = nullptr; ep = ti_epilogue{};
    switch (which) {
      case 0: W = &L.qkv; x = e->h; xk = TI_X_F32_RMSNORM; ldx = H; nw = L.attn_norm;
        ep = qkv_epilogue(e, L.kc, L.vc, e->kv_stride); break;
      case 1: W = &L.o; x = e->attn; ldx = qd; ep = resid_epilogue(e); break;
      case 2: W = &L.gu; x = e->h; xk = TI_X_F32_RMSNORM; ldx = H; nw = L.ffn_norm; ep = silu_epilogue(e, p.packed); break;
      case 3: W = &L.down; x = e->act; ldx = I; ep = resid_epilogue(e); break;
      case 4: W = &e->lm; x = e->h; xk = TI_X_F32_RMSNORM; ldx = H; nw = e->out_norm; ep = logits_epilogue(e, e->logits); break;
      case 5: break;
      default: return ti_set_error(TI_ERR_ARG, "ti_engine_time_kernel: which=%d", which);
    }
    if (which == 1 || which == 3) {
      // into a scratch of n*H floats, not h: q holds n*qd >= n*H only if qd >= H
      if ((size_t)qd < (size_t)H) return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_time_kernel: scratch too small");
      ep.out = e->q;
      // the step's producer form (residual add + fold outputs) where it folds, else a plain store
      if (!p.fold && !p.bfold) ep.kind = TI_EPI_STORE_F32;
      fold_into(e, p, ep, L.ffn_norm, which == 1 ? L.gu.N : L.qkv.N);
      if (which == 1 && p.part) {   // O merges the attention's split partials
        x = e->part_o;
        xk = TI_X_ATTN_SPLITS;
        ep.ss_in = e->part_ml;
        ep.n_ss = p.splits;
        ep.head_dim = c.head_dim;
      }
      if (p.packed) xk = TI_X_F16_PACKED;   // enqueue_step's operands
    }
    if (xk == TI_X_F32_RMSNORM) {   // the step's consumer form, behind a producer over qd (gate/up) or inter columns
      const int pk = which == 2 ? qd : I;
      norm_in(e, p, p.fold ? ti_gemm_grid(1, H, pk) : 0, p.bfold ? ti_gemm_fold_partials(c.bits, n, H, pk) : 0, x, xk,
              ldx, nw, ep, W->N);
    }
    return TI_OK;
  };
  const DevLinear* W = nullptr;
  const void* x = nullptr;
  int xk = TI_X_F16, ldx = 0;
  const float* nw = nullptr;
  ti_epilogue ep{};
  TI_TRY(setup(e->layer[0], W, x, xk, ldx, nw, ep));
  if (ep.ss_in == e->ss_rows && ep.n_ss > 0) {   // batched fold: partials of rms 1 per row
    const float v = (float)H / (float)ep.n_ss;
    TI_TRY(ti_fill_uniform_f32(1, 0, (uint64_t)ep.n_ss * TI_FOLD_SS_ROWS, 0.0f, v, e->ss_rows, e->s));
  }
  std::vector<int32_t> base(n, kv_len - 1);
  TI_TRY(ti_memcpy_h2d(e->pos, base.data(), (size_t)n * 4, e->s));
  auto launch = [&]() -> int {
    DevLayer& L = e->layer[cur];
    cur = (cur + 1) % c.layers;
    TI_TRY(setup(L, W, x, xk, ldx, nw, ep));
    // (the one lm_head, 68 MB at 7B, fits the Infinity Cache: back-to-back it runs warm)
    if (which == 5 && p.part) return attn_partials(e, L.kc, L.vc, n, p.splits);
    if (which == 5) return attn_merged(e, p.packed, L.kc, L.vc, e->kv_stride, n, p.splits);
    return gemm_rows(e, *W, n, x, xk, ldx, nw, ep, which == 2 ? 2 : 4, false);
  };
  // The `reps` launches are captured once into a graph and the graph is replayed `rounds`
  // times between two HIP events: no host launch cost inside the timed region (eager
  // launches of ~10 us kernels can go host-bound on a slow host and read 2x long), and
  // several milliseconds of back-to-back work, so the clocks are those of a running step.
  TI_TRY(ti_stream_sync(e->s));
  OwnedExec owned;
  TI_TRY(capture_graph(e, [&] {
    int rc = TI_OK;
    for (int r = 0; r < reps && rc == TI_OK; ++r) rc = launch();
    return rc;
  }, &owned.g));
  const hipGraphExec_t gx = owned.g;
  const int rounds = which == 6 ? std::max(4, 32 / reps) : std::max(4, 4096 / reps);
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t el = hipEventCreate(&a);
  if (el == hipSuccess) el = hipEventCreate(&b);
  if (el == hipSuccess) el = hipGraphLaunch(gx, e->s);   // warm (code objects, caches, clocks)
  if (el == hipSuccess) el = hipEventRecord(a, e->s);
  for (int r = 0; r < rounds && el == hipSuccess; ++r) el = hipGraphLaunch(gx, e->s);
  if (el == hipSuccess) el = hipEventRecord(b, e->s);
  if (el == hipSuccess) el = hipEventSynchronize(b);
  float ms = 0.0f;
  if (el == hipSuccess) el = hipEventElapsedTime(&ms, a, b);
  if (a) hipEventDestroy(a);
  if (b) hipEventDestroy(b);
  E_CHECK(el, "ti_engine_time_kernel: graph replay");
  // per projection (all row chunks of it, and the rms_norm prep of the batched path)
  *avg_us = (double)ms * 1000.0 / ((double)reps * rounds);
  if (which == 5) {
    *bytes = 2.0 * n * (double)kvd * kv_len * (double)e->kv_esz() + (double)n * qd * (4 + 2);
  } else if (which == 6) {   // every layer's weights + scales, K/V read at kv_len, K/V row written
    double wl = 0.0;
    for (const DevLinear* L : {&e->layer[0].qkv, &e->layer[0].o, &e->layer[0].gu, &e->layer[0].down})
      wl += (double)ti_wpack_tile_bytes(c.bits, L->K, L->N) + (double)ti_wpack_scale_bytes(c.bits, L->K, L->N);
    *bytes = c.layers * (wl + 2.0 * (double)kvd * kv_len * (double)e->kv_esz() + 2.0 * kvd * (double)e->kv_esz());
  } else {
    const double wbytes = (double)ti_wpack_tile_bytes(c.bits, W->K, W->N) + (double)ti_wpack_scale_bytes(c.bits, W->K, W->N);
    *bytes = wbytes + (double)n * W->K * (xk == TI_X_F16 || xk == TI_X_F16_FOLDED ? 2 : 4);
    if (xk == TI_X_ATTN_SPLITS) *bytes = wbytes + (double)n * W->K * 2;   // the merged row, as the unsplit input
  }
  return TI_OK;
}

}  // extern "C"

// ------------------------------------------------------------- in-step launch stamps
unsigned long long* ti_stamp_next(int kind, long grid) {
  StampCtx& c = g_stamp;
  if (!c.on) return nullptr;
  const size_t i = c.info.size() / 3;
  const bool stamped = grid > 0 && kind != TI_STAMP_KIND_RMSNORM && kind != TI_STAMP_KIND_OTHER;
  c.info.insert(c.info.end(), {(int32_t)kind, (int32_t)c.tag, stamped ? (int32_t)grid : 0});
  if (!c.base || i >= c.offs.size() || !stamped) return nullptr;
  return c.base + c.offs[i];
}

namespace {

// Capture `ksteps` replay steps back to back as one graph with the stamp context on (base NULL:
// record only).
int capture_stamped(ti_engine* e, int ksteps, unsigned long long* base, const std::vector<size_t>& offs,
                    std::vector<int32_t>& info, hipGraphExec_t* out) {
  StampCtx& c = g_stamp;
  c = StampCtx{};
  c.on = true;
  c.base = base;
  c.offs = offs;
  const int rc = capture_graph(e, [&] {
    int r = TI_OK;
    for (int k = 0; k < ksteps && r == TI_OK; ++k) r = enqueue_step(e, e->replay_M, StepMode{});
    return r;
  }, out);
  info = c.info;
  c = StampCtx{};
  return rc;
}

}  // namespace

int ti_engine_stamp_steps(ti_engine* e, int steps, int cap, int32_t* info_out, double* t_out, int* n_launch) {
  if (!e || e->replay_M < 1 || steps < 1 || steps > 256 || cap < 1 || !info_out || !t_out || !n_launch)
    return ti_set_error(TI_ERR_ARG, "ti_engine_stamp_steps: call ti_engine_replay_prepare first; 1 <= steps <= 256, "
                        "cap >= 1");
  DeviceScope bind_(e);
  TI_TRY(ti_stream_sync(e->s));
  // pass 1: one step's launch list and grids; pass 2: `steps` steps back to back in one graph, every
  // stamped launch with its own slot (so the timed steps run as replays do: no host gap between them)
  std::vector<int32_t> info, info2;
  TI_TRY(capture_stamped(e, 1, nullptr, {}, info, nullptr));
  const size_t n = info.size() / 3, nt = n * (size_t)steps;
  std::vector<size_t> offs(nt);
  size_t words = 0;
  for (size_t i = 0; i < nt; ++i) {
    offs[i] = words;
    words += (size_t)info[3 * (i % n) + 2] * kStampWords;
  }
  if (words == 0) return ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_stamp_steps: no stamped launch in the step");
  void* buf = nullptr;
  TI_TRY(ti_malloc(&buf, words * 8));
  unsigned long long* st = static_cast<unsigned long long*>(buf);
  OwnedExec owned;
  int rc = capture_stamped(e, steps, st, offs, info2, &owned.g);
  if (rc == TI_OK && (info2.size() != nt * 3 || !std::equal(info.begin(), info.end(), info2.begin())))
    rc = ti_set_error(TI_ERR_UNSUPPORTED, "ti_engine_stamp_steps: the two captures differ");
  std::vector<unsigned long long> h(words);
  for (int it = 0; rc == TI_OK && it < 2; ++it) {   // it 0: untimed (caches, clocks); it 1: the one read
    hipError_t he = hipMemsetAsync(st, 0, words * 8, e->s);
    if (he == hipSuccess) he = hipGraphLaunch(owned.g, e->s);
    if (he == hipSuccess && it == 1) he = hipMemcpyAsync(h.data(), st, words * 8, hipMemcpyDeviceToHost, e->s);
    if (he == hipSuccess) he = hipStreamSynchronize(e->s);
    if (he != hipSuccess) rc = ti_check_hip(he, "ti_engine_stamp_steps: replay");
  }
  ti_free(buf);
  TI_TRY(rc);
  // TI_STAMP_RAW=<file> (diagnostic): the stamp words as read, for per-workgroup questions the means below cannot
  // answer -- uint64 {launches per step, steps, words per workgroup}, int32 info[3 n], uint64 offs[n steps], the words
  if (const char* raw = getenv("TI_STAMP_RAW")) {
    if (FILE* f = fopen(raw, "wb")) {
      const unsigned long long hdr[3] = {n, (unsigned long long)steps, (unsigned long long)kStampWords};
      std::vector<unsigned long long> o64(offs.begin(), offs.end());
      fwrite(hdr, 8, 3, f);
      fwrite(info.data(), 4, 3 * n, f);
      fwrite(o64.data(), 8, nt, f);
      fwrite(h.data(), 8, words, f);
      fclose(f);
    }
  }
  // per launch (all steps): first / last entry, last end, median workgroup end, mean wave-end skew,
  // workgroups sharing a CU, phase marks
  constexpr double kUs = 0.01;   // s_memrealtime: 100 MHz
  std::vector<double> acc(n * TI_STAMP_FIELDS, 0.0), first(nt, 0.0), last_end(nt, 0.0);
  for (size_t i = 0; i < nt; ++i) {
    const int wgs = info[3 * (i % n) + 2];
    if (wgs == 0) continue;
    unsigned long long f = ~0ull, le = 0, lent = 0;
    double wskew = 0.0;
    std::vector<unsigned long long> ends, cus;   // cus: (XCC, SE / SH / CU) of each workgroup
    ends.reserve(wgs);
    double ph[6] = {0, 0, 0, 0, 0, 0}, sskew = 0.0;
    int sskew_n = 0;
    int phn[6] = {0, 0, 0, 0, 0, 0};
    for (int w = 0; w < wgs; ++w) {
      const unsigned long long* p = h.data() + offs[i] + (size_t)w * kStampWords;
      if (p[0]) {
        f = std::min(f, p[0]);
        lent = std::max(lent, p[0]);
      }
      if (p[15]) cus.push_back((p[15] & 0x7FFFFFFF00000000ull) | (p[15] & 0xFF00ull));
      unsigned long long smn = ~0ull, smx = 0;   // diagnostic builds: the waves' ends of stream
      for (int k = 16; k < 24; ++k)
        if (p[k]) {
          smn = std::min(smn, p[k]);
          smx = std::max(smx, p[k]);
        }
      if (smx) {
        sskew += (double)(smx - smn);
        ++sskew_n;
      }
      unsigned long long mn = ~0ull, mx = 0;
      for (int k = 1; k <= 8; ++k)   // wave ends (words 1..8)
        if (p[k]) {
          mn = std::min(mn, p[k]);
          mx = std::max(mx, p[k]);
        }
      if (mx) {
        ends.push_back(mx);
        le = std::max(le, mx);
        wskew += (double)(mx - mn);
      }
      for (int k = 0; k < 6; ++k)   // phase marks of diagnostic builds (words 9..14), relative to entry
        if (p[0] && p[9 + k] >= p[0]) {
          ph[k] += (double)(p[9 + k] - p[0]);
          ++phn[k];
        }
    }
    if (f == ~0ull || ends.empty()) continue;
    std::nth_element(ends.begin(), ends.begin() + ends.size() / 2, ends.end());
    const unsigned long long med = ends[ends.size() / 2];
    first[i] = (double)f;
    last_end[i] = (double)le;
    double* a = acc.data() + (i % n) * TI_STAMP_FIELDS;
    a[0] += (double)(le - f) * kUs;
    a[2] += (double)(lent - f) * kUs;
    a[3] += wskew / (double)ends.size() * kUs;
    a[4] += (double)(le - med) * kUs;
    std::sort(cus.begin(), cus.end());
    a[6] += (double)(cus.end() - std::unique(cus.begin(), cus.end()));   // workgroups on an already-used CU
    for (int k = 0; k < 6; ++k) a[7 + k] += phn[k] ? ph[k] / phn[k] * kUs : 0.0;
    a[13] += sskew_n ? sskew / sskew_n * kUs : 0.0;
  }
  // periods: first entry -> the next stamped launch's first entry (across step boundaries: the steps
  // ran back to back); the very last launch: its span + the mean boundary
  double gap_sum = 0.0;
  int gap_n = 0;
  size_t last = nt;
  for (size_t i = 0; i < nt; ++i) {
    if (!first[i]) continue;
    size_t j = i + 1;
    while (j < nt && !first[j]) ++j;
    double* a = acc.data() + (i % n) * TI_STAMP_FIELDS;
    if (j < nt) {
      a[1] += (first[j] - first[i]) * kUs;
      a[5] += (first[j] - last_end[i]) * kUs;
      gap_sum += (first[j] - last_end[i]) * kUs;
      ++gap_n;
    } else {
      last = i;
    }
  }
  if (last < nt) {
    const double gap = gap_n ? gap_sum / gap_n : 0.0;
    acc[(last % n) * TI_STAMP_FIELDS + 1] += (last_end[last] - first[last]) * kUs + gap;
    acc[(last % n) * TI_STAMP_FIELDS + 5] += gap;
  }
  *n_launch = (int)n;
  for (size_t i = 0; i < n && (int)i < cap; ++i) {
    for (int k = 0; k < 3; ++k) info_out[3 * i + k] = info[3 * i + k];
    for (int k = 0; k < TI_STAMP_FIELDS; ++k) t_out[i * TI_STAMP_FIELDS + k] = acc[i * TI_STAMP_FIELDS + k] / steps;
  }
  return TI_OK;
}
