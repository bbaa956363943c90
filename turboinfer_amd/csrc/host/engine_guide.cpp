// engine_guide.cpp -- token-automaton guided decoding as engine state (ti_engine_set_guide) and as a library of
// guides that requests name by handle (ti_engine_add_guide, ti_engine_serve_requests_guided): the upload of the CSR
// and the per-state allow-bitmask, the per-slot state row, and the launch the sampled step graphs take.
#include "engine_impl.hpp"

using namespace ti_eng;

namespace ti_eng {

// The entry points that produce tokens without the sampled step graph cannot follow a guide.
int guide_refuse(const ti_engine* e, const char* fn) {
  if (!e->guide_active()) return TI_OK;
  return ti_set_error(TI_ERR_UNSUPPORTED, "%s: a guide is set (ti_engine_set_guide); only ti_engine_generate_sampled "
                      "and ti_engine_serve_sampled apply it", fn);
}

// Slots [first, first + count) start a request: their state becomes the guide's start state.
int guide_start_slots(ti_engine* e, int first, int count) {
  return ti_guide_reset(e->guide_state, first, count, e->guide_start, e->s);
}

// Slot `slot` starts a request of ti_engine_serve_requests_guided: the start state of its library guide, or -1
// (free) for a request without one.
int guide_reset_slot(ti_engine* e, int slot, int handle) {
  return ti_guide_reset(e->guide_state, slot, 1, handle > 0 ? e->guide_lib[handle - 1].start : -1, e->s);
}

// ti_guide_step on the rows the sampler is about to read (enqueue_step; graph-capturable); with mode.rows_guide
// ti_guide_step_rows over the library's table, each row's handle in e->row_params
int guide_enqueue(ti_engine* e, int M, StepMode mode) {
  ti_guide_args ga{};
  ga.logits = e->logits;
  ga.ldl = e->c.vocab;
  ga.M = M;
  ga.V = e->c.vocab;
  if (!mode.rows_guide) ga.guide = e->guide;
  ga.state = e->guide_state;
  ga.draw_stride = e->draw_cap;
  ga.advance = mode.advance;
  ga.step_ctr = e->step_ctr;
  ga.n_in = e->n_in;
  ga.out_tokens = e->out_tokens;
  ga.out_stride = e->out_cap;
  ga.carry = mode.carry ? e->pen_carry : nullptr;
  if (mode.rows_guide) return ti_guide_step_rows(&ga, e->guide_table, TI_GUIDE_CAP, e->row_params, e->s);
  return ti_guide_step(&ga, e->s);
}

static int guide_free(ti_engine* e) {
  for (void* p : e->guide_bufs) E_CHECK(hipFree(p), "hipFree(guide)");
  e->guide_bufs.clear();
  e->guide = ti_guide_dev{};
  e->guide_start = 0;
  return TI_OK;
}

template <class T>
static int guide_upload(ti_engine* e, std::vector<void*>& bufs, const T** dst, const T* src, size_t count) {
  void* p = nullptr;
  TI_TRY(ti_malloc(&p, count * sizeof(T)));
  bufs.push_back(p);
  TI_TRY(ti_memcpy_h2d(p, src, count * sizeof(T), e->s));
  *dst = static_cast<const T*>(p);
  return TI_OK;
}

// A checked guide on the device: its CSR and the per-state allow-bitmask, in buffers appended to `bufs` (the
// caller frees them, also after an error); returns once the copies have read the host arrays.
static int guide_to_device(ti_engine* e, const ti_guide* g, std::vector<void*>& bufs, ti_guide_dev* out) {
  const int n = g->n_states, W = (e->c.vocab + 31) / 32;
  const size_t nnz = (size_t)g->row_ptr[n];
  std::vector<uint32_t> mask((size_t)n * W, 0u);
  for (int s = 0; s < n; ++s)
    for (int64_t i = g->row_ptr[s]; i < g->row_ptr[s + 1]; ++i) {
      const int32_t v = g->tokens[i];
      mask[(size_t)s * W + (v >> 5)] |= 1u << (v & 31);
    }
  ti_guide_dev d{};
  d.n_states = n;
  d.mask_words = W;
  TI_TRY(guide_upload(e, bufs, &d.row_ptr, g->row_ptr, (size_t)n + 1));
  TI_TRY(guide_upload(e, bufs, &d.tokens, g->tokens, nnz));
  TI_TRY(guide_upload(e, bufs, &d.next, g->next, nnz));
  TI_TRY(guide_upload(e, bufs, &d.mask, mask.data(), mask.size()));
  TI_TRY(ti_stream_sync(e->s));   // (the copies read host memory the caller and this frame own)
  *out = d;
  return TI_OK;
}

static int free_bufs(std::vector<void*>& bufs) {
  int rc = TI_OK;
  for (void* p : bufs)
    if (hipFree(p) != hipSuccess) rc = ti_set_error(TI_ERR_HIP, "hipFree(guide)");
  bufs.clear();
  return rc;
}

}  // namespace ti_eng

extern "C" {

int ti_engine_set_guide(ti_engine* e, const ti_guide* g) {
  const char* fn = "ti_engine_set_guide";
  if (!e) return ti_set_error(TI_ERR_ARG, "%s: null", fn);
  if (e->c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "%s: compat engine", fn);
  const ti_engine_config& c = e->c;
  if (g) TI_TRY(ti_guide_check(g, c.vocab));
  if (!g && !e->guide_active()) return TI_OK;
  DeviceScope bind_(e);
  TI_TRY(drop_graphs(e));   // the step graphs bake the guide's buffers in (synchronises the stream)
  TI_TRY(guide_free(e));
  if (!e->guide_state) TI_TRY(e->alloc_t(&e->guide_state, (size_t)c.max_batch));
  if (!e->pen_carry) TI_TRY(e->alloc_t(&e->pen_carry, (size_t)c.max_batch));
  TI_TRY(ti_guide_reset(e->guide_state, 0, c.max_batch, -1, e->s));
  if (!g) return ti_stream_sync(e->s);
  ti_guide_dev d{};
  const int rc = guide_to_device(e, g, e->guide_bufs, &d);
  if (rc != TI_OK) {
    guide_free(e);
    return rc;
  }
  e->guide = d;
  e->guide_start = g->start;
  return TI_OK;
}

int ti_engine_guide_states(ti_engine* e, int32_t* out) {
  if (!e || !out) return ti_set_error(TI_ERR_ARG, "ti_engine_guide_states: null");
  if (!e->guide_state) {
    std::fill(out, out + e->c.max_batch, -1);
    return TI_OK;
  }
  DeviceScope bind_(e);
  return ti_memcpy_d2h(out, e->guide_state, (size_t)e->c.max_batch * 4, e->s);   // (synchronises the stream)
}

int ti_engine_add_guide(ti_engine* e, const ti_guide* g, int* out_handle) {
  const char* fn = "ti_engine_add_guide";
  if (!e || !g || !out_handle) return ti_set_error(TI_ERR_ARG, "%s: null", fn);
  if (e->c.compat) return ti_set_error(TI_ERR_UNSUPPORTED, "%s: compat engine", fn);
  const ti_engine_config& c = e->c;
  TI_TRY(ti_guide_check(g, c.vocab));
  DeviceScope bind_(e);
  if (!e->guide_table) {   // zeroed: every entry unused (new buffers, which no captured graph has baked in)
    TI_TRY(e->alloc_t(&e->guide_table, (size_t)TI_GUIDE_CAP));
    e->guide_lib.assign(TI_GUIDE_CAP, ti_engine::LibGuide{});
  }
  if (!e->guide_state) {
    TI_TRY(e->alloc_t(&e->guide_state, (size_t)c.max_batch));
    TI_TRY(ti_guide_reset(e->guide_state, 0, c.max_batch, -1, e->s));
  }
  if (!e->pen_carry) TI_TRY(e->alloc_t(&e->pen_carry, (size_t)c.max_batch));
  int h = 0;
  while (h < TI_GUIDE_CAP && e->guide_lib[h].live) ++h;
  if (h == TI_GUIDE_CAP) return ti_set_error(TI_ERR_ARG, "%s: the library holds TI_GUIDE_CAP = %d guides", fn, TI_GUIDE_CAP);
  ti_engine::LibGuide& slot = e->guide_lib[h];
  ti_guide_dev d{};
  int rc = guide_to_device(e, g, slot.bufs, &d);
  // the one entry, in stream order behind whatever step still reads the table; d is this frame's: wait for the copy
  if (rc == TI_OK) rc = ti_memcpy_h2d(e->guide_table + h, &d, sizeof(d), e->s);
  if (rc == TI_OK) rc = ti_stream_sync(e->s);
  if (rc != TI_OK) {
    free_bufs(slot.bufs);
    return rc;
  }
  slot.live = true;
  slot.start = g->start;
  *out_handle = h + 1;
  return TI_OK;
}

int ti_engine_remove_guide(ti_engine* e, int handle) {
  const char* fn = "ti_engine_remove_guide";
  if (!e) return ti_set_error(TI_ERR_ARG, "%s: null", fn);
  if (handle < 0 || handle > TI_GUIDE_CAP)
    return ti_set_error(TI_ERR_ARG, "%s: handle %d not in [0, TI_GUIDE_CAP %d]", fn, handle, TI_GUIDE_CAP);
  if (handle > 0 && (e->guide_lib.empty() || !e->guide_lib[handle - 1].live))
    return ti_set_error(TI_ERR_ARG, "%s: handle %d is not live", fn, handle);
  if (e->guide_lib.empty()) return TI_OK;   // (0 on an empty library)
  DeviceScope bind_(e);
  TI_TRY(ti_stream_sync(e->s));   // no step in flight reads the entries about to go
  const int lo = handle ? handle - 1 : 0, hi = handle ? handle : TI_GUIDE_CAP;
  E_CHECK(hipMemsetAsync(e->guide_table + lo, 0, (size_t)(hi - lo) * sizeof(ti_guide_dev), e->s), "hipMemsetAsync(guide table)");
  TI_TRY(ti_stream_sync(e->s));   // a zeroed entry is inert (ti_guide_step_rows): its buffers can go
  int rc = TI_OK;
  for (int h = lo; h < hi; ++h) {
    ti_engine::LibGuide& slot = e->guide_lib[h];
    const int r = free_bufs(slot.bufs);
    if (rc == TI_OK) rc = r;
    slot = ti_engine::LibGuide{};
  }
  return rc;
}

int ti_engine_guide_count(ti_engine* e, int* out) {
  if (!e || !out) return ti_set_error(TI_ERR_ARG, "ti_engine_guide_count: null");
  *out = (int)std::count_if(e->guide_lib.begin(), e->guide_lib.end(), [](const ti_engine::LibGuide& g) { return g.live; });
  return TI_OK;
}

}  // extern "C"
