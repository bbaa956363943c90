// engine_guide.cpp -- token-automaton guided decoding as engine state (ti_engine_set_guide): the upload of the
// CSR and the per-state allow-bitmask, the per-slot state row, and the launch the sampled step graphs take.
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

// ti_guide_step on the rows the sampler is about to read (enqueue_step; graph-capturable)
int guide_enqueue(ti_engine* e, int M, StepMode mode) {
  ti_guide_args ga{};
  ga.logits = e->logits;
  ga.ldl = e->c.vocab;
  ga.M = M;
  ga.V = e->c.vocab;
  ga.guide = e->guide;
  ga.state = e->guide_state;
  ga.draw_stride = e->draw_cap;
  ga.advance = mode.advance;
  ga.step_ctr = e->step_ctr;
  ga.n_in = e->n_in;
  ga.out_tokens = e->out_tokens;
  ga.out_stride = e->out_cap;
  ga.carry = mode.carry ? e->pen_carry : nullptr;
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
static int guide_upload(ti_engine* e, const T** dst, const T* src, size_t count) {
  void* p = nullptr;
  TI_TRY(ti_malloc(&p, count * sizeof(T)));
  e->guide_bufs.push_back(p);
  TI_TRY(ti_memcpy_h2d(p, src, count * sizeof(T), e->s));
  *dst = static_cast<const T*>(p);
  return TI_OK;
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
  const int n = g->n_states, W = (c.vocab + 31) / 32;
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
  int rc = guide_upload(e, &d.row_ptr, g->row_ptr, (size_t)n + 1);
  if (rc == TI_OK) rc = guide_upload(e, &d.tokens, g->tokens, nnz);
  if (rc == TI_OK) rc = guide_upload(e, &d.next, g->next, nnz);
  if (rc == TI_OK) rc = guide_upload(e, &d.mask, mask.data(), mask.size());
  if (rc == TI_OK) rc = ti_stream_sync(e->s);   // (the copies read host memory the caller and this frame own)
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

}  // extern "C"
