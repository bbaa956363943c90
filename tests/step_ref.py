"""Plain numpy models of the two kernels the device loop is built on (include/ti_hip.h):

  ti_step_begin     (step_begin_kernel, kernels/misc.hip)  -> step_begin_ref
  ti_kv_copy_slots  (kv_copy_kernel,    kernels/misc.hip)  -> kv_copy_ref

and of the two key encodings ti_step_begin reads: the lm_head's TI_EPI_LOGITS_ARGMAX key (logit_key) and
ti_sample_step's feedback key (sampled_key).  Nothing here touches a device; tests/test_step_ref.py pins the
models to hand-written cases and shows that the compare helpers reject each way the kernels could be subtly
wrong, and the GPU tests (test_gpu_step_begin.py, test_gpu_kv_copy.py) compare the kernels with them.

The rules of one ti_step_begin launch at step s (= *step_ctr), row m of M:
  key    = max of the row's TI_ARGMAX_SLOTS slots; its token 0xFFFFFFFF - (key & 0xFFFFFFFF) as an int32, so
           equal values at two indices give the lower index and an all-zero row gives -1
  s <  n_in[m]:  the token is in_tokens[m][s]; out_tokens is not written
  s >= n_in[m]:  the token is the key's, written unclamped to out_tokens[m][s - n_in[m]] when that index is
                 below out_stride (n_in NULL: n_in[m] = 0)
  gather token 0 when the token is outside [0, vocab)
  pos[m] = base_pos[m] + s; all slots of the row become 0
  h[m]   = the embedding row's fp16 values as fp32 (exact), or with placeholder_first >= 0
           float32(0.1) * float32((off + i) % 100), off = placeholder_first at s == 0 and 0 afterwards
  fold_x = float16(h * fold_w), the product taken in fp32 and rounded once; fold_ss = sum h^2
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

SLOTS = 32          # TI_ARGMAX_SLOTS
SS_RTOL = 1e-5      # fold_ss against the float64 sum (test_gpu_batched.py test_batched_fold_producer_consumer)


# ------------------------------------------------------------------ keys
def logit_key(value, index) -> int:
    """The lm_head's TI_EPI_LOGITS_ARGMAX key (float_order_key in kernels/gemv.hip): the order-preserving bits
    of the fp32 logit in the high word (a negative value's pattern inverted, a non-negative one's sign bit set;
    -0.0 therefore ranks just below +0.0), 0xFFFFFFFF - index in the low word."""
    u = int(np.array(value, np.float32).view(np.uint32))
    hi = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    return (hi << 32) | (0xFFFFFFFF - int(index))


def sampled_key(token) -> int:
    """ti_sample_step's feedback key: high word all ones (above every logit key), 0xFFFFFFFF - token below."""
    return (0xFFFFFFFF << 32) | (0xFFFFFFFF - int(token))


def key_token(key) -> int:
    """The token of a key, as the int32 the kernel computes."""
    t = (0xFFFFFFFF - (int(key) & 0xFFFFFFFF)) & 0xFFFFFFFF
    return t - (1 << 32) if t & 0x80000000 else t


# ------------------------------------------------------------------ step begin
@dataclass
class StepCase:
    """One launch's inputs, mirroring ti_step_args."""
    argmax: np.ndarray                         # uint64 [M][SLOTS], before the launch
    base_pos: np.ndarray                       # int32 [M]
    s: int                                     # *step_ctr
    emb: Optional[np.ndarray] = None           # float16 [vocab][hidden]; None with a placeholder
    hidden: int = 0                            # taken from emb when given
    vocab: int = 0                             # taken from emb when given
    in_tokens: Optional[np.ndarray] = None     # int32 [M][in_stride]
    n_in: Optional[np.ndarray] = None          # int32 [M]; None = NULL
    out_stride: int = 0
    out_tokens: Optional[np.ndarray] = None    # int32 [M][out_stride], before the launch; None = NULL
    placeholder_first: int = -1
    fold_w: Optional[np.ndarray] = None        # float32 [hidden]; given = fold_x / fold_ss are produced

    def __post_init__(self):
        if self.emb is not None:
            assert self.emb.dtype == np.float16 and self.emb.ndim == 2
            self.vocab, self.hidden = self.emb.shape
        self.argmax = np.asarray(self.argmax, np.uint64).reshape(-1, SLOTS)
        self.base_pos = np.asarray(self.base_pos, np.int32).reshape(-1)
        assert self.argmax.shape[0] == self.base_pos.size

    @property
    def M(self) -> int:
        return self.base_pos.size

    def at(self, **kw) -> "StepCase":
        return replace(self, **kw)


@dataclass
class StepResult:
    h: np.ndarray                      # float32 [M][hidden]
    pos: np.ndarray                    # int32 [M]
    out_tokens: Optional[np.ndarray]   # int32 [M][out_stride] after the launch
    argmax: np.ndarray                 # uint64 [M][SLOTS] after the launch
    fold_x: Optional[np.ndarray]       # float16 [M][hidden]
    fold_ss: Optional[np.ndarray]      # [M]: float64 from the model, float32 from the device
    tokens: Optional[np.ndarray] = None   # int32 [M]: the gathered rows (model only; not compared)


class StepModel:
    """step_begin_ref, one overridable method per rule (tests/test_step_ref.py derives its mutants from it)."""

    def row_key(self, slots: np.ndarray) -> int:
        return int(slots.max())

    def key_token(self, key: int) -> int:
        return key_token(key)

    def record_index(self, s: int, nin: int, out_stride: int) -> Optional[int]:
        """Where in out_tokens[m] the step's token is recorded; None = not recorded."""
        return s - nin if 0 <= s - nin < out_stride else None

    def gather_token(self, tok: int, vocab: int) -> int:
        return tok if 0 <= tok < vocab else 0

    def pos(self, base: int, s: int) -> int:
        return base + s

    def cleared(self, slots: np.ndarray) -> np.ndarray:
        return np.zeros_like(slots)

    def fold_x(self, h: np.ndarray, w: np.ndarray) -> np.ndarray:
        return (h.astype(np.float32) * w.astype(np.float32)).astype(np.float16)

    def fold_ss(self, h: np.ndarray) -> float:
        return float(np.sum(h.astype(np.float64) ** 2))

    def run(self, c: StepCase) -> StepResult:
        M, H = c.M, c.hidden
        h = np.empty((M, H), np.float32)
        pos = np.empty(M, np.int32)
        out = None if c.out_tokens is None else np.array(c.out_tokens, np.int32).reshape(M, c.out_stride)
        argmax = np.empty_like(c.argmax)
        toks = np.empty(M, np.int32)
        for m in range(M):
            nin = 0 if c.n_in is None else int(c.n_in[m])
            if c.s < nin:
                tok = int(c.in_tokens[m][c.s])
            else:
                tok = self.key_token(self.row_key(c.argmax[m]))
            idx = self.record_index(c.s, nin, c.out_stride)
            if out is not None and idx is not None and m * c.out_stride + idx < out.size:
                out.reshape(-1)[m * c.out_stride + idx] = tok   # flat, as the kernel indexes it
            toks[m] = self.gather_token(tok, c.vocab)
            pos[m] = self.pos(int(c.base_pos[m]), c.s)
            argmax[m] = self.cleared(c.argmax[m])
            if c.placeholder_first >= 0:
                off = c.placeholder_first if c.s == 0 else 0
                h[m] = np.float32(0.1) * ((off + np.arange(H, dtype=np.int64)) % 100).astype(np.float32)
            else:
                h[m] = self.emb_row(c, int(toks[m]))
        fx = fss = None
        if c.fold_w is not None:
            fx = np.stack([self.fold_x(h[m], c.fold_w) for m in range(M)])
            fss = np.array([self.fold_ss(h[m]) for m in range(M)], np.float64)
        return StepResult(h, pos, out, argmax, fx, fss, toks)

    def emb_row(self, c: StepCase, tok: int) -> np.ndarray:
        return c.emb[tok].astype(np.float32)


def step_begin_ref(case: StepCase) -> StepResult:
    return StepModel().run(case)


def double_rounding_input(n=1 << 18):
    """(v fp16, w fp32) pairs whose fp32 product rounds to another fp16 than their exact product does."""
    rng = np.random.RandomState(5)
    v = rng.standard_normal(n).astype(np.float16)
    w = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    once = (v.astype(np.float64) * w.astype(np.float64)).astype(np.float16)     # 35-bit product: exact in float64
    twice = (v.astype(np.float32) * w).astype(np.float16)
    hit = np.flatnonzero(once.view(np.uint16) != twice.view(np.uint16))
    return v[hit], w[hit]


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def assert_step_equal(got: StepResult, ref: StepResult) -> None:
    """Everything bit for bit, except fold_ss within SS_RTOL of the float64 sum."""
    for name in ("h", "pos", "out_tokens", "argmax", "fold_x", "fold_ss"):
        g, r = getattr(got, name), getattr(ref, name)
        assert (g is None) == (r is None), f"{name}: present on one side only"
        if g is None:
            continue
        g, r = np.asarray(g), np.asarray(r)
        assert g.shape == r.shape, f"{name}: shape {g.shape} != {r.shape}"
        if name == "fold_ss":
            g64, r64 = g.astype(np.float64), r.astype(np.float64)
            ok = np.isfinite(g64) & (np.abs(g64 - r64) <= SS_RTOL * np.abs(r64))
            assert ok.all(), f"fold_ss: rows {np.flatnonzero(~ok)[:4]} got {g64[~ok][:4]} want {r64[~ok][:4]}"
            continue
        if name in ("h", "fold_x"):
            assert g.dtype == r.dtype, f"{name}: dtype {g.dtype} != {r.dtype}"
            g, r = _bits(g), _bits(r)
        bad = np.argwhere(g != r)
        assert bad.size == 0, (f"{name}: {len(bad)} of {g.size} differ, first at {tuple(bad[0])}: "
                               f"got {g[tuple(bad[0])]} want {r[tuple(bad[0])]}")


# ------------------------------------------------------------------ KV slot copy
def kv_copy_ref(buffers, src_off, dst_off, rows, row_pitch, row_elems):
    """ti_kv_copy_slots on host copies of the caches (uint16 arrays, one per table entry): in every buffer,
    `rows` rows of row_elems elements, row r at r * row_pitch, from element src_off to dst_off.  The whole
    source is read before any destination is written.  Returns new arrays."""
    out = []
    for b in buffers:
        b = np.asarray(b)
        assert b.dtype == np.uint16 and b.ndim == 1
        src = [b[src_off + r * row_pitch: src_off + r * row_pitch + row_elems].copy() for r in range(rows)]
        assert all(s.size == row_elems for s in src), "source outside the buffer"
        o = b.copy()
        for r in range(rows):
            at = dst_off + r * row_pitch
            assert at >= 0 and at + row_elems <= o.size, "destination outside the buffer"
            o[at: at + row_elems] = src[r]
        out.append(o)
    return out


def index_hash(n: int, salt: int = 0) -> np.ndarray:
    """uint16 [n]: no two elements of an aligned block of 65536 equal (an odd multiplier permutes the low 16
    bits), blocks and buffers told apart by the mixed-in high bits and `salt`."""
    i = np.arange(n, dtype=np.uint64)
    return (((i * np.uint64(40503)) ^ ((i >> np.uint64(16)) * np.uint64(0x9E37)) ^ np.uint64(salt * 0x6B43))
            & np.uint64(0xFFFF)).astype(np.uint16)


def assert_buffers_equal(got, ref) -> None:
    assert len(got) == len(ref)
    for t, (g, r) in enumerate(zip(got, ref)):
        g, r = np.asarray(g), np.asarray(r)
        assert g.shape == r.shape and g.dtype == r.dtype, f"buffer {t}: {g.dtype}{g.shape} != {r.dtype}{r.shape}"
        bad = np.flatnonzero(g != r)
        assert bad.size == 0, (f"buffer {t}: {bad.size} elements differ, first at {bad[0]} (got {g[bad[0]]}, "
                               f"want {r[bad[0]]}), last at {bad[-1]}")
