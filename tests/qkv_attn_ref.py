"""Test helper: a float64 reference of ONE ti_qkv_attn_partials launch, seeded inputs
that make a single wrong key visible, and a host merge of the launch's partials.  numpy only.

The reference knows nothing of the kernel's splits, ring or tile ownership: it is the operation,
    rms     = sqrt(sum(ss) / K + eps)
    q, k, v = (fx @ W) / rms                     W: the dequantized q | k | v weight as the GPU sees it
    q, k    = RoPE at position p, interleaved (even, odd) pairs (tensor_engine.cpp:1602-1612)
    row p of the K / V cache = fp16(k), fp16(v)
    per head: scores q . k_n / sqrt(head_dim) over keys n in [0, p], their logsumexp, softmax . V
in float64 on the fp16 inputs (fx, the caches) exactly as given.  `merge_partials` turns the launch's
part_o / part_ml into the same two per-head quantities (merged row, logsumexp), so a test never has
to know where the kernel put its split bounds.

Inputs (all seeded):
  flat          normal caches, K rows x 0.5 (what test_gpu_qkv_attn.py uses): an almost flat softmax.
  needle(j)     the flat cache with row j replaced: for every kv-head, K row j = c * sum_g q^_g over the
                unit reference q of the group's heads, V row j a fresh normal row.  c (one per kv-head)
                is the smallest value that gives row j a 0.95 share of every head's softmax in the
                reference; callers assert >= 0.9 on the float64 reference before launching
                (`assert_share`).  A kernel that drops, masks or misplaces key j is then off by about
                |v| ~ 1 instead of 1 / p.
  new_key_only  every old K row = -c * sum_g q^_g, so the step's own key p holds >= 0.9 at any p.
Choice for groups whose unit q do not all lean towards their plain sum (a head with q^_g . sum q^ <= 0, or
so small that the row would leave fp16's comfortable range, |element| > DIR_CAP: to be expected at GQA group 16, where q^_g . sum q^ is 1 +- 0.5):
still ONE row per kv-head, but the sum is weighted, sum_g w_g q^_g with w = (Q^ Q^T)^-1 1, the
minimum-norm row with the same cosine to every head of the group (for orthogonal heads w = 1: the plain
sum).  It serves new_key_only too, where one-row-per-head planting cannot (every old row would have to
lean away from every head).  The share is never lowered.

`multiplicity` / `new_row_from` perturb the REFERENCE side (a key counted 0 or 2 times, another
kv-head's new row): how the tests' sensitivity was shown, and what test_qkv_attn_ref.py checks.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

f16, f32, f64 = np.float16, np.float32, np.float64

EPS = 1e-5
SHARE = 0.9                              # the precondition the callers assert
_AIM = float(np.log(0.95 / 0.05))        # margin over the other keys' logsumexp the rows are built for
DIR_CAP = 48.0                           # largest |element| accepted for a planted fp16 K row

# (bits, K, heads, kv_heads, head_dim, splits): the smallest shape per code path of qkv_attn.hip
BASE_SHAPES = [
    (8, 1024, 12, 3, 64, 4),      # <8,64,1,1>, heads not a power of two
    (4, 1024, 8, 4, 64, 4),       # GQA group 2: one k / v tile per workgroup
    (8, 1024, 16, 16, 64, 4),     # hd 64 MHA: two tiles per workgroup (nkv == 2 at runtime)
    (4, 2048, 32, 4, 64, 4),      # <4,64,2,2>
    (8, 2048, 32, 2, 64, 8),      # group 16: kv_tiles < heads
    (4, 2048, 32, 32, 64, 8),     # hd 64 MHA, one tile each
    (8, 2048, 24, 6, 64, 8),      # <8,64,1,2>, heads 24
    (4, 4096, 8, 8, 128, 8),      # hd 128, smallest
    (8, 4096, 24, 24, 128, 8),    # hd 128, heads 24: rcpf(24) in nk_base
]
BENCH_SHAPES = [(8, 2048, 32, 4, 64, 8), (4, 4096, 32, 32, 128, 8)]
ALL_SHAPES = BASE_SHAPES + BENCH_SHAPES


def shape_id(shape) -> str:
    return "w%d-K%d-h%d-kv%d-hd%d-s%d" % tuple(shape)


def shape_seed(shape) -> int:
    bits, K, heads, kv_heads, hd, splits = shape
    return bits * 1000003 + K * 101 + heads * 17 + kv_heads * 7 + hd + splits


# ------------------------------------------------------------------ seeded inputs
def make_weight(shape) -> np.ndarray:
    """The q | k | v weight [K][(heads + 2 kv_heads) head_dim], fp32, before quantization."""
    bits, K, heads, kv_heads, hd, splits = shape
    rng = np.random.default_rng(shape_seed(shape))
    w = rng.standard_normal((K, (heads + 2 * kv_heads) * hd), dtype=f32)
    w *= f32(0.03)
    return w


def dequantized(oracle, w: np.ndarray, bits: int) -> np.ndarray:
    """W as the GPU sees it (test_gpu_kernels.deq): int x fp16 scale, exact in fp32."""
    K, N = w.shape
    out = np.empty((K, N), f32)

    def block(c):   # (groups run along K: column blocks are independent; ctypes calls drop the GIL)
        q, s = oracle.quantize_groups(np.ascontiguousarray(w[:, c:c + 256]), bits)
        out[:, c:c + 256] = oracle.dequantize_groups(q, s)

    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(block, range(0, N, 256)))
    return out


def make_fx(K: int, seed: int) -> np.ndarray:
    return (np.random.RandomState(7000 + seed).standard_normal(K) * 0.5).astype(f16)


def make_ss(K: int, n_ss: int, seed: int, total: float | None = None) -> np.ndarray:
    """n_ss positive partial sums of squares; with `total`, scaled to sum to it."""
    ss = (np.abs(np.random.RandomState(8000 + seed).standard_normal(n_ss)) + 0.05) * (K / n_ss)
    if total is not None:
        ss *= total / ss.sum()
    return ss.astype(f32)


def flat_cache(kv_heads: int, max_seq: int, hd: int, seed: int):
    rng = np.random.RandomState(9000 + seed)
    kc = (rng.standard_normal((kv_heads, max_seq, hd)) * 0.5).astype(f16)
    vc = rng.standard_normal((kv_heads, max_seq, hd)).astype(f16)
    return kc, vc


# ------------------------------------------------------------------ the reference
def project(fx: np.ndarray, wf: np.ndarray, block: int = 1024) -> np.ndarray:
    """fx @ W in float64 (column blocks: no float64 copy of the whole weight)."""
    x = np.asarray(fx).astype(f64)
    out = np.empty(wf.shape[1], f64)
    for c in range(0, wf.shape[1], block):
        out[c:c + block] = x @ wf[:, c:c + block].astype(f64)
    return out


def rope_interleaved(x: np.ndarray, cs_p: np.ndarray) -> np.ndarray:
    """x [..., hd], cs_p [hd / 2][2] (cos, sin) of the position: pairs (2i, 2i + 1)."""
    c, s = cs_p[:, 0].astype(f64), cs_p[:, 1].astype(f64)
    xe, xo = x[..., 0::2], x[..., 1::2]
    out = np.empty_like(x)
    out[..., 0::2] = xe * c - xo * s
    out[..., 1::2] = xo * c + xe * s
    return out


class Proj:
    """rms and the step's q / k / v rows (float64), the new cache rows rounded to fp16."""

    def __init__(self, lin, ss, eps, cs, p, K, heads, kv_heads, hd):
        qd, kvd = heads * hd, kv_heads * hd
        assert lin.shape == (qd + 2 * kvd,)
        self.heads, self.kv_heads, self.hd, self.p = heads, kv_heads, hd, int(p)
        self.rms = float(np.sqrt(np.asarray(ss).astype(f64).sum() / K + float(f32(eps))))
        y = np.asarray(lin, f64) / self.rms
        cs_p = np.asarray(cs).reshape(-1, hd // 2, 2)[p]
        self.q = rope_interleaved(y[:qd].reshape(heads, hd), cs_p)
        self.k = rope_interleaved(y[qd:qd + kvd].reshape(kv_heads, hd), cs_p)
        self.v = y[qd + kvd:].reshape(kv_heads, hd).copy()
        self.k16, self.v16 = self.k.astype(f16), self.v.astype(f16)


class Attn:
    """scores [heads][p + 1], lse [heads], row [heads][hd] over keys [0, p], row p = the fp16 new row."""

    def __init__(self, pr: Proj, kc, vc, multiplicity=None, new_row_from=None):
        heads, kvh, hd, p = pr.heads, pr.kv_heads, pr.hd, pr.p
        g = heads // kvh
        src = np.arange(kvh) if new_row_from is None else np.asarray(new_row_from)
        keys = np.concatenate([np.asarray(kc)[:, :p], pr.k16[src][:, None]], axis=1).astype(f64)
        vals = np.concatenate([np.asarray(vc)[:, :p], pr.v16[src][:, None]], axis=1).astype(f64)
        sc = np.matmul(pr.q.reshape(kvh, g, hd), keys.transpose(0, 2, 1)) / np.sqrt(float(hd))   # [kvh][g][p + 1]
        mult = np.ones(p + 1) if multiplicity is None else np.asarray(multiplicity, f64)
        with np.errstate(divide="ignore"):
            z = sc + np.log(mult)
        m = z.max(axis=-1, keepdims=True)
        e = np.exp(z - m)
        tot = e.sum(axis=-1, keepdims=True)
        self.scores = sc.reshape(heads, p + 1)
        self.lse = (m + np.log(tot)).reshape(heads)
        self.weights = (e / tot).reshape(heads, p + 1)
        self.row = np.matmul(e / tot, vals).reshape(heads, hd)


def launch_ref(lin, ss, eps, cs, p, kc, vc, K, heads, kv_heads, hd, **perturb):
    pr = Proj(lin, ss, eps, cs, p, K, heads, kv_heads, hd)
    return pr, Attn(pr, kc, vc, **perturb)


def merge_partials(part_o, part_ml):
    """part_o [heads][S][hd] (fp16), part_ml [heads][S][2] (max, sum) -> (row [heads][hd],
    lse [heads] = M + log(sum_s l_s e^(m_s - M))), float64."""
    o = np.asarray(part_o).astype(f64)
    m = np.asarray(part_ml)[..., 0].astype(f64)
    l = np.asarray(part_ml)[..., 1].astype(f64)
    live = l > 0
    mm = np.where(live, m, -np.inf)
    M = mm.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(live, l * np.exp(mm - M), 0.0)
    tot = w.sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        row = (w[..., None] * o).sum(axis=1) / tot
        lse = (M + np.log(tot)).reshape(-1)
    return row, lse


def check_partials(part_o, part_ml):
    """Every split is empty (l == 0, m == -inf, a zero row) or live (l > 0, finite m, a finite row)."""
    o = np.asarray(part_o).astype(f64)
    m, l = np.asarray(part_ml)[..., 0], np.asarray(part_ml)[..., 1]
    empty = (l == 0) & np.isneginf(m) & ~o.any(axis=-1)
    live = (l > 0) & np.isfinite(l) & np.isfinite(m) & np.isfinite(o).all(axis=-1)
    assert np.all(empty | live), f"malformed splits at (head, split) {np.argwhere(~(empty | live))[:8].tolist()}"
    assert np.all(live.any(axis=1)), "a head with no live split"


# ------------------------------------------------------------------ planted rows
def _directions(pr: Proj, need: np.ndarray):
    """Per kv-head, the fp16 K row c * sum_g w_g q^_g that gives every head g of the group a score of at
    least need[g] (need may be <= 0), and the c used.  w = 1 where that works, else the minimum-norm
    weights (module docstring)."""
    heads, kvh, hd = pr.heads, pr.kv_heads, pr.hd
    g = heads // kvh
    qn = np.linalg.norm(pr.q, axis=1)
    qhat = (pr.q / qn[:, None]).reshape(kvh, g, hd)
    rows = np.empty((kvh, hd), f16)
    cs_ = np.empty(kvh)
    for i in range(kvh):
        Q = qhat[i]
        nd = need[i * g:(i + 1) * g]
        for w in (np.ones(g), None):
            if w is None:
                w = np.linalg.solve(Q @ Q.T, np.ones(g))
            d = w @ Q
            a = (pr.q[i * g:(i + 1) * g] @ d) / np.sqrt(float(hd))     # score per unit c
            if np.all(a > 0):
                c = max(float(np.max(nd / a)), 0.05)
                if np.abs(c * d).max() <= DIR_CAP:
                    break
        else:
            raise AssertionError(f"kv-head {i}: no fp16 row reaches the share")
        rows[i] = (c * d * (1 + 2.0 ** -9)).astype(f16)     # (a hair over: fp16 rounding of the row cannot undershoot)
        cs_[i] = c
    return rows, cs_


def needle_rows(pr: Proj, flat: Attn, j: int, seed: int):
    """K / V rows [kv_heads][hd] (fp16) for row j of the flat cache, 0 <= j < p; `flat` is the
    reference on the flat cache at the same p."""
    assert 0 <= j < pr.p
    sc = flat.scores
    oth = np.delete(sc, j, axis=1)
    m = oth.max(axis=1)
    lse_oth = m + np.log(np.exp(oth - m[:, None]).sum(axis=1))
    krow, _ = _directions(pr, lse_oth + _AIM)
    vrow = np.random.RandomState(10000 + 131 * seed + j).standard_normal((pr.kv_heads, pr.hd)).astype(f16)
    return krow, vrow


def new_key_only_row(pr: Proj):
    """The K row [kv_heads][hd] (fp16) every OLD position gets, so that key p holds the share (p >= 1)."""
    g = pr.heads // pr.kv_heads
    s_new = np.einsum("hd,hd->h", pr.q, np.repeat(pr.k16.astype(f64), g, axis=0)) / np.sqrt(float(pr.hd))
    need = _AIM + np.log(float(pr.p)) - s_new       # old scores are -c a_g: c a_g >= need
    krow, _ = _directions(pr, need)
    return (-krow.astype(f32)).astype(f16)


def assert_share(at: Attn, key: int, share: float = SHARE):
    w = at.weights[:, key]
    assert np.all(w >= share), f"key {key} holds only {w.min():.3f} of head {int(w.argmin())}'s softmax"
