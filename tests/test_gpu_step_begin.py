"""ti_step_begin (step_begin_kernel, kernels/misc.hip) against the numpy model of tests/step_ref.py.

Every buffer the launch may write starts from a fill pattern with guard bytes on both sides and is compared in
full with the model's, bit for bit; the only inexact comparison is fold_ss (rtol 1e-5 of the float64 sum).  The
embedding table always sits between two sentinel rows inside a larger allocation, so a gather that misses its
clamp reads a sentinel and fails the comparison instead of leaving the allocation.  Inputs are checked to be
unchanged.  The hand-shake tests cross the two key encodings the kernel reads with their real writers: the
lm_head's TI_EPI_LOGITS_ARGMAX epilogue and ti_sample_step."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from step_ref import (SLOTS, StepCase, StepResult, assert_step_equal, double_rounding_input, logit_key, sampled_key,
                      step_begin_ref)

pytestmark = pytest.mark.gpu

f16, f32 = np.float16, np.float32
GUARD = 64          # bytes on each side of every buffer
FILL = 0xA5
VOCAB = 11
SENTINEL = (1234.0, -4321.0)   # the rows before and after the table


class Guarded:
    """A device array inside a larger allocation: GUARD bytes of FILL before and after it."""

    def __init__(self, ti, init: np.ndarray, lead: int = 0):
        """lead: bytes of `init` in front of where .ptr points (the table's first sentinel row)."""
        init = np.ascontiguousarray(init)
        self.ti, self.dtype, self.shape, self.n = ti, init.dtype, init.shape, init.nbytes
        g = np.full(GUARD, FILL, np.uint8)
        self.host0 = np.concatenate([g, init.reshape(-1).view(np.uint8), g])
        self.buf = ti.DeviceBuffer.from_array(self.host0)
        self.ptr = self.buf.ptr + GUARD + lead

    def at(self, byte_offset: int) -> int:
        return self.ptr + byte_offset

    def read(self) -> np.ndarray:
        raw = self.buf.download(np.uint8, self.host0.size)
        assert np.all(raw[:GUARD] == FILL) and np.all(raw[GUARD + self.n:] == FILL), "a guard byte was written"
        return raw[GUARD:GUARD + self.n].view(self.dtype).reshape(self.shape).copy()

    def unchanged(self) -> bool:
        return np.array_equal(self.buf.download(np.uint8, self.host0.size), self.host0)


def filled(shape, dtype) -> np.ndarray:
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype).reshape(shape)


def table(emb: np.ndarray) -> np.ndarray:
    """The embedding table between its two sentinel rows."""
    H = emb.shape[1]
    return np.concatenate([np.full((1, H), SENTINEL[0], f16), emb, np.full((1, H), SENTINEL[1], f16)])


class DeviceStep:
    """The buffers of one StepCase on the device and its ti_step_args; launch() then result()."""

    def __init__(self, ti, case: StepCase, fold_x: bool | None = None, fold_w: bool | None = None):
        """fold_x / fold_w: pass the pointer or NULL regardless of the case (the refusal tests)."""
        self.ti, self.case = ti, case
        M, H = case.M, case.hidden
        fold = case.fold_w is not None
        self.inputs, a = {}, ti.StepArgs()
        if case.emb is not None:
            self.inputs["emb"] = Guarded(ti, table(case.emb), lead=2 * H)
            a.emb = self.inputs["emb"].ptr
        for name in ("in_tokens", "n_in", "base_pos", "fold_w"):
            v = getattr(case, name)
            if v is not None:
                self.inputs[name] = Guarded(ti, np.ascontiguousarray(v, f32 if name == "fold_w" else np.int32))
        self.ctr = self.inputs["step_ctr"] = Guarded(ti, np.array([case.s], np.int32))
        self.h = Guarded(ti, filled((M, H), f32))
        self.pos = Guarded(ti, filled(M, np.int32))
        self.argmax = Guarded(ti, case.argmax)
        self.out = None if case.out_tokens is None else Guarded(ti, np.asarray(case.out_tokens, np.int32))
        self.fx = Guarded(ti, filled((M, H), f16)) if fold or fold_x else None
        self.ss = Guarded(ti, filled(M, f32)) if fold or fold_x else None
        a.h, a.hidden, a.M, a.vocab = self.h.ptr, H, M, case.vocab
        a.in_stride = 0 if case.in_tokens is None else np.asarray(case.in_tokens).reshape(M, -1).shape[1]
        a.out_stride, a.placeholder_first = case.out_stride, case.placeholder_first
        a.in_tokens = self.inputs["in_tokens"].ptr if "in_tokens" in self.inputs else None
        a.n_in = self.inputs["n_in"].ptr if "n_in" in self.inputs else None
        a.argmax, a.pos, a.base_pos, a.step_ctr = self.argmax.ptr, self.pos.ptr, self.inputs["base_pos"].ptr, self.ctr.ptr
        a.out_tokens = self.out.ptr if self.out else None
        a.fold_w = self.inputs["fold_w"].ptr if "fold_w" in self.inputs and fold_w is not False else None
        a.fold_x = self.fx.ptr if self.fx and fold_x is not False else None
        a.fold_ss = self.ss.ptr if self.ss and fold_x is not False else None
        self.args = a

    def launch(self) -> int:
        rc = self.ti.lib().ti_step_begin(C.byref(self.args), None)
        self.ti.sync()
        return rc

    def outputs(self):
        return [b for b in (self.h, self.pos, self.argmax, self.out, self.fx, self.ss) if b is not None]

    def result(self) -> StepResult:
        for name, b in self.inputs.items():
            assert b.unchanged(), f"the launch wrote its input {name}"
        fold = self.case.fold_w is not None
        return StepResult(self.h.read(), self.pos.read(), self.out.read() if self.out else None, self.argmax.read(),
                          self.fx.read() if fold else None, self.ss.read() if fold else None)


def run(ti, case: StepCase) -> StepResult:
    d = DeviceStep(ti, case)
    assert d.launch() == 0, ti.lib().ti_last_error()
    return d.result()


def check(ti, case: StepCase) -> StepResult:
    ref = step_begin_ref(case)
    assert_step_equal(run(ti, case), ref)
    return ref


def keys(M, *entries) -> np.ndarray:
    """uint64 [M][SLOTS], zero except (row, slot, key) entries."""
    a = np.zeros((M, SLOTS), np.uint64)
    for m, slot, key in entries:
        a[m, slot] = key
    return a


def embedding(hidden, seed=0) -> np.ndarray:
    return np.random.RandomState(1000 + hidden + seed).standard_normal((VOCAB, hidden)).astype(f16)


def norm_w(hidden) -> np.ndarray:
    return (1 + 0.1 * np.random.RandomState(2000 + hidden).standard_normal(hidden)).astype(f32)


# ------------------------------------------------------------------ gather paths
@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("hidden", [8, 2048, 2056, 8192, 8200, 100, 4100])
def test_gather_paths(ti, hidden, M, fold):
    """The 16-byte path at one piece in all (8), one per thread (2048), a second piece for thread 0 alone (2056)
    and its last size (8192); the scalar path past the limit (8200) and at sizes that are no multiple of 8.
    Step 0 feeds prompt tokens, step 1 a prompt token and fed-back keys; tokens 0 and vocab - 1 both occur."""
    in_tokens = np.array([[0, VOCAB - 1], [VOCAB - 1, 4], [7, 0]], np.int32)[:M]
    n_in = np.array([2, 1, 1], np.int32)[:M]
    am = keys(3, (1, 17, logit_key(0.5, VOCAB - 1)), (1, 2, logit_key(0.25, 3)), (2, 31, logit_key(-1.0, 0)))[:M]
    case = StepCase(argmax=am, base_pos=[5, 0, 300][:M], s=0, emb=embedding(hidden), in_tokens=in_tokens, n_in=n_in,
                    out_stride=2, out_tokens=filled((M, 2), np.int32), fold_w=norm_w(hidden) if fold else None)
    ref = check(ti, case)
    assert ref.tokens.tolist() == [0, VOCAB - 1, 7][:M]
    ref = check(ti, case.at(s=1))
    assert ref.tokens.tolist() == [VOCAB - 1, VOCAB - 1, 0][:M]


@pytest.mark.parametrize("hidden", [2056, 100], ids=["vector", "scalar"])
def test_fold_small_and_signed_values(ti, hidden):
    """fold_x = float16(h * fold_w) where the product is an fp16 subnormal, rounds to zero, is -0.0, or sits on the
    fp16 rounding boundary in fp32 but not exactly (test_step_ref.py's double-rounding inputs): one rounding, of
    the fp32 product, to nearest even."""
    v, w = double_rounding_input()
    assert v.size >= 8
    emb, fw = embedding(hidden, seed=1), norm_w(hidden)
    small = np.array([6e-8, 3.05e-5, 6.1e-5, -0.0, 0.0, -6e-8, 2e-6, -4.7e-5, 1e-3, 65504.0 / 4096], f16)
    for t in range(VOCAB):
        emb[t, 8:8 + small.size] = small * f16(1 + t)
        emb[t, 40:48] = v[:8]
    fw[40:48] = w[:8]
    fw[8:8 + small.size] *= f32(0.37)
    case = StepCase(argmax=keys(2, (1, 5, logit_key(2.0, 9))), base_pos=[0, 1], s=0, emb=emb, n_in=np.array([1, 0], np.int32),
                    in_tokens=np.array([[3], [0]], np.int32), fold_w=fw)
    ref = check(ti, case)
    assert ref.tokens.tolist() == [3, 9]
    exact = (emb[3, 40:48].astype(np.float64) * fw[40:48].astype(np.float64)).astype(f16)
    assert np.all(ref.fold_x[0, 40:48] != exact)       # the inputs do tell one rounding from two


# ------------------------------------------------------------------ token out of range
@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("hidden", [8, 100], ids=["vector", "scalar"])
def test_token_out_of_range_gathers_row_0(ti, hidden, fold):
    """Prompt tokens -1 and vocab, an all-zero argmax row (token -1) and a key for index vocab: each gathers row 0
    -- a missing clamp would read one of the sentinel rows, still inside the allocation -- and the fed-back rows
    record the key's own token."""
    M = 4
    in_tokens = np.array([[-1], [VOCAB], [0], [0]], np.int32)
    n_in = np.array([1, 1, 0, 0], np.int32)
    am = keys(M, (3, 9, logit_key(1.0, VOCAB)), (0, 0, logit_key(1.0, 2)))
    case = StepCase(argmax=am, base_pos=np.arange(M), s=0, emb=embedding(hidden), in_tokens=in_tokens, n_in=n_in,
                    out_stride=1, out_tokens=filled((M, 1), np.int32), fold_w=norm_w(hidden) if fold else None)
    ref = check(ti, case)
    assert ref.tokens.tolist() == [0] * M
    fill = int(filled(1, np.int32)[0])
    assert ref.out_tokens.reshape(-1).tolist() == [fill, fill, -1, VOCAB]
    assert np.array_equal(ref.h, np.tile(case.emb[0].astype(f32), (M, 1)))


# ------------------------------------------------------------------ token choice
def test_token_choice(ti):
    """Keys in the lm_head's encoding scattered over a row's slots; one row per rule."""
    rows = [
        ("the maximum in slot 31 only", [(31, logit_key(3.0, 6)), (0, logit_key(2.5, 1)), (30, logit_key(-1.0, 0))], 6),
        ("equal values at indices 7 and 3", [(4, logit_key(1.5, 7)), (19, logit_key(1.5, 3)), (5, logit_key(1.25, 0))], 3),
        ("equal values, the lower index in the later slot", [(2, logit_key(1.5, 9)), (29, logit_key(1.5, 8))], 8),
        # the lm_head's key keeps the sign of zero: +0.0 ranks above -0.0 whatever their indices
        ("-0.0 at index 2 against +0.0 at index 9", [(7, logit_key(-0.0, 2)), (8, logit_key(0.0, 9))], 9),
        ("-0.0 at both", [(7, logit_key(-0.0, 5)), (1, logit_key(-0.0, 4))], 4),
        ("negative values only", [(3, logit_key(-7.0, 1)), (12, logit_key(-0.5, 10)), (13, logit_key(-np.inf, 0))], 10),
        ("a sampled key next to a larger logit", [(0, sampled_key(5)), (6, logit_key(np.inf, 2)), (1, logit_key(9.0, 0))], 5),
        ("one key, the rest empty", [(16, logit_key(-3.0, 1))], 1),
    ]
    M = len(rows)
    am = keys(M, *[(m, slot, key) for m, (_, entries, _) in enumerate(rows) for slot, key in entries])
    case = StepCase(argmax=am, base_pos=np.zeros(M), s=0, emb=embedding(8), out_stride=1,
                    out_tokens=filled((M, 1), np.int32))
    ref = step_begin_ref(case)
    assert ref.tokens.tolist() == [want for _, _, want in rows]
    got = run(ti, case)
    for m, (name, _, want) in enumerate(rows):
        assert got.out_tokens[m, 0] == want, name
    assert_step_equal(got, ref)


# ------------------------------------------------------------------ prompt against feedback, out_stride
@pytest.mark.parametrize("n_in", [[0, 1, 3], None], ids=["n_in", "null"])
def test_prompt_against_feedback(ti, n_in):
    """Steps 0..4 of three streams whose prompts hold 0, 1 and 3 tokens (or n_in NULL: none); before every step
    the host plants the key of the token the model expects next.  The record of fed-back tokens carries over."""
    M, stride = 3, 5
    in_tokens = np.array([[9, 9, 9], [4, 9, 9], [10, 0, 6]], np.int32)
    out = filled((M, stride), np.int32)
    emb = embedding(100)
    for s in range(5):
        fed = [(3 * s + 2 * m + 1) % VOCAB for m in range(M)]
        am = keys(M, *[(m, (7 * s + 11 * m) % SLOTS, logit_key(0.5 * s - m, fed[m])) for m in range(M)])
        case = StepCase(argmax=am, base_pos=[0, 10, 20], s=s, emb=emb, in_tokens=in_tokens,
                        n_in=None if n_in is None else np.array(n_in, np.int32), out_stride=stride, out_tokens=out)
        ref = check(ti, case)
        prompt = [0, 0, 0] if n_in is None else n_in
        assert ref.tokens.tolist() == [in_tokens[m, s] if s < prompt[m] else fed[m] for m in range(M)]
        out = ref.out_tokens
    fill = int(filled(1, np.int32)[0])
    assert np.count_nonzero(out != fill) == (15 if n_in is None else 5 + 4 + 2)


def test_out_stride_edge(ti):
    """out_stride 2: the write at s - n_in == 1 happens, the one at 2 does not -- it would land in the next row's
    first entry (or, for the last row, in the guard)."""
    M, stride = 2, 2
    out = filled((M, stride), np.int32)
    fill = int(out[0, 0])
    seen = []
    for s in range(4):
        am = keys(M, (0, 3, logit_key(1.0, 2 + s)), (1, 4, logit_key(1.0, 6 + s)))
        case = StepCase(argmax=am, base_pos=[0, 0], s=s, emb=embedding(8), in_tokens=np.array([[1], [1]], np.int32),
                        n_in=np.array([1, 0], np.int32), out_stride=stride, out_tokens=out)
        out = check(ti, case).out_tokens
        seen.append(out.reshape(-1).tolist())
    assert seen == [[fill, fill, 6, fill], [3, fill, 6, 7], [3, 4, 6, 7], [3, 4, 6, 7]]


# ------------------------------------------------------------------ placeholder
@pytest.mark.parametrize("hidden", [100, 256])
@pytest.mark.parametrize("s", [0, 2])
@pytest.mark.parametrize("first", [0, 37])
def test_placeholder(ti, first, s, hidden):
    """0.1f * ((off + i) % 100), off = placeholder_first at step 0 only; no table.  The token bookkeeping runs as
    ever."""
    case = StepCase(argmax=keys(2, (0, 1, logit_key(1.0, 4)), (1, 30, logit_key(2.0, 8))), base_pos=[3, 0], s=s,
                    hidden=hidden, vocab=VOCAB, placeholder_first=first, out_stride=3, out_tokens=filled((2, 3), np.int32))
    ref = check(ti, case)
    assert ref.h[0, 1] == f32(0.1) * f32(((first if s == 0 else 0) + 1) % 100)
    assert ref.out_tokens[:, s].tolist() == [4, 8]


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(ti):
    base = StepCase(argmax=keys(2, (0, 1, logit_key(1.0, 4))), base_pos=[3, 0], s=0, emb=embedding(8),
                    in_tokens=np.array([[1], [2]], np.int32), n_in=np.array([1, 1], np.int32), out_stride=1,
                    out_tokens=filled((2, 1), np.int32))
    cases = {
        "fold_x with a placeholder": DeviceStep(ti, base.at(placeholder_first=0, fold_w=norm_w(8))),
        "fold_x without fold_w": DeviceStep(ti, base, fold_x=True),
        "fold_x without fold_w (given then dropped)": DeviceStep(ti, base.at(fold_w=norm_w(8)), fold_w=False),
        "n_in without in_tokens": DeviceStep(ti, base),
        "M = 0": DeviceStep(ti, base),
    }
    cases["n_in without in_tokens"].args.in_tokens = None
    cases["M = 0"].args.M = 0
    for name, d in cases.items():
        assert d.launch() != 0, name
        assert b"ti_step_begin" in ti.lib().ti_last_error(), name
        for b in d.outputs() + list(d.inputs.values()):
            assert b.unchanged(), name
    d = DeviceStep(ti, base)            # the same arguments untouched do launch
    assert d.launch() == 0
    assert_step_equal(d.result(), step_begin_ref(base))


# ------------------------------------------------------------------ hand-shakes
@pytest.mark.parametrize("fold", [False, True], ids=["rmsnorm", "folded"])
def test_handshake_with_lm_head(ti, oracle, fold):
    """ti_step_begin then the lm_head (int4, TI_EPI_LOGITS_ARGMAX, step_ctr += 1) on the same device buffers for 6
    steps, M = 3, n_in = [1, 3, 2].  Each step's fed-back token must be the lowest-index argmax of the logits the
    device itself wrote the step before; h, pos, out_tokens and the counter follow the model; the logits stay within
    the GEMM form's bound of the float64 product (test_gpu_kernels.py test_gemm_rmsnorm_prologue; folded:
    test_gpu_fold.py).  TI_X_F16_FOLDED takes one row per launch, so the folded variant runs the lm_head once per
    row on that row's fold_x / fold_ss / argmax slots, the last launch advancing the counter."""
    M, H, V, steps, stride = 3, 256, 48, 6, 6
    rng = np.random.RandomState(77)
    emb = rng.standard_normal((V, H)).astype(f16)
    w = (rng.standard_normal((H, V)) * 0.05).astype(f32)
    nw = (1 + 0.1 * rng.standard_normal(H)).astype(f32)
    tiles, scales = ti.wpack_host(w, 4)
    q, sc = oracle.quantize_groups(w, 4)
    wf = oracle.dequantize_groups(q, sc).astype(np.float64)
    td, sd, nwd = (ti.DeviceBuffer.from_array(a) for a in (tiles, scales, nw))
    in_tokens = np.array([[5, 0, 0], [47, 0, 13], [20, 21, 0]], np.int32)
    n_in = np.array([1, 3, 2], np.int32)
    case = StepCase(argmax=np.zeros((M, SLOTS), np.uint64), base_pos=[0, 4, 9], s=0, emb=emb, in_tokens=in_tokens, n_in=n_in,
                    out_stride=stride, out_tokens=filled((M, stride), np.int32), fold_w=nw if fold else None)
    d = DeviceStep(ti, case)
    logits_d = Guarded(ti, filled((M, V), f32))
    model_keys, out = case.argmax, case.out_tokens
    for s in range(steps):
        ref = step_begin_ref(case.at(s=s, argmax=model_keys, out_tokens=out))
        assert d.launch() == 0, ti.lib().ti_last_error()
        assert_step_equal(d.result(), ref)
        out = ref.out_tokens
        ep = ti.Epilogue()
        ep.kind, ep.ldo, ep.advance = ti.EPI_LOGITS_ARGMAX, V, 1
        if fold:
            for m in range(M):
                ep.out, ep.argmax = logits_d.at(4 * m * V), d.argmax.at(8 * m * SLOTS)
                ep.ss_in, ep.n_ss = d.ss.at(4 * m), 1
                ep.step_ctr = d.ctr.ptr if m == M - 1 else None
                ti.check(ti.lib().ti_gemm_wq_a16(td.ptr, sd.ptr, 4, d.fx.at(2 * m * H), ti.X_F16_FOLDED, H, None, 1e-5,
                                                 1, V, H, C.byref(ep), None))
        else:
            ep.out, ep.argmax, ep.step_ctr = logits_d.ptr, d.argmax.ptr, d.ctr.ptr
            ti.check(ti.lib().ti_gemm_wq_a16(td.ptr, sd.ptr, 4, d.h.ptr, ti.X_F32_RMSNORM, H, nwd.ptr, 1e-5, M, V, H,
                                             C.byref(ep), None))
        ti.sync()
        assert d.ctr.read()[0] == s + 1
        d.ctr.host0[GUARD:GUARD + 4] = np.array([s + 1], np.int32).view(np.uint8)    # now the expected input
        logits = logits_d.read()
        xa = oracle.rms_norm(ref.h, nw).astype(f16).astype(np.float64)
        rel = 2.5e-3 if fold else 2e-5 + 1e-3
        bound = rel * (np.abs(xa) @ np.abs(wf)) + 1e-6
        err = np.abs(logits.astype(np.float64) - xa @ wf)
        assert np.all(err <= bound), f"step {s}: max err {err.max()} (bound {bound.min()})"
        best = np.argmax(logits, axis=1)         # lowest index among equal maxima
        got_keys = d.argmax.read()
        want = [logit_key(logits[m, best[m]], best[m]) for m in range(M)]
        assert got_keys.max(axis=1).tolist() == want, f"step {s}"
        model_keys = keys(M, *[(m, 0, want[m]) for m in range(M)])
    fed = [[int(t) for t in out[m, :steps - n_in[m]]] for m in range(M)]
    assert all(0 <= t < V for row in fed for t in row)
    assert np.all(out[0, steps - 1:] == filled(1, np.int32)[0])       # row 0 fed back steps 1..5: 5 entries of 6


def test_handshake_with_sampler(ti):
    """ti_sample_step (top_k = 1: the draw does not matter) writes its key into slot 0 of rows that already hold
    logit keys for another token; the next ti_step_begin feeds the sampled token back and records it."""
    L = ti.lib()
    vp, i32, cf = C.c_void_p, C.c_int32, C.c_float
    L.ti_sample_step.argtypes = [vp, i32, i32, i32, cf, i32, cf, vp, i32, vp, i32, vp, vp, vp, vp]
    M, V, S, H = 3, 48, 4, 100
    rng = np.random.RandomState(91)
    logits = rng.standard_normal((M, V)).astype(f32)
    sampled = np.argmax(logits, axis=1)
    other = [(int(t) + 1) % V for t in sampled]
    am = keys(M, *[(m, 0, logit_key(logits[m].max() + 1, other[m])) for m in range(M)],
              *[(m, 3 + m, logit_key(logits[m].max() + 2, other[m])) for m in range(M)])
    n_in = np.array([1, 2, 3], np.int32)
    emb = rng.standard_normal((V, H)).astype(f16)
    # the lm_head of step 2 has advanced the counter to 3: the sampler looks back one step, step_begin runs step 3
    case = StepCase(argmax=am, base_pos=[0, 0, 7], s=3, emb=emb, in_tokens=np.zeros((M, 3), np.int32), n_in=n_in,
                    out_stride=S, out_tokens=filled((M, S), np.int32))
    d = DeviceStep(ti, case)
    ld, dd = ti.DeviceBuffer.from_array(logits), ti.DeviceBuffer.from_array(np.full(M * S, 0.5, f32))
    ti.check(L.ti_sample_step(ld.ptr, V, M, V, 1.0, 1, 1.0, dd.ptr, S, d.ctr.ptr, 1, d.inputs["n_in"].ptr, d.argmax.ptr,
                              None, None))
    ti.sync()
    after = d.argmax.read()
    want = am.copy()
    want[:, 0] = [sampled_key(t) for t in sampled]
    assert np.array_equal(after, want)
    ref = step_begin_ref(case.at(argmax=after))
    assert ref.tokens.tolist() == sampled.tolist()
    assert d.launch() == 0, L.ti_last_error()
    got = d.result()
    assert_step_equal(got, ref)
    assert [got.out_tokens[m, 3 - n_in[m]] for m in range(M)] == sampled.tolist()
