"""CPU oracle of the codec GEMM kernels alone — TEST INFRASTRUCTURE ONLY.

What tts_op_gemm_planes / tts_op_split_planes (include/tts_mi355x_ops.h; gemm_x3p_kernel of
tts-max_amd/csrc/codec_gemm.hip, gemm_bx3_kernel and gemm_f32_kernel of codec_kernels.hip) must
compute, C = act(A . B^T + bias) + resid over fp32 operands, restated in numpy:

* `split(x)`: the (h, m, l) bf16 planes of an fp32 array, h = bf16(x), m = bf16(x - h),
  l = bf16(x - h - m), round to nearest even; h + m + l == x exactly.
* `reference(case)`: the result in float64, and S = |A| . |B|^T per element, the scale of the
  accumulation error.
* `restate(case, mutant=None)`: the bf16-split kernels in fp32: K in 32-element steps in order,
  two 16-element MFMA slices per step, the six plane products of a slice in the kernels' order
  (am.bm, al.bh, ah.bl, am.bh, ah.bm, ah.bh) accumulated in fp32, then acc + bias, swish,
  resid + v, and the planes of the stored value.  Not bit-equal to the GPU (the summation order
  inside an MFMA is not documented); it shows that an honest kernel passes `judge`.
* MUTANTS of the restatement by keyword: the faults these kernels can plausibly have.
  tests/test_codec_gemm_reference.py shows that `judge` fails every one of them.

Two families of cases, shared by the CPU test and tests/test_gpu_codec_gemm.py:

* exact: entries c0 + c1 2^-9 + c2 2^-18 (c in {-1, 0, 1}, c0 != 0) against an operand of at most
  32 non-zeros per row (columns 0 and K - 1 among them).  Every product is a multiple of 2^-18,
  every partial sum in any order stays below 2^6 with bias and resid (multiples of 2^-18 below
  8), so fp32 accumulation is exact and the comparison is bit equality with float64.  Variants:
  a3b1 (three-plane A, +-1 B), a1b3, a2b2 (two planes each: only the am.bm product carries the
  2^-18 terms).  The terms the kernels drop (am.bl, al.bm, al.bl) are zero in all three.  Only
  act 0: the swish is not exact.
* random: standard-normal A, B, bias, resid.  Per element e = |C - ref| / S, with two bars:
  max e <= (K + 4) 2^-24 (the worst case of fp32 accumulation plus the dropped terms, <= 2^-26),
  and rms(e) <= RMS_FACTOR x the rms(e) of torch's CPU fp32 matmul with the same epilogue in
  fp32 (`cpu_fp32`).  The rms of a handful of elements is no statistic (one element's CPU error
  is exactly 0 about one time in three), so the rms bar applies from RMS_MIN_ELEMS elements; the
  1 x 1 x 32 shape keeps the hard bound and the exact cases, and the (TM+5, TN+4, 32) shape
  carries the rms bar for a single K step.
"""

from __future__ import annotations

import dataclasses
import functools
import zlib

import numpy as np
import torch

F32 = np.float32
RMS_FACTOR = 4.0      # headroom for the MFMA-internal accumulation order
RMS_MIN_ELEMS = 256
GUARD_F32 = 0x7FA55AA5   # an fp32 NaN pattern no arithmetic produces
GUARD_BF16 = 0xFFFF      # plane buffers' fill (a bf16 NaN)

MUTANTS = ("drop_l", "drop_mm", "swap_ml_a", "skip_last_step", "skip_second_half", "permute_a_chunks",
           "partial_m_row", "resid_before_act", "cp_from_unrounded")

# ---- kernel forms: name -> (form code of tts_op_gemm_planes, TM, TN, kernel, A operand, B operand)
def x3p_form(tile: int, ilv: int = -1, pp: bool = False, four: bool = False) -> int:
    return tile | ((2 if ilv < 0 else ilv) << 3) | (0x20 if pp else 0) | (0x40 if four else 0)


X3P_TILES = ((256, 128), (128, 128), (128, 64), (64, 64), (32, 32), (128, 128))
FORMS: dict[str, tuple] = {}
for _t in range(5):
    for _i in (0, 1):
        FORMS[f"x3p_t{_t}_ilv{_i}"] = (x3p_form(_t, _i), *X3P_TILES[_t], "x3p", "Ap", "Bp")
FORMS["x3p_t5_3stage"] = (x3p_form(5), 128, 128, "x3p", "Ap", "Bp")
FORMS["x3p_t0_pp"] = (x3p_form(0, -1, pp=True), 256, 128, "x3p", "Ap", "Bp")
FORMS["x3p_t4_4stage"] = (x3p_form(4, -1, four=True), 32, 32, "x3p", "Ap", "Bp")
for _i, (_n, _tm, _tn, _a, _b) in enumerate((("256x128_ApBp", 256, 128, "Ap", "Bp"), ("128x128_ApBp", 128, 128, "Ap", "Bp"),
                                             ("256x128_Bp", 256, 128, "A", "Bp"), ("128x256_Bp", 128, 256, "A", "Bp"),
                                             ("128x128_Bp", 128, 128, "A", "Bp"), ("64x64_Bp", 64, 64, "A", "Bp"),
                                             ("128x128", 128, 128, "A", "B"), ("64x64", 64, 64, "A", "B"))):
    FORMS[f"bx3_{_n}"] = (0x100 + _i, _tm, _tn, "bx3", _a, _b)
for _i, (_n, _tm) in enumerate((("64x64_k64", 64), ("64x64_k16", 64), ("128x128_k32", 128), ("128x128_k16", 128))):
    FORMS[f"f32_{_n}"] = (0x200 + _i, _tm, _tm, "f32", "A", "B")
ANCHOR = "bx3_64x64"   # every bf16-split form must give this form's bits


def kstep_of(form_name: str) -> int:
    """K elements per staged step of a form: 32 for the bf16-split kernels, the fp32 kernel's own."""
    return {"k64": 64, "k32": 32, "k16": 16}[form_name.rsplit("_", 1)[1]] if form_name.startswith("f32_") else 32


def shapes(TM: int, TN: int, ks: int = 32):
    """(M, N, K, lda, ldc) per form tile and K step: the places where a tiled GEMM goes wrong."""
    return [
        (1, 1, ks, ks, 1),                               # one row and column, one K step, scalar epilogue
        (TM + 5, TN + 4, ks, ks, TN + 4),                # one K step over enough elements for the rms bar
        (TM + 5, TN + 4, 2 * ks, 2 * ks, TN + 4),        # four ragged tiles, vector epilogue, two steps
        (TM + 5, TN + 3, 3 * ks, 3 * ks, TN + 4),        # ldc = N + 1: scalar epilogue, three steps
        (4 * TM - 3, 2 * TN, 5 * ks, 5 * ks, 2 * TN),    # eight tiles (XCD remap on), five steps
        (TM + 5, 64, 3 * ks, ks, 64),                    # lda < K: the k = 3 conv window over M + 2 rows
        (70, 68, 2048, 2048, 68),                        # 64 steps of 32
    ]


# ---- the split ------------------------------------------------------------------------------
def rbf(x: np.ndarray) -> np.ndarray:
    """fp32 -> the nearest bf16 (ties to even), as fp32.  Finite inputs."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(F32)


def split(x):
    """(h, m, l) of an fp32 array (numpy, or torch CPU -> torch), each bf16-valued fp32."""
    if isinstance(x, torch.Tensor):
        return tuple(torch.from_numpy(p) for p in split(x.numpy()))
    x = np.ascontiguousarray(x, dtype=F32)
    h = rbf(x)
    r = x - h
    m = rbf(r)
    return h, m, rbf(r - m)


def bits16(p: np.ndarray) -> np.ndarray:
    """bf16-valued fp32 -> its 16 bits."""
    return (np.ascontiguousarray(p, dtype=F32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def planes_bits(x: np.ndarray) -> np.ndarray:
    """[3, ...] uint16: the planes as the kernels store them."""
    return np.stack([bits16(p) for p in split(x)])


def from_bits16(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << np.uint32(16)).view(F32)


# ---- cases ----------------------------------------------------------------------------------
@dataclasses.dataclass(eq=False)
class Problem:
    """One set of operands; `Case` adds the epilogue's configuration."""
    name: str
    family: str   # random | a3b1 | a1b3 | a2b2
    M: int
    N: int
    K: int
    lda: int
    ldc: int
    tm: int
    abuf: np.ndarray   # fp32 [(M - 1) * lda + K]: row m = abuf[m * lda : m * lda + K]
    B: np.ndarray      # [N, K]
    bias: np.ndarray   # [N]
    resid: np.ndarray  # [M, ldc] (columns >= N unused)

    @property
    def A(self) -> np.ndarray:
        return np.lib.stride_tricks.as_strided(self.abuf, (self.M, self.K), (4 * self.lda, 4), writeable=False)

    @functools.cached_property
    def acc64(self):
        return self.A.astype(np.float64) @ self.B.astype(np.float64).T

    @functools.cached_property
    def S(self):
        return np.abs(self.A).astype(np.float64) @ np.abs(self.B).astype(np.float64).T

    @functools.cached_property
    def acc_cpu32(self):
        """torch's CPU fp32 matmul of the same operands: the yardstick of the rms bar."""
        return (torch.from_numpy(np.array(self.A)) @ torch.from_numpy(self.B).t()).numpy()


@dataclasses.dataclass(eq=False)
class Case:
    p: Problem
    act: int
    bias: bool
    resid: bool

    @property
    def name(self):
        return f"{self.p.name}_act{self.act}_b{int(self.bias)}_r{int(self.resid)}"


def _three_plane(rng, shape, planes=3):
    c0 = rng.choice(np.array([-1.0, 1.0]), shape)
    c1 = rng.integers(-1, 2, shape).astype(np.float64)
    c2 = rng.integers(-1, 2, shape).astype(np.float64) if planes == 3 else np.zeros(shape)
    return (c0 + c1 * 2.0 ** -9 + c2 * 2.0 ** -18).astype(F32)


def _sparse_rows(rng, rows, width, nnz, values):
    """[rows, width]: at most nnz non-zeros per row, columns 0 and width - 1 among them."""
    out = np.zeros((rows, width), F32)
    for r in range(rows):
        inner = 1 + rng.choice(width - 2, min(nnz - 2, width - 2), replace=False)
        cols = np.concatenate([[0, width - 1], inner])
        out[r, cols] = values(len(cols))
    return out


def _exact_operands(family, M, N, K, lda, seed):
    """A buffer and B of an exact case, with the generator's own checks."""
    rows_buf = ((M - 1) * lda + K) // lda if lda < K else M
    wa = lda if lda < K else K
    per_row = 32 // (K // lda) if lda < K else 32   # a window row spans K / lda buffer rows
    for attempt in range(32):
        rng = np.random.default_rng(seed + 7919 * attempt)
        pm1 = lambda n: rng.choice(np.array([-1.0, 1.0], F32), n)
        if family == "a3b1":
            a = _three_plane(rng, (rows_buf, wa))
            b = _sparse_rows(rng, N, K, 32, pm1)
            dense = [a]
        elif family == "a1b3":
            a = _sparse_rows(rng, rows_buf, wa, per_row, pm1)
            b = _three_plane(rng, (N, K))
            dense = [b]
        else:  # a2b2: two planes on both sides, the sparse side's non-zeros two-plane as well
            a = _three_plane(rng, (rows_buf, wa), planes=2)
            b = _sparse_rows(rng, N, K, 32, lambda n: _three_plane(rng, (n,), planes=2))
            dense = [a, b[b != 0]]
        shares = []
        for d in dense:
            h, m, l = split(d)
            assert np.array_equal(h.astype(np.float64) + m + l, d.astype(np.float64)), "h + m + l != x"
            shares.append((float(np.mean(m != 0)), float(np.mean(l != 0))))
        floor_l = 0.25 if family != "a2b2" else 0.0
        if all(sm >= 0.25 and sl >= floor_l for sm, sl in shares):
            break   # (a 32-entry operand misses a floor now and then: the next seed)
    # the planes the case is about are populated: m on >= 25 % of the multi-plane entries, l too
    assert all(sm >= 0.25 and sl >= floor_l for sm, sl in shares), (family, shares)
    if family == "a2b2":
        assert all(sl == 0 for _, sl in shares)
    return a.reshape(-1), b, shares


def problem(family, M, N, K, lda, ldc, tm) -> Problem:
    seed = zlib.crc32(f"{family}/{M}/{N}/{K}/{lda}/{ldc}".encode())
    rng = np.random.default_rng(seed)
    name = f"{family}_{M}x{N}x{K}" + (f"_lda{lda}" if lda != K else "") + (f"_ldc{ldc}" if ldc != N else "")
    if family == "random":
        abuf = rng.standard_normal((M - 1) * lda + K).astype(F32)
        B = rng.standard_normal((N, K)).astype(F32)
        bias = rng.standard_normal(N).astype(F32)
        resid = rng.standard_normal((M, ldc)).astype(F32)
        return Problem(name, family, M, N, K, lda, ldc, tm, abuf, B, bias, resid)
    abuf, B, _ = _exact_operands(family, M, N, K, lda, seed)
    q = 2.0 ** -18
    bias = (rng.integers(-2 ** 21, 2 ** 21, N, endpoint=True) * q).astype(F32)
    resid = (rng.integers(-2 ** 21, 2 ** 21, (M, ldc), endpoint=True) * q).astype(F32)
    p = Problem(name, family, M, N, K, lda, ldc, tm, abuf, B, bias, resid)
    # the premise of bit equality: at most 32 products of magnitude < 1.004 per output, every
    # one a multiple of 2^-18, and the float64 result is an fp32 number
    assert int(np.minimum((p.A != 0).sum(1)[:, None], (B != 0).sum(1)[None, :]).max()) <= 32
    assert float(p.S.max()) + 16 < 64
    full = p.acc64 + bias[None, :] + resid[:, :N]
    for ref in (p.acc64, full):
        assert np.array_equal(ref.astype(F32).astype(np.float64), ref), "float32(ref) != ref"
    return p


FAMILIES = ("random", "a3b1", "a1b3", "a2b2")


def cases_of(p: Problem):
    """Every epilogue configuration the GPU test runs on a problem."""
    acts = (0, 1) if p.family == "random" else (0,)
    return [Case(p, act, bool(b), bool(r)) for act in acts for r in (0, 1) for b in (0, 1)]


@functools.lru_cache(maxsize=2)
def problems(TM: int, TN: int, ks: int = 32):
    return [problem(f, *s, TM) for s in shapes(TM, TN, ks) for f in FAMILIES]


# ---- reference, yardstick, restatement ------------------------------------------------------
def _epilogue(acc, c: Case, dt):
    p = c.p
    v = acc.astype(dt)
    if c.bias:
        v = v + p.bias.astype(dt)[None, :]
    if c.act == 1:
        with np.errstate(over="ignore"):   # (exp(-v) = inf gives -0, as the kernels' expf)
            v = v / (dt(1.0) + np.exp(-v))
    if c.resid:
        v = p.resid[:, :p.N].astype(dt) + v
    return v


def reference(c: Case):
    """(float64 result, S)."""
    return _epilogue(c.p.acc64, c, np.float64), c.p.S


def cpu_fp32(c: Case) -> np.ndarray:
    return _epilogue(c.p.acc_cpu32, c, F32)


_PRODUCTS = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))   # (A plane, B plane), kernel order


def _accumulate(p: Problem, mutant):
    A = np.array(p.A)
    if mutant == "partial_m_row":
        A[p.M - 1] = A[p.M - 2]
    ap, bp = list(split(A)), list(split(p.B))
    if mutant == "swap_ml_a":
        ap[1], ap[2] = ap[2], ap[1]
    acc = np.zeros((p.M, p.N), F32)
    steps = p.K // 32 - (1 if mutant == "skip_last_step" else 0)
    for s in range(steps):
        for kk in range(1 if mutant == "skip_second_half" else 2):
            ks = slice(32 * s + 16 * kk, 32 * s + 16 * kk + 16)
            ka = ks
            if mutant == "permute_a_chunks":   # chunk c of the step read from chunk c ^ 1
                ka = np.arange(ks.start, ks.stop).reshape(2, 8)[::-1].reshape(-1)
            for ia, ib in _PRODUCTS:
                if mutant == "drop_l" and 2 in (ia, ib):
                    continue
                if mutant == "drop_mm" and (ia, ib) == (1, 1):
                    continue
                acc = acc + ap[ia][:, ka] @ bp[ib][:, ks].T
    return acc


_acc_cache: dict = {}


def applies(c: Case, mutant) -> bool:
    p = c.p
    if mutant == "partial_m_row":
        return p.M >= 2 and p.M % p.tm != 0
    if mutant == "resid_before_act":
        return c.resid and c.act == 1
    if mutant == "cp_from_unrounded":
        return c.resid
    return True


def restate(c: Case, mutant=None):
    """(C fp32 [M, N], Cp uint16 [3, M, N]) of the bf16-split kernels restated in fp32."""
    assert mutant is None or (mutant in MUTANTS and applies(c, mutant)), mutant
    p = c.p
    am = mutant if mutant in MUTANTS[:7] else None
    key = (id(p), am)
    if key not in _acc_cache:
        _acc_cache[key] = (p, _accumulate(p, am))   # (p kept alive: the key is its id)
    acc = _acc_cache[key][1]
    if mutant == "resid_before_act":
        v = acc + p.bias[None, :] if c.bias else acc
        v = p.resid[:, :p.N] + v
        with np.errstate(over="ignore"):
            v = (v / (F32(1.0) + np.exp(-v))).astype(F32)
    else:
        v = _epilogue(acc, c, F32)
    cp = planes_bits(v)
    if mutant == "cp_from_unrounded":   # the residual add contracted into the split: no fp32 rounding
        u = p.resid[:, :p.N].astype(np.float64) + _epilogue(acc, Case(p, c.act, c.bias, False), F32).astype(np.float64)
        h = _round_to_bf16_f64(u)
        r = u - h
        m = _round_to_bf16_f64(r)
        cp = np.stack([bits16(h), bits16(m), bits16(_round_to_bf16_f64(r - m))])
    return v.astype(F32), cp


def _round_to_bf16_f64(x: np.ndarray) -> np.ndarray:
    """float64 -> nearest bf16-valued number (ties to even), as fp32."""
    m, e = np.frexp(x)               # x = m 2^e, |m| in [0.5, 1)
    return np.ldexp(np.rint(m * 256.0), e - 8).astype(F32)


# ---- the judge ------------------------------------------------------------------------------
def judge(c: Case, C: np.ndarray, Cp: np.ndarray | None = None):
    """C [M, N] fp32 as a launch stored it, and Cp [3, M, N] uint16 where the launch wrote planes
    (a planes-only launch is judged with the C of the same launch writing C: h + m + l rebuilds
    C only above ~2^-100, where l does not underflow) -> (figures, fails)."""
    p = c.p
    fails = []
    fig = {}
    C = np.ascontiguousarray(C, dtype=F32)
    ref, S = reference(c)
    if not np.isfinite(C).all():
        fails.append("non-finite output")
    elif p.family == "random":
        e = np.abs(C.astype(np.float64) - ref) / S
        hard = (p.K + 4) * 2.0 ** -24
        fig["max_e_over_bound"] = float(e.max() / hard)
        if e.max() > hard:
            fails.append(f"max e {e.max():.3e} > (K + 4) 2^-24 = {hard:.3e}")
        if e.size >= RMS_MIN_ELEMS:
            e_cpu = np.abs(cpu_fp32(c).astype(np.float64) - ref) / S
            rms, rms_cpu = float(np.sqrt(np.mean(e * e))), float(np.sqrt(np.mean(e_cpu * e_cpu)))
            fig["rms_ratio"] = rms / rms_cpu
            fig["rms_cpu"] = rms_cpu
            if rms > RMS_FACTOR * rms_cpu:
                fails.append(f"rms e {rms:.3e} > {RMS_FACTOR} x {rms_cpu:.3e} (CPU fp32)")
    else:
        nbad = int((C.view(np.uint32) != ref.astype(F32).view(np.uint32)).sum())
        fig["exact_mismatches"] = nbad
        if nbad:
            fails.append(f"{nbad} elements differ from the exact result")
    if Cp is not None:
        nbad = int((np.asarray(Cp) != planes_bits(C)).sum())
        if nbad:
            fails.append(f"{nbad} plane entries are not the split of the stored C")
    return fig, fails
