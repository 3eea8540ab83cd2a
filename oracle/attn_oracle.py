"""CPU oracle of the SpeechLM attention kernels alone — TEST INFRASTRUCTURE ONLY.

What tts_op_attn_prefill / tts_op_attn_decode (include/tts_mi355x_ops.h; the kernels of
tts-max_amd/csrc/lm_attn.hip on the core lm_attn_core.h) must compute, restated in torch:

* RoPE and the cache layout, to the bit: HF's bf16 apply_rotary_pos_emb (x*cos +
  rotate_half(x)*sin, every op rounded to bf16, as lm_oracle.py), the roped k into K
  [slot][kv head][max_seq][D], the raw v into V^T in tiles of 16 dimensions x 32 positions
  (vt_off below restates the kernels' index formula), a K-sliced projection's fp32 partials
  summed in slice order and rounded once to bf16.
* The attention in float64 from the roped bf16 q / k / v, with the numerics the header of
  lm_attn_core.h claims: global max, p = exp(s - max), p rounded to bf16 for P.V, l = the sum
  of the unrounded p, o = (P.V) / l.  Beside o it returns A = sum bf16(p) |v| / l per output
  element, the scale of the accumulation error.
* The same function in fp32 with 64-position chunked sums (`restate`): another valid order
  of the same sums, rounded to bf16 as the kernels round.  tests/test_attn_reference.py takes
  the bar of the random cases from it.
* Mutants of the same function by keyword (MUTANTS): the faults these kernels can plausibly
  have.  tests/test_attn_reference.py shows that every one of them fails the cases below.

The cases (decode_cases, prefill_cases, chains) are shared by the CPU test and by
tests/test_gpu_attn_ops.py, so what the CPU test proves about the inputs and the bars holds
for what the GPU test runs.

The unit of the random cases is u = ulp_bf16(|ref|) / 2 + 2^-20 A per element: the final
rounding plus the fp32 accumulation over the context.  BAR is in that unit."""

from __future__ import annotations

import dataclasses
import math
import zlib

import numpy as np
import torch

from oracle.lm_oracle import configs, hf_rope_table, rotate_half

BF16 = torch.bfloat16

# The bar of the random cases, in u.  tests/test_attn_reference.py asserts 2 r <= BAR <= m / 2
# with r = the fp32 restatements' largest error over the random cases and m = the smallest,
# over all mutants and random cases a mutant applies to, of the mutant's largest error; its
# docstring records both (r = 3.14, m = 330 when this was set).  Factor 2 over r: what the
# restatements lack of the kernels (the MFMA's accumulation order, the hardware exp2).
# Why r is not ~1: u covers the final rounding and the accumulation, not a FLIP of bf16(p_j).
# An fp32 score differs from the float64 one by ~1e-6, so about one p in 10^4 rounds to the
# other bf16 neighbour, which moves every output of that head by 2^-8 p_j |v_j| / l.  Where the
# output itself cancels to ~0 (u ~ 2^-20 A) that is 4096 p_j |v_j| / sum(p |v|) u: a few u at a
# broad context of 500..1,100 positions (r is such an element: 2.5 u at 545, 3.1 u at 1,089),
# and not a fault of the summation (the figure does not move with the chunk length).
BAR = 8.0
CENSUS_ULPS = 1.0  # census cases: |out - count / ctx| in bf16 ulps of the expected value
SPIKE_ABS = 1e-6   # spike cases: |out - v[p*]| <= SPIKE_ABS + 1 bf16 ulp

POISON_NAN = 0x7FA5  # a bf16 NaN pattern that no arithmetic produces
POISON_BIG = 0x7F62  # bf16 3.0e38


def vt_off(S: int, d, p):
    """Offset of element (dimension d, position p) in a (slot, kv head) V^T block of stride S:
    tile (d / 16, p / 32) of 16 x 32 bf16, the 32 positions of a dimension contiguous."""
    return (((d >> 4) * (S >> 5) + (p >> 5)) * 16 + (d & 15)) * 32 + (p & 31)


def vt_index(S: int, D: int) -> torch.Tensor:
    """idx[p][d] = vt_off(S, d, p): logical V [.., S, D] = tiles.reshape(.., S * D)[.., idx]."""
    p = torch.arange(S)[:, None]
    d = torch.arange(D)[None, :]
    return vt_off(S, d, p)


def vt_encode(V: torch.Tensor) -> torch.Tensor:
    """Logical V [.., S, D] -> the V^T tile buffer [.., S * D]."""
    S, D = V.shape[-2:]
    flat = torch.empty(*V.shape[:-2], S * D, dtype=V.dtype)
    flat[..., vt_index(S, D).reshape(-1)] = V.reshape(*V.shape[:-2], S * D)
    return flat


def vt_decode(flat: torch.Tensor, S: int, D: int) -> torch.Tensor:
    return flat.reshape(*flat.shape[:-1], S * D)[..., vt_index(S, D)]


def rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """bf16 x [.., D] at bf16 table rows cos / sin (broadcast): every op rounded to bf16."""
    return (x * cos) + (rotate_half(x) * sin)


def sum_parts(part: torch.Tensor) -> torch.Tensor:
    """fp32 partials [nsl, rows, ld] -> bf16 rows: summed in slice order, rounded once."""
    acc = torch.zeros_like(part[0])
    for sl in range(part.shape[0]):
        acc = acc + part[sl]
    return acc.to(BF16)


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """The bf16 ulp at |x| (float64)."""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# Faults by keyword.  Positions are relative to a row's context ctx = pos + 1 ("mid" = ctx / 2).
MUTANTS = (
    "drop_mid",       # position ctx / 2 is not attended
    "drop_first",     # position 0 is not attended
    "dup_mid",        # position ctx / 2 is attended twice
    "xor32_mid",      # position (ctx / 2) ^ 32 is read in place of ctx / 2 (a V^T tile / k-step off)
    "plus64_mid",     # position ctx / 2 + 64 is read in place of ctx / 2 (a wave off)
    "stale_k",        # decode: the cache's stale K row for the new position, not the new k
    "stale_v",        # decode: the cache's stale V column for the new position, not the new v
    "mask_plus",      # decode: position ctx is attended too
    "mask_minus",     # decode: position ctx - 1 (the new one) is not attended
    "rope_plus",      # RoPE at pos + 1
    "rope_minus",     # RoPE at pos - 1
    "kv_neighbour",   # the next kv head's K / V
    "head_rot",       # the q heads rotated by one inside their GQA group
    "other_slot",     # the next slot's cache
    "causal_plus",    # prefill: a query attends position pos + 1 of its own 16-row block
    "causal_minus",   # prefill: a query does not attend itself (inside its block)
)


@dataclasses.dataclass
class Case:
    name: str
    family: str            # "census" | "spike" | "random"
    kind: str              # "decode" | "prefill"
    H: int
    KVH: int
    D: int
    S: int                 # max_seq: the cache's position stride
    nslots: int
    qkv: torch.Tensor      # bf16 [rows, ld] (q | k | v, then unused columns)
    row_slot: list
    row_pos: list
    K0: torch.Tensor       # caches before the call, logical bf16 [nslots, KVH, S, D], poisoned
    V0: torch.Tensor
    cos: torch.Tensor      # bf16 [S, D]
    sin: torch.Tensor
    scale: float           # the op's float32 argument, as a Python float
    part: torch.Tensor | None = None    # decode: fp32 [nsl, rows, ld] in place of qkv
    seqs: list | None = None            # prefill: (slot, first position, length) per sequence
    expect: torch.Tensor | None = None  # census / spike: the known answer, float64 [rows, H * D]

    @property
    def rows(self):
        return len(self.row_pos)

    @property
    def ld(self):
        return self.qkv.shape[1]

    def blocks(self):
        """Prefill: (block start, block end) positions of each row's 16-row query block."""
        out = []
        for _, p0, n in self.seqs:
            for i in range(n):
                b0 = p0 + (i // 16) * 16
                out.append((b0, min(b0 + 16, p0 + n)))
        return out


@dataclasses.dataclass
class Result:
    out: torch.Tensor     # [rows, H * D]: float64 unrounded (reference) or bf16 (restatement, kernels)
    A: torch.Tensor | None
    K1: torch.Tensor      # caches after the call (logical)
    V1: torch.Tensor
    q_rot: torch.Tensor   # bf16 [rows, H * D]
    applied: bool = True  # a mutant changed something in at least one row


def _chunk_sum(x: torch.Tensor, chunk: int) -> torch.Tensor:
    """Sum over dim -2 ([.., n, D]) in chunks of `chunk` rows, then over the chunks."""
    n = x.shape[-2]
    pad = (-n) % chunk
    if pad:
        x = torch.cat([x, torch.zeros(*x.shape[:-2], pad, x.shape[-1], dtype=x.dtype)], -2)
    return x.reshape(*x.shape[:-2], -1, chunk, x.shape[-1]).sum(-2).sum(-2)


def _attend(q, K, V, scale, dtype, chunk, exp2=False):
    """q [G, D], K / V [n, D] (bf16) -> o, A [G, D] in dtype.  exp2: p as 2^((s - max) log2 e),
    the form the kernels evaluate."""
    q, K, V = q.to(dtype), K.to(dtype), V.to(dtype)
    s = (q @ K.t()) * scale
    d = s - s.amax(-1, keepdim=True)
    p = torch.exp2(d * 1.44269504088896341) if exp2 else torch.exp(d)
    pb = p.to(BF16).to(dtype)
    if chunk:
        l = _chunk_sum(p[..., None], chunk)
        o = _chunk_sum(pb[..., None] * V[None], chunk)
    else:
        l = p.sum(-1, keepdim=True)
        o = pb @ V
    return o / l, (pb @ V.abs()) / l


def run(c: Case, dtype=torch.float64, chunk: int = 0, mutant: str | None = None, exp2: bool = False) -> Result:
    """The op on the CPU.  float64, no chunk, no mutant: the reference (out unrounded).  Any
    other dtype: out rounded to bf16 as the kernels round it."""
    assert mutant is None or mutant in MUTANTS, mutant
    H, KVH, D, S, G = c.H, c.KVH, c.D, c.S, c.H // c.KVH
    decode = c.kind == "decode"
    applied = False
    qkv = sum_parts(c.part) if c.part is not None else c.qkv
    rows = c.rows
    q = qkv[:, : H * D].reshape(rows, H, D)
    k = qkv[:, H * D: (H + KVH) * D].reshape(rows, KVH, D)
    v = qkv[:, (H + KVH) * D: (H + 2 * KVH) * D].reshape(rows, KVH, D)
    pos = torch.tensor(c.row_pos)
    rpos = pos
    if mutant in ("rope_plus", "rope_minus"):
        rpos = (pos + (1 if mutant == "rope_plus" else -1)).clamp(0, S - 1)
        applied = bool((rpos != pos).any()) and not bits_equal(c.cos[rpos], c.cos[pos])
    cos, sin = c.cos[rpos][:, None, :], c.sin[rpos][:, None, :]
    q_rot, k_rot = rope(q, cos, sin), rope(k, cos, sin)
    K1, V1 = c.K0.clone(), c.V0.clone()
    for r in range(rows):
        K1[c.row_slot[r], :, c.row_pos[r]] = k_rot[r]
        V1[c.row_slot[r], :, c.row_pos[r]] = v[r]
    blocks = None if decode else c.blocks()
    out = torch.zeros(rows, H, D, dtype=dtype)
    A = torch.zeros(rows, H, D, dtype=dtype)
    for r in range(rows):
        slot, p_new = c.row_slot[r], c.row_pos[r]
        ctx = p_new + 1
        idx = list(range(ctx))
        mid = ctx // 2
        if mutant == "drop_mid" and ctx >= 2:
            del idx[mid]
        elif mutant == "drop_first" and ctx >= 2:
            del idx[0]
        elif mutant == "dup_mid":
            idx.append(mid)
        elif mutant == "xor32_mid" and (mid ^ 32) < ctx:
            idx[mid] = mid ^ 32
        elif mutant == "plus64_mid" and mid + 64 < ctx:
            idx[mid] = mid + 64
        elif mutant == "mask_plus" and decode and ctx < S:
            idx.append(ctx)
        elif mutant == "mask_minus" and decode and ctx >= 2:
            del idx[-1]
        elif mutant == "causal_plus" and not decode and p_new + 1 < blocks[r][1]:
            idx.append(p_new + 1)
        elif mutant == "causal_minus" and not decode and p_new > blocks[r][0]:
            del idx[-1]
        if mutant == "other_slot" and c.nslots > 1:
            slot = (slot + 1) % c.nslots
        Ks, Vs = K1[slot], V1[slot]
        if decode and mutant == "stale_k":
            Ks = Ks.clone()
            Ks[:, p_new] = c.K0[slot, :, p_new]
        if decode and mutant == "stale_v":
            Vs = Vs.clone()
            Vs[:, p_new] = c.V0[slot, :, p_new]
        if idx != list(range(ctx)) or slot != c.row_slot[r] or (decode and mutant in ("stale_k", "stale_v")):
            applied = True
        for j in range(KVH):
            jj = (j + 1) % KVH if mutant == "kv_neighbour" else j
            qg = q_rot[r, j * G: (j + 1) * G]
            if mutant == "head_rot":
                qg = torch.roll(qg, 1, 0)
            if mutant in ("kv_neighbour", "head_rot"):
                applied = applied or KVH > 1 or mutant == "head_rot"
            o, a = _attend(qg, Ks[jj, idx], Vs[jj, idx], c.scale, dtype, chunk, exp2)
            out[r, j * G: (j + 1) * G] = o
            A[r, j * G: (j + 1) * G] = a
    out, A = out.reshape(rows, H * D), A.reshape(rows, H * D)
    if not (dtype == torch.float64 and not chunk and mutant is None):
        out = out.to(BF16)
    return Result(out, A, K1, V1, q_rot.reshape(rows, H * D), applied or mutant is None)


def reference(c: Case) -> Result:
    return run(c)


def restate(c: Case, mutant: str | None = None, exp2: bool = False) -> Result:
    """fp32 with 64-position chunked sums, rounded to bf16: a valid order of the kernels' sums."""
    return run(c, dtype=torch.float32, chunk=64, mutant=mutant, exp2=exp2)


def err_u(ref: Result, out: torch.Tensor) -> float:
    """Largest error of `out` against the float64 reference in u (inf if not finite)."""
    o = out.double()
    if not bool(torch.isfinite(o).all()):
        return math.inf
    u = 0.5 * bf16_ulp(ref.out) + 2.0 ** -20 * ref.A
    return float(((o - ref.out).abs() / u).max())


def judge(c: Case, ref: Result, out: torch.Tensor, K1: torch.Tensor, V1: torch.Tensor,
          q_rot: torch.Tensor | None = None):
    """What the GPU test asserts of one call: (figure, failures).  figure = the family's error
    measure: bf16 ulps of the expected value (census), the same beyond SPIKE_ABS (spike), u
    (random); inf if an output is not finite."""
    fails = []
    o = out.double()
    if not bool(torch.isfinite(o).all()):
        fails.append("output not finite")
    # the caches: the reference's bits at every defined position, the poison untouched elsewhere
    if not bits_equal(K1, ref.K1):
        fails.append("K cache bits differ from the reference (RoPE, layout or a write outside the new positions)")
    if not bits_equal(V1, ref.V1):
        fails.append("V^T cache bits differ from the reference (layout or a write outside the new positions)")
    if q_rot is not None and not bits_equal(q_rot, ref.q_rot):
        fails.append("q_rot bits differ from the reference")
    if "output not finite" in fails:
        return math.inf, fails
    if c.family == "census":
        fig = float(((o - c.expect).abs() / bf16_ulp(c.expect)).max())
        bar = CENSUS_ULPS
    elif c.family == "spike":
        fig = float((((o - c.expect).abs() - SPIKE_ABS).clamp_min(0) / bf16_ulp(c.expect)).max())
        bar = 1.0
    else:
        fig = err_u(ref, out)
        bar = BAR
    if not fig <= bar:
        fails.append(f"{c.family} error {fig:.3g} beyond the bar {bar}")
    return fig, fails


# ------------------------------------------------------------------------------ cases ----

def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _poisoned(nslots, KVH, S, D, bits):
    t = torch.empty(nslots, KVH, S, D, dtype=BF16)
    t.view(torch.int16).fill_(int(np.int16(np.uint16(bits))))
    return t


def identity_tables(S, D):
    return torch.ones(S, D, dtype=BF16), torch.zeros(S, D, dtype=BF16)


def _tables(arch, S, D, identity):
    if identity:
        return identity_tables(S, D)
    assert arch.head_dim == D
    return hf_rope_table(arch, S)


ARCH = {64: configs.TTS1, 128: configs.TTS1_MAX_2L}


def _scale(D):
    return float(np.float32(1.0 / math.sqrt(D)))


def census_code(p: torch.Tensor, D: int) -> torch.Tensor:
    """V of position p: bit (d mod 12) of p in the lower half of the dimensions, its complement
    in the upper half.  [.., D] bf16 of 0 / 1."""
    d = torch.arange(D)
    bit = (p[..., None] >> (d % 12)) & 1
    return torch.where(d < D // 2, bit, 1 - bit).to(BF16)


def _slots(rows, nslots, g):
    """A non-identity assignment of rows to distinct slots that leaves slots unused in between."""
    perm = torch.randperm(nslots, generator=g).tolist()
    s = perm[:rows]
    if s == sorted(s) and rows > 1:
        s = s[::-1]
    return s


def make_case(name, family, kind, D, *, ctxs=None, seqs=None, S, H=8, KVH=2, nslots=None, qscale=1.0,
              poison=POISON_NAN, nsl=0, pad=64, spike=None, K0=None, V0=None, slots=None) -> Case:
    """One case.  decode: ctxs = the context of each row (pos = ctx - 1); prefill: seqs = (first
    position, length) per sequence.  K0 / V0: caches to continue from (a chain), else poisoned
    caches with random (census: coded) content at the positions below each row's first.
    spike: per row and kv head the position p* (decode: any below ctx; prefill: per row)."""
    g = _gen(name)
    decode = kind == "decode"
    nrow_units = len(ctxs) if decode else len(seqs)
    nslots = nslots or nrow_units + 3
    slots = slots or _slots(nrow_units, nslots, g)
    if decode:
        row_slot, row_pos = list(slots), [x - 1 for x in ctxs]
        first = row_pos
        sq = None
    else:
        sq = [(slots[b], p0, n) for b, (p0, n) in enumerate(seqs)]
        row_slot = [s for s, p0, n in sq for _ in range(n)]
        row_pos = [p0 + i for s, p0, n in sq for i in range(n)]
        first = [p0 for _, p0, _ in sq]
    rows = len(row_pos)
    G = H // KVH
    identity = family == "spike"
    cos, sin = _tables(ARCH[D], S, D, identity)
    ld = (H + 2 * KVH) * D + pad
    q = torch.randn(rows, H, D, generator=g) * qscale
    k = torch.randn(rows, KVH, D, generator=g)
    v = torch.randn(rows, KVH, D, generator=g)
    fresh = K0 is None
    if fresh:
        K0, V0 = _poisoned(nslots, KVH, S, D, poison), _poisoned(nslots, KVH, S, D, poison)
        for u_, slot in enumerate(slots):  # the prefix below the unit's first position
            n0 = first[u_]
            K0[slot, :, :n0] = torch.randn(KVH, n0, D, generator=g).to(BF16)
            V0[slot, :, :n0] = torch.randn(KVH, n0, D, generator=g).to(BF16)
    else:
        K0, V0 = K0.clone(), V0.clone()
    expect = None
    if family == "census":
        q = torch.zeros_like(q)
        v = census_code(torch.tensor(row_pos), D)[:, None, :].expand(rows, KVH, D).float()
        if fresh:
            for u_, slot in enumerate(slots):
                V0[slot, :, : first[u_]] = census_code(torch.arange(first[u_]), D)
        cnt = torch.stack([census_code(torch.arange(p + 1), D).double().sum(0) / (p + 1) for p in row_pos])
        expect = cnt[:, None, :].expand(rows, H, D).reshape(rows, H * D).contiguous()
    elif family == "spike":
        # q and the key at p* share one nonzero dimension; every other key is 0:
        # score(p*) = 24^2 D^-0.5 >= 50.9, every other score 0
        assert fresh
        c0 = 24.0
        q = torch.zeros_like(q)
        k = torch.zeros_like(k)
        expect = torch.zeros(rows, H, D, dtype=torch.float64)
        vb = v.to(BF16)
        if decode:
            for r in range(rows):
                K0[row_slot[r], :, : row_pos[r]] = 0
                for j in range(KVH):
                    ps = spike[r][j]
                    dim = ps % D
                    q[r, j * G: (j + 1) * G, dim] = c0
                    if ps == row_pos[r]:
                        k[r, j, dim] = c0
                        expect[r, j * G: (j + 1) * G] = vb[r, j].double()
                    else:
                        K0[row_slot[r], j, ps, dim] = c0
                        expect[r, j * G: (j + 1) * G] = V0[row_slot[r], j, ps].double()
        else:
            # key p = 24 e_(p mod D) (positions below D, so distinct), query row = 24 e_(p* mod D)
            assert max(row_pos) < D and all(p0 == 0 for p0 in first)
            for r in range(rows):
                ps = spike[r]
                assert 0 <= ps <= row_pos[r]
                k[r, :, row_pos[r] % D] = c0
                q[r, :, ps % D] = c0
            r_of = {(row_slot[r], row_pos[r]): r for r in range(rows)}
            for r in range(rows):
                expect[r] = vb[r_of[(row_slot[r], spike[r])]].double().repeat_interleave(G, 0)
        expect = expect.reshape(rows, H * D)
    qkv = torch.randn(rows, ld, generator=g).to(BF16)  # (the unused columns: finite noise)
    qkv[:, : (H + 2 * KVH) * D] = torch.cat([q.reshape(rows, -1), k.reshape(rows, -1), v.reshape(rows, -1)], 1).to(BF16)
    part = None
    if nsl:
        # fp32 partials whose slice-ordered sum, rounded once, is the case's qkv
        part = torch.randn(nsl, rows, ld, generator=g) * 0.5
        if family != "random":  # the exact inputs of the family: the last slice completes them
            acc = torch.zeros(rows, ld)
            for sl in range(nsl - 1):
                acc = acc + part[sl]
            part[-1] = qkv.float() - acc
            assert bits_equal(sum_parts(part), qkv)
    return Case(name, family, kind, H, KVH, D, S, nslots, qkv, row_slot, row_pos, K0, V0, cos, sin, _scale(D),
                part=part, seqs=sq, expect=expect)


DEC_CTX = {
    64: [1, 2, 63, 64, 65, 128, 129, 1023, 1024, 1025, 1089],
    128: [1, 31, 32, 33, 64, 511, 512, 513, 545],
}
DEC_S = {64: 1152, 128: 576}
# 17 rows at head dim 64: the list plus contexts inside a wave, one before a pass edge and the
# last wave of the second pass
DEC_CTX17 = DEC_CTX[64] + [3, 100, 500, 1000, 1087, 1088]
FULL = [(64, 64), (64, 1088), (128, 576)]  # (D, ctx == max_seq)


def spike_positions(D: int, ctx: int) -> list:
    """0, every wave edge +- 1 (the pass edges are wave edges), ctx - 2 and ctx - 1."""
    pw = 64 if D == 64 else 32
    ps = {0, ctx - 2, ctx - 1}
    for e in range(pw, ctx, pw):
        ps |= {e - 1, e, e + 1}
    return sorted(p for p in ps if 0 <= p < ctx)


def decode_cases() -> list:
    out = []
    for D in (64, 128):
        S = DEC_S[D]
        ctxs = DEC_CTX17 if D == 64 else DEC_CTX[D]
        out.append(make_case(f"dec_census_d{D}", "census", "decode", D, ctxs=ctxs, S=S))
        for qs in (1.0, 3.0):
            out.append(make_case(f"dec_random_d{D}_q{qs:g}", "random", "decode", D, ctxs=ctxs, S=S, qscale=qs))
        ctx = max(ctxs)
        ps = spike_positions(D, ctx)
        ps += [ps[-1]] * (len(ps) % 2)
        out.append(make_case(f"dec_spike_d{D}", "spike", "decode", D, ctxs=[ctx] * (len(ps) // 2), S=S,
                             spike=[ps[2 * r: 2 * r + 2] for r in range(len(ps) // 2)]))
    for D, ctx in FULL:  # ctx == max_seq: the last position of the stride
        out.append(make_case(f"dec_census_full_d{D}_{ctx}", "census", "decode", D, ctxs=[ctx], S=ctx))
        out.append(make_case(f"dec_random_full_d{D}_{ctx}", "random", "decode", D, ctxs=[ctx], S=ctx))
    out.append(make_case("dec_random_rows3", "random", "decode", 64, ctxs=[129, 1, 1025], S=1088, nslots=7, pad=8))
    out.append(make_case("dec_random_rows1_nopad", "random", "decode", 128, ctxs=[513], S=576, pad=0))
    out.append(make_case("dec_random_big_poison", "random", "decode", 64, ctxs=[65, 1024, 2], S=1152,
                         poison=POISON_BIG))
    out.append(make_case("dec_census_big_poison", "census", "decode", 128, ctxs=[33, 512], S=576, poison=POISON_BIG))
    for rows in (1, 17):  # a K-sliced projection's partials, 4 slices
        ctxs = [1025] if rows == 1 else DEC_CTX17
        out.append(make_case(f"dec_random_part4_rows{rows}", "random", "decode", 64, ctxs=ctxs, S=1152, nsl=4))
    out.append(make_case("dec_census_part4", "census", "decode", 128, ctxs=[545, 32, 1], S=576, nsl=4))
    # the real head counts
    out.append(make_case("dec_random_h32", "random", "decode", 64, ctxs=[1025, 65, 200], S=1088, H=32, KVH=8))
    out.append(make_case("dec_census_h32", "census", "decode", 128, ctxs=[513, 33], S=576, H=32, KVH=8))
    return out


RAGGED = [1, 15, 16, 17, 33, 50]


def _prefill_spike(seqs):
    """p* per row: itself, its predecessor, 0, its block's first row, the row before its block,
    the middle — in turn."""
    sp = []
    for p0, n in seqs:
        for i in range(n):
            pos = p0 + i
            b0 = (i // 16) * 16
            sp.append(max(0, [pos, pos - 1, 0, b0, b0 - 1, pos // 2][len(sp) % 6]))
    return sp


def prefill_cases() -> list:
    out = []
    seqs = [(0, n) for n in RAGGED]
    for D in (64, 128):
        out.append(make_case(f"pre_census_d{D}", "census", "prefill", D, seqs=seqs, S=64))
        out.append(make_case(f"pre_spike_d{D}", "spike", "prefill", D, seqs=seqs, S=64, spike=_prefill_spike(seqs)))
        for qs in (1.0, 3.0):
            out.append(make_case(f"pre_random_d{D}_q{qs:g}", "random", "prefill", D, seqs=seqs, S=64, qscale=qs))
    out.append(make_case("pre_random_big_poison", "random", "prefill", 64, seqs=seqs, S=128, poison=POISON_BIG))
    out.append(make_case("pre_random_h32", "random", "prefill", 64, seqs=[(0, 17), (0, 5)], S=64, H=32, KVH=8))
    out.append(make_case("pre_census_h32", "census", "prefill", 128, seqs=[(0, 33), (0, 16)], S=64, H=32, KVH=8))
    return out


def chains(ref_of=reference) -> list:
    """Calls on top of the caches an earlier call wrote: [(name, [case, case])].  The second
    case's K0 / V0 are the reference's caches after the first."""
    out = []
    for D in (64, 128):
        for fam in ("census", "random"):
            # a 40-position prefix written by an earlier call, continued by 33 rows (positions
            # 40..72: the blocks start at 40, 56, 72), beside a new sequence
            a = make_case(f"chain_pre_{fam}_d{D}_a", fam, "prefill", D, seqs=[(0, 40), (0, 9)], S=128, nslots=5,
                          slots=[3, 1])
            ra = ref_of(a)
            b = make_case(f"chain_pre_{fam}_d{D}_b", fam, "prefill", D, seqs=[(40, 33), (0, 17)], S=128, nslots=5,
                          slots=[3, 4], K0=ra.K1, V0=ra.V1)
            out.append((f"prefill_continued_{fam}_d{D}", [a, b]))
            # a decode step on top of a prefill-written cache
            p = make_case(f"chain_dec_{fam}_d{D}_a", fam, "prefill", D, seqs=[(0, n) for n in (50, 33, 1)], S=64,
                          nslots=5, slots=[4, 0, 2])
            rp = ref_of(p)
            d = make_case(f"chain_dec_{fam}_d{D}_b", fam, "decode", D, ctxs=[34, 2, 51], S=64, nslots=5,
                          slots=[0, 2, 4], K0=rp.K1, V0=rp.V1)
            out.append((f"prefill_then_decode_{fam}_d{D}", [p, d]))
    return out
