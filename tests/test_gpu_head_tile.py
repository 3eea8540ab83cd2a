"""The tile lm_head alone (tts_op_head_pick, form 0: head_tile_kernel of lm_pgemm.hip — the
lm_head of the 65..256-row decode step) against the decode head run in 32-row chunks (form 1),
the prefill GEMM's sums, a numpy restatement of the pick's epilogue and a float64 reference.

Shapes: M = 65 and 80 (one 128-row m-block, partly empty), 129 (three 64-row m-blocks, the last
with one row), 256 (two full 128-row blocks); K = 1024 / 2048 / 4096 (one, two and four canonical
K chunks; the three stream-plan layouts of a small matrix); N = 64 x 37 = 2368 (37 column blocks
in groups of three: 13 argmax partials a row, the last group holding one block), and one case at
the real vocabulary (3029 blocks, 1010 partials)."""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_SMALL = 64 * 37
PARTS = 1024
MS = [65, 80, 129, 256]
KS = [1024, 2048, 4096]


@pytest.fixture(scope="module")
def lib():
    from tts_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load_library()


def _check(st):
    from tts_amd import _lib

    _lib.check(st)


def _tiled(lib, w):
    N, K = w.shape
    t = torch.empty_like(w)
    _check(lib.tts_op_retile(w.data_ptr(), t.data_ptr(), N, K, 0, None))
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def head_pick(lib, x, wt, N, seen, eos, form, penalty=1.0, counts=None, freq=0.0, row_pen=None, row_freq=None,
              want_logits=True):
    """-> (part_val [M][nparts], part_idx [M][nparts], logits [M][N] or None), on the CPU."""
    M, K = x.shape
    pv = torch.full((M, PARTS), float("nan"), device="cuda")
    pi = torch.full((M, PARTS), -7, dtype=torch.int32, device="cuda")
    lg = torch.full((M, N), float("nan"), device="cuda") if want_logits else None
    n = ctypes.c_int32(0)
    _check(lib.tts_op_head_pick(x.data_ptr(), M, K, None, 0.0, wt.data_ptr(), N, seen.data_ptr(), seen.shape[1],
                                penalty, _ptr(counts), freq, eos.data_ptr(), _ptr(row_pen), _ptr(row_freq),
                                pv.data_ptr(), pi.data_ptr(), ctypes.byref(n), _ptr(lg), form, None))
    torch.cuda.synchronize()
    assert 1 <= n.value <= PARTS
    return pv[:, :n.value].cpu(), pi[:, :n.value].cpu(), None if lg is None else lg.cpu()


def pick_from_parts(pv, pi):
    """finalize's reduction: the largest partial, the lowest id among equal ones."""
    mx = pv.max(dim=1, keepdim=True).values
    return torch.where(pv == mx, pi.long(), torch.full_like(pi, 2 ** 31 - 1).long()).min(dim=1).values


def argmax_lowest(lg):
    mx = lg.max(dim=1, keepdim=True).values
    ids = torch.arange(lg.shape[1]).expand_as(lg)
    return torch.where(lg == mx, ids, torch.full_like(ids, 2 ** 31 - 1)).min(dim=1).values


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _state(M, N, g, seen_frac=0.3, eos_rows=True, with_counts=True):
    """seen bits [M][N/32 + 1], counts u16 [M][(N/32 + 1) * 32], eos_mask [M] (device)."""
    stride = N // 32 + 1
    bits = torch.rand(M, stride * 32, generator=g) < seen_frac
    bits[:, N:] = False
    w = (bits.view(M, stride, 32).long() << torch.arange(32)).sum(-1)
    seen = torch.from_numpy(w.numpy().astype(np.uint32).view(np.int32)).cuda()
    counts = None
    if with_counts:  # counts only where seen (a generated id is in the set), 0..5
        c = (torch.randint(0, 6, (M, stride * 32), generator=g) * bits).to(torch.int16)
        counts = c.cuda()
    eos = torch.full((M,), -1, dtype=torch.int32)
    if eos_rows:
        eos[::3] = torch.randint(0, N, (len(eos[::3]),), generator=g).to(torch.int32)
    return seen, counts, eos.cuda(), bits[:, :N]


def _int_inputs(M, N, K, g, device="cpu"):
    x = torch.randint(-2, 3, (M, K), generator=g, device=device).to(torch.bfloat16)
    w = torch.randint(-2, 3, (N, K), generator=g, device=device).to(torch.bfloat16)
    return x, w


def _rne_bf16(v64):
    return torch.from_numpy(v64).to(torch.float32).to(torch.bfloat16).to(torch.float32).numpy()


def _restate(sums, bits, counts, eos, penalty, freq):
    """The epilogue in numpy fp32: integer sum -> RNE bf16 -> penalty -> frequency -> EOS mask."""
    v = _rne_bf16(sums.astype(np.float64)).astype(np.float32)
    p = np.float32(penalty)
    pen = np.where(v < 0, v * p, v / p).astype(np.float32)
    v = np.where(bits, pen, v)
    if counts is not None:
        v = (v - np.float32(freq) * counts.astype(np.float32)).astype(np.float32)
    for m, e in enumerate(eos):
        if e >= 0:
            v[m, e] = -np.inf
    return v


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_exact_sums_tile_head_equals_chunked_decode_head(lib, M, K):
    """Small-integer operands: every fp32 partial sum is exact whatever the K order, so the tile
    head and the decode head must agree on every processed logit and every picked id bit for bit;
    with penalties whose arithmetic numpy restates exactly (1.0, 2.0; frequency 0.5) both equal
    the restatement."""
    g = torch.Generator().manual_seed(M * 31 + K)
    N = N_SMALL
    x, w = _int_inputs(M, N, K, g)
    assert float((x.float().abs() @ w.float().abs().t()).max()) < 2 ** 24
    sums = (x.double() @ w.double().t()).numpy()
    xd, wt = x.cuda(), _tiled(lib, w.cuda())
    seen, counts, eos, bits = _state(M, N, g)
    no_eos = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    for penalty in (1.0, 1.1, 1.4, 2.0):
        for cnt, freq in ((None, 0.0), (counts, 0.5), (counts, 0.3)):
            for em in (eos, no_eos):
                out = [head_pick(lib, xd, wt, N, seen, em, form, penalty, cnt, freq) for form in (0, 1)]
                (pv0, pi0, lg0), (pv1, pi1, lg1) = out
                assert _same_bits(lg0, lg1), (penalty, freq, int((lg0 != lg1).sum()))
                assert torch.equal(pick_from_parts(pv0, pi0), pick_from_parts(pv1, pi1)), (penalty, freq)
                assert torch.equal(pick_from_parts(pv0, pi0), argmax_lowest(lg0)), (penalty, freq)
                if penalty in (1.0, 2.0) and freq in (0.0, 0.5):
                    ref = _restate(sums, bits.numpy(), None if cnt is None else cnt.cpu().numpy()[:, :N].astype(np.int64),
                                   em.cpu().numpy(), penalty, freq)
                    assert np.array_equal(lg0.numpy().view(np.uint32), ref.view(np.uint32)), (penalty, freq)


def test_exact_sums_real_vocabulary(lib):
    """N = 193,856 = 64 x 3029 (not a multiple of 128), M = 65: 1010 partials a row, the last group
    with two column blocks."""
    M, K, N = 65, 2048, 193856
    g = torch.Generator(device="cuda").manual_seed(5)
    x, w = _int_inputs(M, N, K, g, device="cuda")
    wt = _tiled(lib, w)
    del w
    gc = torch.Generator().manual_seed(6)
    seen, counts, eos, _ = _state(M, N, gc)
    (pv0, pi0, lg0) = head_pick(lib, x, wt, N, seen, eos, 0, 1.1, counts, 0.3)
    assert pv0.shape[1] == 1010
    (pv1, pi1, lg1) = head_pick(lib, x, wt, N, seen, eos, 1, 1.1, counts, 0.3)
    assert _same_bits(lg0, lg1), int((lg0 != lg1).sum())
    assert torch.equal(pick_from_parts(pv0, pi0), pick_from_parts(pv1, pi1))
    assert torch.equal(pick_from_parts(pv0, pi0), argmax_lowest(lg0))
    # partial g = the maximum (lowest id) of columns [192 g, 192 g + 192)
    for gi in (0, 1, 504, 1008, 1009):
        blk = lg0[:, 192 * gi:192 * (gi + 1)]
        assert _same_bits(pv0[:, gi], blk.max(dim=1).values)
        assert torch.equal(pi0[:, gi].long(), argmax_lowest(blk) + 192 * gi)


@pytest.fixture(scope="module")
def random_case(lib):
    """One random weight matrix per K, 256 random rows; the prefill GEMM's bf16 output over all
    256 rows (computed once, shared)."""
    out = {}
    for K in KS:
        g = torch.Generator().manual_seed(K)
        x = (torch.randn(256, K, generator=g) * 0.5).to(torch.bfloat16)
        w = (torch.randn(N_SMALL, K, generator=g) * 0.02).to(torch.bfloat16)
        out[K] = (x, w, _tiled(lib, w.cuda()))
    return out


def _plain_logits(lib, x, wt, M):
    """penalty 1, nothing seen, no mask: the processed logits are the bf16 logits."""
    N = N_SMALL
    seen = torch.zeros(M, N // 32 + 1, dtype=torch.int32, device="cuda")
    eos = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    return head_pick(lib, x[:M].cuda(), wt, N, seen, eos, 0)


@pytest.mark.parametrize("K", KS)
def test_k_order_is_the_prefill_gemms(lib, random_case, K):
    """Random inputs: the tile head's fp32 sums are the canonical-chunk sums of pgemm_kernel, so
    its logits equal float(tts_op_pgemm(epi 0)) bit for bit at every M, and a row's bits do not
    depend on M (65 rows vs 256)."""
    x, w, wt = random_case[K]
    N = N_SMALL
    got = {}
    for M in MS:
        pv, pi, lg = _plain_logits(lib, x, wt, M)
        out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        xd = x[:M].cuda()
        _check(lib.tts_op_pgemm(xd.data_ptr(), M, K, wt.data_ptr(), N, out.data_ptr(), N, None, 0, None))
        torch.cuda.synchronize()
        assert _same_bits(lg, out.float().cpu()), (M, int((lg != out.float().cpu()).sum()))
        assert torch.equal(pick_from_parts(pv, pi), argmax_lowest(lg))
        got[M] = lg
    for M in MS[1:]:
        assert _same_bits(got[M][:65], got[65]), M


@pytest.mark.parametrize("K", KS)
def test_accuracy_against_float64(lib, random_case, K):
    """tests/test_gpu_ops.py's bar for tts_op_pgemm (within 2 bf16 ulps everywhere, at most 1 %
    of the elements differing at all) against the float64 product rounded once to bf16."""
    x, w, wt = random_case[K]
    _, _, lg = _plain_logits(lib, x, wt, 256)
    ref = (x.double() @ w.double().t()).to(torch.bfloat16).float()
    ulp = torch.clamp(ref.abs(), min=1e-30) * 2.0 ** -7
    bad = (lg - ref).abs() > 2 * ulp + 1e-6
    assert bad.sum().item() == 0, f"{bad.sum().item()} elements beyond 2 ulps"
    ndiff = (lg != ref).float().mean().item()
    assert ndiff <= 0.01, f"{ndiff:.4f} of elements differ"


@pytest.mark.parametrize("M", [80, 129])
def test_ties_and_edges(lib, M):
    """Rows with chosen logits (x row m = unit vector m, so logit[m][n] = W[n][m]): equal maxima in
    different column blocks of one partial, in the two column waves of one block, and in different
    partials (lowest id wins); the maximum at the masked EOS column; maxima that the penalties
    turn negative; -inf columns, a whole partial of them.  Both forms; the tile head's partials
    are the true maxima of the 192-column groups."""
    N, K = N_SMALL, 1024
    g = torch.Generator().manual_seed(M)
    L = torch.randint(-8, 0, (M, N), generator=g).float()  # background: -8..-1
    eos = torch.full((M,), -1, dtype=torch.int32)
    stride = N // 32 + 1
    bits = torch.zeros(M, stride * 32, dtype=torch.bool)
    counts = torch.zeros(M, stride * 32, dtype=torch.int16)
    expect = {}
    L[0, 70] = L[0, 10] = 5.0; expect[0] = 10            # blocks 1 and 0 of partial 0
    L[1, 40] = L[1, 5] = 5.0; expect[1] = 5              # column waves 1 and 0 of block 0
    L[2, 2000] = L[2, 300] = 5.0; expect[2] = 300        # partials 10 and 1
    L[3, 77] = 9.0; L[3, 1500] = 4.0; eos[3] = 77; expect[3] = 1500
    # 3.0 at a seen column with count 10: 3 / 1.5 - 0.5 * 10 = -3 < the unseen -0.5 at column 900
    L[4, :] = -1.0; L[4, 100] = 3.0; L[4, 900] = -0.5; bits[4, 100] = True; counts[4, 100] = 10; expect[4] = 900
    # every logit negative, the largest one seen: -1 * 1.5 = -1.5 < -1.25
    L[5, :] = -2.0; L[5, 640] = -1.0; L[5, 641] = -1.25; bits[5, 640] = True; expect[5] = 641
    # the last row of the batch (alone in its m-block at M = 129): ties in the last, one-block partial
    L[M - 1, 2367] = L[M - 1, 2304] = 7.0; expect[M - 1] = 2304
    w = torch.zeros(N, K)
    w[:, :M] = L.t()
    x = torch.zeros(M, K)
    x[torch.arange(M), torch.arange(M)] = 1.0
    # -inf logits: 3e38 * -3e38 overflows the fp32 product; row 6: partial 0 all -inf, and two more columns
    x[6, 6] = 3.0e38
    w[:192, 6] = -3.0e38; w[1000, 6] = -3.0e38; w[2367, 6] = -3.0e38
    w[192:, 6] = torch.where(w[192:, 6] == -3.0e38, w[192:, 6], torch.full_like(w[192:, 6], -1e-38))
    w[500, 6] = 1e-38; expect[6] = 500
    xb, wb = x.to(torch.bfloat16), w.to(torch.bfloat16)
    assert torch.equal(xb.float()[:, :6], x[:, :6]) and torch.equal(wb.float()[:, :6], w[:, :6])
    wt = _tiled(lib, wb.cuda())
    wv = (bits.view(M, stride, 32).long() << torch.arange(32)).sum(-1)
    seen = torch.from_numpy(wv.numpy().astype(np.uint32).view(np.int32)).cuda()
    outs = [head_pick(lib, xb.cuda(), wt, N, seen, eos.cuda(), form, 1.5, counts.cuda(), 0.5) for form in (0, 1)]
    (pv0, pi0, lg0), (pv1, pi1, lg1) = outs
    assert _same_bits(lg0, lg1)
    assert bool(torch.isneginf(lg0[6, :192]).all()) and bool(torch.isneginf(lg0[6, [1000, 2367]]).all())
    assert float(lg0[3, 77]) == float("-inf") and float(lg0[4, 100]) == -3.0 and float(lg0[5, 640]) == -1.5
    for pv, pi, lg in outs:
        pick = pick_from_parts(pv, pi)
        assert torch.equal(pick, argmax_lowest(lg))
        for m, e in expect.items():
            assert int(pick[m]) == e, (m, int(pick[m]), e)
        # every partial is a value the row holds at the partial's id, and the largest is the row's
        ok = pi.long().clamp(0, N - 1)
        assert _same_bits(torch.gather(lg, 1, ok), pv)
        # the ids of a row's partials are distinct (disjoint column sets)
        assert all(len(set(r.tolist())) == len(r) for r in pi)
    ngroups = (37 + 2) // 3
    assert pv0.shape[1] == ngroups
    for gi in range(ngroups):  # the tile head: partial g = columns [192 g, 192 g + 192), here checked in full
        blk = lg0[:, 192 * gi:192 * (gi + 1)]
        assert _same_bits(pv0[:, gi], blk.max(dim=1).values), gi
        assert torch.equal(pi0[:, gi].long(), argmax_lowest(blk) + 192 * gi), gi
    assert float(pv0[6, 0]) == float("-inf") and int(pi0[6, 0]) == 0


@pytest.mark.parametrize("M,K", [(65, 1024), (129, 2048), (256, 4096)])
def test_per_row_form(lib, random_case, M, K):
    """Every row carrying the same penalties: the uniform form's bits.  Mixed rows: each row equals
    the uniform run with that row's penalties."""
    x, w, wt = random_case[K]
    N = N_SMALL
    g = torch.Generator().manual_seed(M + K)
    seen, counts, eos, _ = _state(M, N, g)
    xd = x[:M].cuda()
    combos = [(1.0, 0.0), (1.1, 0.5), (1.4, 0.3)]
    uni = [head_pick(lib, xd, wt, N, seen, eos, 0, p, counts, f) for p, f in combos]
    for (p, f), u in zip(combos, uni):
        rp = torch.full((M,), p, device="cuda")
        rf = torch.full((M,), f, device="cuda")
        r = head_pick(lib, xd, wt, N, seen, eos, 0, 9.0, counts, 9.0, rp, rf)  # (the scalars are not read)
        assert _same_bits(r[2], u[2]) and _same_bits(r[0], u[0]) and torch.equal(r[1], u[1]), (p, f)
    which = torch.arange(M) % 3
    rp = torch.tensor([combos[i][0] for i in which.tolist()], device="cuda")
    rf = torch.tensor([combos[i][1] for i in which.tolist()], device="cuda")
    for form in (0, 1):  # (each form against its own uniform runs: on random inputs the K orders differ)
        ref = uni if form == 0 else [head_pick(lib, xd, wt, N, seen, eos, 1, p, counts, f) for p, f in combos]
        r = head_pick(lib, xd, wt, N, seen, eos, form, 9.0, counts, 9.0, rp, rf)
        for i in range(3):
            rows = which == i
            assert _same_bits(r[2][rows], ref[i][2][rows]), (form, i)
            assert _same_bits(r[0][rows], ref[i][0][rows]) and torch.equal(r[1][rows], ref[i][1][rows]), (form, i)
        assert torch.equal(pick_from_parts(r[0], r[1]), argmax_lowest(r[2])), form


def test_rejects_bad_shapes(lib):
    one = torch.zeros(64, dtype=torch.int32, device="cuda")
    for M, N, K in ((257, 2368, 1024), (65, 2368 + 16, 1024), (65, 2368, 1024 + 64), (0, 2368, 1024)):
        n = ctypes.c_int32(0)
        st = lib.tts_op_head_pick(one.data_ptr(), M, K, None, 0.0, one.data_ptr(), N, one.data_ptr(), N // 32 + 1, 1.0,
                                  None, 0.0, one.data_ptr(), None, None, one.data_ptr(), one.data_ptr(),
                                  ctypes.byref(n), None, 0, None)
        assert st == 1, (M, N, K)
