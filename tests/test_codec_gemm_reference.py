"""The codec GEMM oracle (oracle/codec_gemm_oracle.py) and the cases tests/test_gpu_codec_gemm.py
runs on the GPU, checked on the CPU: the fp32 restatement of the bf16-split kernels passes every
case under the judge the GPU test calls, every fault the oracle can inject fails at least one,
the exact-case generators' own assertions hold, and the shapes sit on the boundaries.

Measured here (CPU only, nothing below is a kernel measurement), 32 x 32 and 64 x 64 tile shapes:
the restatement's rms(e) is 0.57 .. 1.47 x the CPU fp32 matmul's and its largest e 0.066 of the
hard bound; the mildest mutants on the random cases, drop_mm and swap_ml_a, sit at 8.3 .. 27 x the
CPU figure and drop_l at 10 .. 34 x, so the factor 4 of the rms bar separates them."""

import numpy as np
import pytest

from oracle import codec_gemm_oracle as go

TILES = ((32, 32), (64, 64))


@pytest.fixture(scope="module")
def matrix():
    rec = {"plain": {}, "ratio": {}, "caught": {mu: [] for mu in go.MUTANTS}, "mutant_ratio": {}}
    for tile in TILES:
        for p in go.problems(*tile):
            for c in go.cases_of(p):
                C, Cp = go.restate(c)
                fig, fails = go.judge(c, C, Cp)
                rec["plain"][c.name] = fails
                if "rms_ratio" in fig:
                    rec["ratio"][c.name] = (fig["rms_ratio"], fig["max_e_over_bound"])
                for mu in go.MUTANTS:
                    if not go.applies(c, mu):
                        continue
                    mfig, mfails = go.judge(c, *go.restate(c, mu))
                    if mfails:
                        rec["caught"][mu].append(c.name)
                    if "rms_ratio" in mfig:
                        rec["mutant_ratio"][(mu, c.name)] = mfig["rms_ratio"]
    return rec


def test_split_is_exact_and_rounds_to_nearest_even():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(4096) * np.exp2(rng.integers(-20, 21, 4096))).astype(np.float32)
    x[:4] = [0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]   # two ties: down to 1, up to 1 + 2^-6
    h, m, l = go.split(x)
    assert np.array_equal(h.astype(np.float64) + m + l, x.astype(np.float64))
    assert h[2] == 1.0 and h[3] == np.float32(1.0 + 2.0 ** -6)
    assert go.bits16(h)[1] == 0x8000 and go.bits16(m)[1] == 0 and go.bits16(l)[1] == 0
    for p in (h, m, l):   # bf16-valued
        assert not (p.view(np.uint32) & 0xFFFF).any()
    import torch
    th, tm, tl = go.split(torch.from_numpy(x))
    assert torch.equal(th, torch.from_numpy(x).to(torch.bfloat16).float())   # torch's RNE cast agrees
    assert np.array_equal(go.from_bits16(go.planes_bits(x)), np.stack([h, m, l]))


def test_restatement_passes_every_case(matrix):
    bad = {k: v for k, v in matrix["plain"].items() if v}
    assert not bad, bad
    r = matrix["ratio"]
    print("restatement rms ratio %.2f .. %.2f, largest e / bound %.3f" %
          (min(v[0] for v in r.values()), max(v[0] for v in r.values()), max(v[1] for v in r.values())))


@pytest.mark.parametrize("mutant", go.MUTANTS)
def test_every_mutant_fails_a_case(matrix, mutant):
    assert matrix["caught"][mutant], f"no case notices {mutant}"
    rr = [v for (mu, _), v in matrix["mutant_ratio"].items() if mu == mutant]
    print(mutant, "fails", len(matrix["caught"][mutant]), "cases; rms ratio on random cases %.1f .. %.1f" % (min(rr), max(rr)))


def test_accumulation_mutants_fail_the_exact_cases_too(matrix):
    """The exact cases need no tolerance: each fault of the K loop changes their bits."""
    for mu in ("drop_l", "drop_mm", "swap_ml_a", "skip_last_step", "skip_second_half", "permute_a_chunks",
               "partial_m_row"):
        fam = {n.split("_")[0] for n in matrix["caught"][mu]}
        assert fam & {"a3b1", "a1b3", "a2b2"}, (mu, fam)
    assert any(n.startswith("a2b2") for n in matrix["caught"]["drop_mm"])


def test_exact_generators_hold_their_premises():
    """fp32 sums of an exact case in random K orders equal float64 bit for bit; the plane shares
    are asserted by the generator itself (>= 25 %)."""
    rng = np.random.default_rng(11)
    for fam in ("a3b1", "a1b3", "a2b2"):
        p = go.problem(fam, 70, 70, 160, 160, 70, 64)
        A, B = np.array(p.A), p.B
        want = p.acc64.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), p.acc64)
        for _ in range(3):
            acc = np.zeros((p.M, p.N), np.float32)
            for k in rng.permutation(p.K):
                acc = acc + A[:, k:k + 1] * B[None, :, k]
            assert np.array_equal(acc, want)
        _, _, shares = go._exact_operands(fam, 70, 70, 160, 160, 1)
        assert all(sm >= 0.25 for sm, _ in shares)
        if fam != "a2b2":
            assert all(sl >= 0.25 for _, sl in shares)
        # both ends of K are in play on the sparse side
        sparse = B if fam != "a1b3" else A
        assert (sparse[:, 0] != 0).all() and (sparse[:, -1] != 0).all()


def test_the_cases_cover_the_boundaries():
    tiles = sorted({(f[1], f[2], go.kstep_of(n)) for n, f in go.FORMS.items()})
    assert len(go.FORMS) == 13 + 8 + 4 and len({f[0] for f in go.FORMS.values()}) == 25
    assert {ks for _, _, ks in tiles} == {16, 32, 64}
    for tm, tn, ks in tiles:
        sh = go.shapes(tm, tn, ks)
        assert any(M % tm and N % tn and M > tm and N > tn for M, N, *_ in sh)      # ragged last tiles
        assert {K // ks for _, _, K, _, _ in sh} >= {1, 2, 3, 5} and {K for _, _, K, _, _ in sh} >= {2048}  # K steps
        assert any(N % 4 for _, N, *_ in sh) and any(ldc % 4 and N % 4 for _, N, _, _, ldc in sh)
        assert any(N % 4 == 0 and ldc % 4 == 0 and N > tn for _, N, _, _, ldc in sh)  # vector epilogue
        ntiles = [-(-M // tm) * -(-N // tn) for M, N, *_ in sh]
        assert any(t % 8 == 0 for t in ntiles) and any(t % 8 for t in ntiles)         # XCD remap on / off
        assert any(lda < K and K % lda == 0 for _, _, K, lda, _ in sh)                # conv window
        assert (1, 1, ks, ks, 1) in sh and all(K % ks == 0 for _, _, K, _, _ in sh)
    p = go.problem("random", 37, 64, 96, 32, 64, 32)
    assert p.abuf.size == (37 + 2) * 32 and np.array_equal(p.A[5], p.abuf[160:256])
    configs = {(c.act, c.bias, c.resid) for c in go.cases_of(p)}
    assert len(configs) == 8
