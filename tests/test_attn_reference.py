"""The attention oracle (oracle/attn_oracle.py) and the cases tests/test_gpu_attn_ops.py runs on
the GPU, checked on the CPU: the bar of the random cases is set here, and every fault the
oracle can inject fails at least one case under the bars the GPU test uses.

Measured when BAR was set (CPU only, nothing here is a kernel measurement):

* r = 3.14 u: the largest error of the fp32 restatements (64-position chunked sums; exp and
  the kernels' exp2 form) against the float64 reference over all random cases — at
  dec_random_d64_q1 (context 1,089; 2.51 u at dec_random_d128_q1, context 545): one bf16(p)
  that rounds the other way on an output that cancels to ~0 (see BAR in the oracle); every
  other random case stays within 1.35 u.
* m = 330 u: the smallest, over all mutants and the random cases a mutant applies to, of the
  mutant's largest error — drop_first at dec_random_full_d64_1088 (one row, 1,088 positions).

2 r = 6.3 <= BAR = 8 <= m / 2 = 165."""

import math

import pytest
import torch

from oracle import attn_oracle as ao
from oracle import lm_oracle


@pytest.fixture(scope="module")
def matrix():
    """Every case with its reference, the restatements and every mutant judged as the GPU test
    judges the kernels."""
    cases = ao.decode_cases() + ao.prefill_cases()
    for _, ch in ao.chains():
        cases += ch
    rec = {"cases": cases, "plain": {}, "r": {}, "m": {}, "caught": {mu: [] for mu in ao.MUTANTS}}
    for c in cases:
        ref = ao.reference(c)
        for exp2 in (False, True):
            rs = ao.restate(c, exp2=exp2)
            rec["plain"][(c.name, exp2)] = ao.judge(c, ref, rs.out, rs.K1, rs.V1, rs.q_rot)
            if c.family == "random":
                rec["r"][(c.name, exp2)] = ao.err_u(ref, rs.out)
        for mu in ao.MUTANTS:
            mr = ao.restate(c, mu)
            if not mr.applied:
                continue
            _, fails = ao.judge(c, ref, mr.out, mr.K1, mr.V1, mr.q_rot)
            if fails:
                rec["caught"][mu].append(c.name)
            if c.family == "random":
                rec["m"][(mu, c.name)] = ao.err_u(ref, mr.out)
    return rec


def test_vt_layout_is_a_permutation_of_16_by_32_tiles():
    for S, D in ((64, 64), (576, 128), (1152, 64)):
        idx = ao.vt_index(S, D)
        assert sorted(idx.reshape(-1).tolist()) == list(range(S * D))
        # the 32 positions of a dimension contiguous, 16 dimensions a tile, tiles position-major
        # inside a row of tiles
        assert int(idx[1, 0] - idx[0, 0]) == 1 and int(idx[0, 1] - idx[0, 0]) == 32
        assert int(idx[32, 0] - idx[0, 0]) == 512 and int(idx[0, 16] - idx[0, 0]) == 16 * S
        V = torch.randn(2, 3, S, D).to(torch.bfloat16)
        assert ao.bits_equal(ao.vt_decode(ao.vt_encode(V), S, D), V)


def test_reference_agrees_with_the_model_oracle_and_the_known_answers(matrix):
    """The float64 attention against lm_oracle's restatement of transformers (fp32, the same
    numerics) on one case, and against the census / spike answers, which need no reference."""
    c = next(x for x in matrix["cases"] if x.name == "pre_random_d64_q1")
    ref = ao.reference(c)
    slot, p0, n = c.seqs[-1]
    r0 = c.rows - n
    H, KVH, D = c.H, c.KVH, c.D
    q = ref.q_rot[r0:].reshape(n, H, D).float().transpose(0, 1)
    K = ref.K1[slot, :, :n].float().repeat_interleave(H // KVH, 0)
    V = ref.V1[slot, :, :n].float().repeat_interleave(H // KVH, 0)
    s = (q @ K.transpose(1, 2)) * (1.0 / math.sqrt(D))
    s = s.masked_fill(torch.arange(n)[None, :] > torch.arange(n)[:, None], float("-inf"))
    pu = torch.exp(s - s.amax(-1, keepdim=True))
    o = ((pu.to(torch.bfloat16).float() @ V) / pu.sum(-1, keepdim=True)).transpose(0, 1).reshape(n, H * D)
    assert ao.err_u(_rows_from(ref, r0), o.to(torch.bfloat16)) <= ao.BAR
    # the rope of the oracle is the model oracle's expression
    x = torch.randn(5, 4, D).to(torch.bfloat16)
    cs, sn = c.cos[:5, None], c.sin[:5, None]
    assert ao.bits_equal(ao.rope(x, cs, sn), (x * cs) + (lm_oracle.rotate_half(x) * sn))
    for c in matrix["cases"]:
        if c.expect is not None:
            d = (ao.reference(c).out - c.expect).abs().max().item()
            # (spike: the other keys weigh exp(-50.9) each)
            assert d <= (1e-12 if c.family == "census" else 1e-15 * c.S + 1e-18), (c.name, d)


def _rows_from(ref, r0):
    return ao.Result(ref.out[r0:], ref.A[r0:], ref.K1, ref.V1, ref.q_rot[r0:])


def test_partials_sum_in_slice_order():
    part = torch.tensor([[[1.0]], [[2.0 ** -24]], [[2.0 ** -24]], [[-1.0]]])
    # ((1 + 2^-24) + 2^-24) - 1 = 0 in fp32 (each small term is half an ulp of 1 and rounds to even)
    assert float(ao.sum_parts(part)) == 0.0
    assert float(ao.sum_parts(part.flip(0))) != 0.0


def test_restatement_passes_every_case(matrix):
    bad = {k: v for k, v in matrix["plain"].items() if v[1]}
    assert not bad, bad


def test_bar_lies_between_the_restatement_and_the_mutants(matrix):
    r = max(matrix["r"].values())
    m = min(matrix["m"].values())
    print(f"r = {r:.3f} u at {max(matrix['r'], key=matrix['r'].get)}; "
          f"m = {m:.3f} u at {min(matrix['m'], key=matrix['m'].get)}; BAR = {ao.BAR}")
    assert 2 * r <= ao.BAR <= m / 2, (r, ao.BAR, m)
    # every mutant was measured on a random case it applies to
    assert {mu for mu, _ in matrix["m"]} == set(ao.MUTANTS)


@pytest.mark.parametrize("mutant", ao.MUTANTS)
def test_every_mutant_fails_a_case(matrix, mutant):
    assert matrix["caught"][mutant], f"no case notices {mutant}"
    fam = {next(c.family for c in matrix["cases"] if c.name == n) for n in matrix["caught"][mutant]}
    print(mutant, "fails", len(matrix["caught"][mutant]), "cases of the families", sorted(fam))


def test_the_cases_cover_the_boundaries():
    dec = {c.name: c for c in ao.decode_cases()}
    assert sorted(p + 1 for p in dec["dec_census_d64"].row_pos)[:3] == [1, 2, 3]
    assert set(ao.DEC_CTX[64]) <= {p + 1 for p in dec["dec_random_d64_q1"].row_pos}
    assert set(ao.DEC_CTX[128]) == {p + 1 for p in dec["dec_random_d128_q3"].row_pos}
    for D, ctx in ao.FULL:
        c = dec[f"dec_random_full_d{D}_{ctx}"]
        assert c.S == ctx == c.row_pos[0] + 1
    ps = ao.spike_positions(64, 1089)
    assert {0, 63, 64, 65, 1023, 1024, 1025, 1087, 1088} <= set(ps)
    assert {0, 31, 32, 33, 511, 512, 513, 543, 544} <= set(ao.spike_positions(128, 545))
    for c in dec.values():
        assert len(set(c.row_slot)) == c.rows and c.nslots > c.rows  # distinct slots, some unused
        if c.rows > 1:
            assert c.row_slot != sorted(c.row_slot)
    assert {dec[n].rows for n in ("dec_random_rows1_nopad", "dec_random_rows3", "dec_random_d64_q1")} == {1, 3, 17}
    assert dec["dec_random_part4_rows17"].part.shape[0] == 4 and dec["dec_random_part4_rows1"].rows == 1
    pre = {c.name: c for c in ao.prefill_cases()}
    assert [n for _, _, n in pre["pre_random_d128_q1"].seqs] == ao.RAGGED
    # the poison covers the position being appended and everything beyond
    c = dec["dec_random_d64_q3"]
    for r in range(c.rows):
        tail = c.K0[c.row_slot[r], :, c.row_pos[r]:].contiguous().view(torch.int16)
        assert bool((tail == ao.POISON_NAN).all())
    assert bool(torch.isnan(c.V0[c.row_slot[0], 0, c.row_pos[0]]).all())
