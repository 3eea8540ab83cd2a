"""The wide decode step (65..256 rows: tile GEMMs + the row-generic decode attention + the tile
lm_head) through the engine: tts_generate, the streaming calls, the slot batches (uniform and
per-request) and tts_lm_score_decode.

Contract inside the wide regime (include/tts_mi355x.h, tts_slots_open): a sequence's tokens depend
only on its prompt, settings and key — not on its row, on what else is resident, or on the entry
point.  Against the narrow regime the K order differs (canonical 1024-chunks vs the decode
stream's), so equality with a batch-1 generate is claimed only where margins are decisive: the
chain fixture (tests/test_gpu_chain.py), whose every step is decided by >= 7.8 logits."""

import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = 24
KW = dict(min_new_tokens=NEW, eos_token_id=-1, repetition_penalty=1.1)


def _golden(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    seqs, po, no = [], 0, 0
    for P, n in zip(z["prompt_lens"], z["hf_new_lens"]):
        seqs.append((z["prompt_ids"][po:po + P].tolist(), z["hf_new"][no:no + n].tolist()))
        po += P
        no += n
    return str(z["arch"]), int(z["seed"]), seqs


def _load(name, max_batch=130):
    from tts_amd import configs
    from tts_amd.speechlm import MI355XSpeechLM

    arch, seed, seqs = _golden(name)
    return MI355XSpeechLM.synthetic(configs.LM_ARCHS[arch], seed=seed, max_batch=max_batch, max_seq_len=256), seqs


@pytest.fixture(scope="module")
def tiny():
    """lm_tiny at max_batch 130; batch A = 70 prompts (the longest golden prompt truncated to 60
    distinct lengths + 10 duplicates), batch B = 130 rows (A permuted + 60 other prompts); their
    greedy ids over 24 new tokens, computed once."""
    m, seqs = _load("lm_tiny")
    base = max((p for p, _ in seqs), key=len)
    A = [base[:8 + i] for i in range(60)] + [base[:8 + 6 * i] for i in range(10)]
    rng = np.random.default_rng(7)
    others = [rng.integers(0, m.arch.vocab_size, 5 + i % 40).tolist() for i in range(60)]
    perm = rng.permutation(130)
    pool = A + others
    B = [pool[j] for j in perm]
    L = max(len(p) for p in pool) + NEW
    out_a = m.generate_batch(A, max_length=L, **KW)
    out_b = m.generate_batch(B, max_length=L, **KW)
    yield dict(m=m, A=A, B=B, perm=perm, L=L, out_a=out_a, out_b=out_b)
    m.close()


def test_tokens_do_not_depend_on_row_or_on_what_else_is_resident(tiny):
    t = tiny
    where = {int(j): r for r, j in enumerate(t["perm"])}  # pool index -> row of B
    assert all(len(o) >= NEW for o in t["out_a"])
    for i in range(70):
        assert t["out_b"][where[i]][:NEW] == t["out_a"][i][:NEW], i
    for i in range(60, 70):  # duplicates inside one batch
        assert t["out_a"][i][:NEW] == t["out_a"][6 * (i - 60)][:NEW], i
    assert len({tuple(o[:NEW]) for o in t["out_a"]}) > 20  # (the prompts do lead to different ids)


def test_score_decode_logits_are_bit_equal_across_batches(tiny):
    t, m = tiny, tiny["m"]
    where = {int(j): r for r, j in enumerate(t["perm"])}
    sa = [p + o[:NEW] for p, o in zip(t["A"], t["out_a"])]
    sb = [p + o[:NEW] for p, o in zip(t["B"], t["out_b"])]
    la = m.score_decode(sa, 3)
    lb = m.score_decode(sb, 3)
    for i in range(70):
        assert torch.equal(la[i], lb[where[i]]), i
    # the decode step's own picks: the last scored position predicts nothing generated, the two
    # before it predict the last two generated ids (rep 1.1 can only demote seen ids: where the
    # raw argmax is unseen it is the pick)
    assert bool(torch.isfinite(la).all())


def test_streaming_equals_generate(tiny):
    t, m = tiny, tiny["m"]
    final = None
    for new, done in m.generate_stream(t["A"], max_length=t["L"], chunk=7, **KW):
        final = new
    assert [o[:NEW] for o in final] == [o[:NEW] for o in t["out_a"]]
    assert final == t["out_a"]


def test_uniform_slot_batch_equals_generate(tiny):
    """70 slots, 90 requests with two lengths of answer: the short ones free their rows after two
    chunks and the queued requests are admitted while the long ones still run."""
    from tts_amd.serving import ContinuousBatcher

    t, m = tiny, tiny["m"]
    prompts = [t["A"][i % 70] for i in range(90)]
    max_new = [NEW if i % 3 else 10 for i in range(90)]
    b = ContinuousBatcher(m, n_slots=70, eos_token_id=-1, repetition_penalty=1.1, chunk=5)
    got = b.generate(prompts, max_new)
    for i, g in enumerate(got):
        assert g == t["out_a"][i % 70][:max_new[i]], i


@pytest.mark.parametrize("name", ["lm_tiny", "lm_tiny128"])
def test_score_decode_65_rows_against_the_oracle(tiny, name):
    """The bar tests/test_gpu_lm.py holds the engine's teacher-forced logits to against the CPU
    oracle (0.1 absolute, the same argmax), on the golden sequences scored as a 65-row batch."""
    from oracle import lm_oracle
    from tts_amd import configs, synth

    arch, seed, seqs = _golden(name)
    m = tiny["m"] if name == "lm_tiny" else _load(name, 65)[0]
    try:
        orc = lm_oracle.LlamaOracle(configs.LM_ARCHS[arch], synth.lm_weights_cpu(configs.LM_ARCHS[arch], seed))
        full = [p + n for p, n in seqs]
        refs = [orc.score(s, 6) for s in full]
        got = m.score_decode([full[r % len(full)] for r in range(65)], 6)
        for r in range(65):
            ref = refs[r % len(full)]
            assert (got[r] - ref).abs().max().item() <= 0.1, r
            assert torch.equal(got[r].argmax(-1), ref.argmax(-1)), r
    finally:
        if name != "lm_tiny":
            m.close()


def test_sampling_at_80_rows(tiny):
    t, m = tiny, tiny["m"]
    P = t["B"][:80]
    kw = dict(max_length=t["L"], **KW)
    greedy = m.generate_batch(P, **kw)
    assert m.generate_batch(P, do_sample=True, temperature=0.8, top_k=1, seed=5, **kw) == greedy
    a = m.generate_batch(P, do_sample=True, temperature=0.8, top_k=50, seed=123, **kw)
    b = m.generate_batch(P, do_sample=True, temperature=0.8, top_k=50, seed=123, **kw)
    c = m.generate_batch(P, do_sample=True, temperature=0.8, top_k=50, seed=124, **kw)
    assert a == b and a != c and a != greedy
    assert all(len(r) >= NEW for r in a + c)


def test_per_request_batch_of_70_slots_equals_uniform_wide_batches(tiny):
    """Greedy and sampled requests with different penalties in one 70-slot per-request batch: each
    equals the uniform 70-slot batch opened with its settings, given its prompt and key."""
    from tts_amd.serving import ContinuousBatcher, RequestSettings as RS

    t, m = tiny, tiny["m"]
    free = t["out_a"][0]
    eos = free[len(free) // 2]
    S = [RS(temperature=0.0, repetition_penalty=1.1, eos_token_id=eos),
         RS(temperature=0.0, repetition_penalty=1.0, eos_token_id=-1),
         RS(temperature=0.8, top_k=50, top_p=1.0, repetition_penalty=1.1, eos_token_id=eos),
         RS(temperature=0.7, top_k=20, top_p=0.9, repetition_penalty=1.4, frequency_penalty=0.3, eos_token_id=-1),
         RS(temperature=1.0, top_k=1, top_p=1.0, repetition_penalty=1.0, eos_token_id=-1)]
    prompts, seeds = t["A"], [100 + i for i in range(70)]
    which = [i % 5 for i in range(70)]
    ref = [None] * 70
    for k, st in enumerate(S):
        rows = [i for i in range(70) if which[i] == k]
        u = ContinuousBatcher(m, n_slots=70, eos_token_id=st.eos_token_id, min_new_tokens=st.min_new_tokens,
                              repetition_penalty=st.repetition_penalty, do_sample=st.do_sample,
                              temperature=st.temperature if st.do_sample else 1.0, top_k=st.top_k, top_p=st.top_p,
                              frequency_penalty=st.frequency_penalty, seed=1, chunk=6)
        for i, o in zip(rows, u.generate([prompts[i] for i in rows], NEW, seed=[seeds[i] for i in rows])):
            ref[i] = o
    b = ContinuousBatcher(m, n_slots=70, chunk=6, per_request=True, seed=5)
    got = b.generate(prompts, NEW, seed=seeds, settings=[S[k] for k in which])
    assert got == ref
    assert any(len(r) < NEW for r in ref) and any(len(r) == NEW for r in ref)  # (some stopped on their EOS)
    assert ref[2] != ref[0] or ref[7] != ref[5]  # (sampled rows differ from greedy ones somewhere)


# ---------------------------------------------------------------- chain parity (TTS-1 dims)
def _chain_ids(new_n):
    """72 rows of the chain model (row r = batch prompt r % 8), the first new_n new ids of each."""
    from tts_amd import configs, synth
    from tts_amd.speechlm import MI355XSpeechLM

    z = np.load(os.path.join(GOLDEN, "lm_chain.npz"))
    cases, po, no = [], 0, 0
    for i, P in enumerate(z["prompt_lens"]):
        n = int(z["hf_new_lens"][i])
        if str(z["group"][i]) == "batch":
            cases.append((z["prompt_ids"][po:po + P].tolist(), z["hf_new"][no:no + n].tolist(), float(z["rep"][i]),
                          int(z["eos"][i])))
        po += P
        no += n
    assert len(cases) == 8 and len({(c[2], c[3]) for c in cases}) == 1
    prompts = [cases[r % 8][0] for r in range(72)]
    L = max(len(p) for p in prompts) + new_n
    m = MI355XSpeechLM.synthetic(configs.LM_ARCHS[str(z["arch"])], seed=int(z["seed"]),
                                 chain=synth.ChainSpec(**json.loads(str(z["chain"]))), max_batch=72, max_seq_len=L + 8)
    try:
        outs = m.generate_batch(prompts, max_length=L, min_new_tokens=new_n, eos_token_id=cases[0][3],
                                repetition_penalty=cases[0][2])
    finally:
        m.close()
    return [o[:new_n] for o in outs], [cases[r % 8][1][:new_n] for r in range(72)]


def test_chain_72_rows_equal_transformers():
    """Decisive margins: every row's first 120 new ids are transformers' batch-1 ids."""
    got, ref = _chain_ids(120)
    for r in range(72):
        assert got[r] == ref[r], (r, next(i for i, (a, b) in enumerate(zip(got[r] + [-9], ref[r] + [-8])) if a != b))


_CHAIN_CHILD = r'''
import json, os, sys
root = sys.argv[1]
sys.path[:0] = [os.path.join(root, "tts-max_amd"), root, os.path.join(root, "tests")]
from test_gpu_wide_step import _chain_ids
got, ref = _chain_ids(40)
print(json.dumps({"equal": got == ref, "rows": len(got)}))
'''


def test_chain_72_rows_with_the_chunked_head():
    """TTS_WIDE_HEAD=0: the wide step's lm_head as the 32-row decode head in chunks; 40 ids."""
    env = dict(os.environ, TTS_WIDE_HEAD="0")
    r = subprocess.run([sys.executable, "-c", _CHAIN_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == {"equal": True, "rows": 72}, res


# ---------------------------------------------------------------- limits
def test_max_batch_257_is_invalid():
    from tts_amd import _lib

    with pytest.raises(_lib.TtsError) as ei:
        _load("lm_tiny", 257)
    assert ei.value.status == _lib.TTS_E_INVALID and "max_batch" in str(ei.value)


def test_65_prompts_on_a_64_row_engine():
    """The existing error (batch out of range), and the engine keeps working."""
    from tts_amd import _lib

    m, seqs = _load("lm_tiny", 64)
    try:
        p = seqs[0][0]
        with pytest.raises(ValueError):
            m.generate_batch([p] * 65, max_length=len(p) + 4, **dict(KW, min_new_tokens=4))
        flat = np.ascontiguousarray(np.array(p * 65, dtype=np.int32))
        lens = np.full(65, len(p), dtype=np.int32)
        out, out_lens = np.zeros((65, 8), dtype=np.int32), np.zeros(65, dtype=np.int32)
        gp = _lib.GenParams(max_length=len(p) + 4, min_new_tokens=4, eos_token_id=-1, repetition_penalty=1.1)
        pi32 = ctypes.POINTER(ctypes.c_int32)
        st = m._lib.tts_generate(m._h, ctypes.byref(gp), flat.ctypes.data_as(pi32), lens.ctypes.data_as(pi32), 65,
                                 out.ctypes.data_as(pi32), 8, out_lens.ctypes.data_as(pi32), None)
        assert st == _lib.TTS_E_INVALID and b"batch out of range" in m._lib.tts_last_error()
        one = m.generate_batch([p], max_length=len(p) + 4, **dict(KW, min_new_tokens=4))[0]
        full = m.generate_batch([p] * 64, max_length=len(p) + 4, **dict(KW, min_new_tokens=4))
        assert len(one) == 4 and all(len(o) == 4 for o in full)
    finally:
        m.close()
