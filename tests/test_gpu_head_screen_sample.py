"""The sampled decode step through the screened lm_head (lm_head_screen.hip's top-k mode +
sample_list_kernel): the ids of the full-head sampled step, bit for bit, with the same seed.

TopKLogitsWarper keeps {c : s_c >= k-th largest s} (ties kept).  The screen bounds every
processed score, lb_c <= s_c <= ub_c; the k-th largest of the workgroups' maxima of lb is a
threshold T <= the k-th largest s, so recomputing exactly every 16-column unit whose maximum of
ub reaches T and keeping the scores >= T gives a superset of the top-k set, which the list
sampler sorts and cuts exactly as the dense sampler does its row.

The switches are read once per process, so each setting runs in a child process (as
tests/test_gpu_head_screen.py): a two-layer copy of the TTS-1 arch (hidden 2048, the real
193,856 vocabulary, tied) and tts1-max-2l (hidden 4096, untied)."""

import functools
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (temperature, top_k, top_p, repetition penalty, frequency penalty)
SETTINGS = [(0.8, 50, 1.0, 1.1, 0.0), (0.7, 20, 0.9, 1.4, 0.0), (1.0, 5, 1.0, 1.0, 0.3)]
ROWS = {"tts1-2l": (1, 8, 16), "tts1-max-2l": (1, 8)}

CHILD = r'''
import dataclasses, json, os, sys
import torch
sys.path.insert(0, os.path.join(sys.argv[1], "tts-max_amd"))
from tts_amd import configs, synth
from tts_amd.speechlm import MI355XSpeechLM
name, mode = sys.argv[2], sys.argv[3]
arch = dataclasses.replace(configs.LM_ARCHS["tts1"], name="tts1-2l", num_layers=2) if name == "tts1-2l" \
    else configs.LM_ARCHS[name]
SETTINGS, ROWS = json.loads(sys.argv[4]), json.loads(sys.argv[5])
vocab = configs.vocab_for(arch)
w = synth.lm_weights_device(arch, 0x5EED, torch.device("cuda", 0))
head = w["model.embed_tokens.weight" if arch.tie_word_embeddings else "lm_head.weight"]
if mode == "twins":
    head[1::2] = head[0::2]
if mode == "outliers":  # heavy-tailed rows: every 7th row x8, one element in 64 of the matrix x40
    g = torch.Generator(device=head.device).manual_seed(5)
    head[::7] *= 8
    mask = torch.rand(head.shape, generator=g, device=head.device) < 1.0 / 64
    head[mask] *= 40
m = MI355XSpeechLM(arch, w, max_batch=16, max_seq_len=128, id_to_code=vocab.id_to_code())
del w, head
torch.cuda.empty_cache()
eos = vocab.speech_end_id
prompts = lambda rows: [synth.synthetic_prompt(vocab, 7 + u, 8 + u % 5, 10 + 2 * u) for u in range(rows)]
out = {}
if mode == "twins":  # odd k, penalty 1.0: the tied pair at the k-th value is kept whole
    for rows in (1, 8):
        p = prompts(rows)
        out[f"twins/{rows}"] = m.generate_batch(p, max_length=max(map(len, p)) + 40, min_new_tokens=30, eos_token_id=eos,
                                                do_sample=True, temperature=1.0, top_k=5, top_p=1.0,
                                                repetition_penalty=1.0, seed=99 + rows)
else:
    for rows in ROWS:
        p = prompts(rows)
        L = max(map(len, p)) + 40
        for T, k, tp, rep, freq in (SETTINGS if mode == "plain" else SETTINGS[:1]):
            out[f"{rows}/{T}/{k}"] = m.generate_batch(p, max_length=L, min_new_tokens=30, eos_token_id=eos, do_sample=True,
                                                      temperature=T, top_k=k, top_p=tp, repetition_penalty=rep,
                                                      frequency_penalty=freq, seed=1000 + rows)
    if mode == "plain":
        p = prompts(3)
        L = max(map(len, p)) + 40
        kw = dict(min_new_tokens=30, eos_token_id=eos, repetition_penalty=1.1)
        out["greedy"] = m.generate_batch(p, max_length=L, **kw)
        out["top1"] = m.generate_batch(p, max_length=L, do_sample=True, temperature=0.8, top_k=1, seed=3, **kw)
        skw = dict(do_sample=True, temperature=0.8, top_k=50, seed=77, **kw)
        out["batch3"] = m.generate_batch(p, max_length=L, **skw)
        chunks = list(m.generate_stream(p, max_length=L, chunk=7, **skw))
        out["stream3"] = chunks[-1][0]
        out["stream_chunks"] = len(chunks)
        from tts_amd.serving import ContinuousBatcher
        b = ContinuousBatcher(m, n_slots=3, eos_token_id=eos, min_new_tokens=8, repetition_penalty=1.1, do_sample=True,
                              temperature=0.8, top_k=50, chunk=5)
        p4 = prompts(4)
        futs = [b.submit(q, n, seed=500 + i) for i, (q, n) in enumerate(zip(p4, (12, 40, 40, 30)))]
        while not all(f.done() for f in futs):  # (the fourth request is admitted when the first row frees)
            b._run_guarded()
        out["slots"] = [f.result() for f in futs]
m.close()
print(json.dumps(out))
'''


@functools.lru_cache(maxsize=None)
def _run(setting, arch, mode="plain"):
    env = dict(os.environ)
    for k in ("TTS_HEAD_SCREEN", "TTS_HEAD_SCREEN_CHECK", "TTS_HEAD_SCREEN_WAIT", "TTS_HEAD_SCREEN_DIAG"):
        env.pop(k, None)
    if setting:
        k, v = setting.split("=")
        env[k] = v
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, arch, mode, json.dumps(SETTINGS), json.dumps(ROWS[arch])],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{setting or 'default'} ({arch}, {mode}): rc {r.returncode}\n{r.stderr[-2000:]}"
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("setting", [None, "TTS_HEAD_SCREEN_WAIT=0", "TTS_HEAD_SCREEN_WAIT=1"])
@pytest.mark.parametrize("arch", ["tts1-2l", "tts1-max-2l"])
def test_screened_sampled_step_draws_the_full_heads_ids(arch, setting):
    full = _run("TTS_HEAD_SCREEN=0", arch)
    got = _run(setting, arch)
    n = 0
    for rows in ROWS[arch]:
        for T, k, *_ in SETTINGS:
            case = f"{rows}/{T}/{k}"
            assert got[case] == full[case], f"{arch} {case} ({setting}): ids differ from the full head's"
            assert all(len(r) >= 30 for r in full[case])
            n += sum(len(r) for r in full[case])
    assert n >= 30 * 3 * sum(ROWS[arch])


def test_top_k_one_is_greedy():
    got = _run(None, "tts1-2l")
    assert got["top1"] == got["greedy"]
    assert got["top1"] == _run("TTS_HEAD_SCREEN=0", "tts1-2l")["greedy"]


@pytest.mark.parametrize("mode", ["plain", "outliers"])
def test_check_mode_finds_every_score_between_its_bounds(mode):
    """Every unit recomputed; an exact score outside [lb, ub] raises (both sides matter for top-k)."""
    checked = _run("TTS_HEAD_SCREEN_CHECK=1", "tts1-2l", mode if mode != "plain" else "check")
    full = _run("TTS_HEAD_SCREEN=0", "tts1-2l", mode if mode != "plain" else "check")
    assert checked == full and len(full) == len(ROWS["tts1-2l"])
    if mode == "outliers":
        assert _run(None, "tts1-2l", mode) == full


def test_ties_at_the_kth_value_are_kept_whole():
    twins = _run(None, "tts1-2l", "twins")
    full = _run("TTS_HEAD_SCREEN=0", "tts1-2l", "twins")
    assert twins == full
    # (every score has an exact twin: with k = 5 the fifth and sixth values tie and both are kept;
    # that the sampler keeps all six ids is asserted on its probs in
    # test_list_sampler_keeps_the_tied_pair_at_the_kth_value; here the screen must have listed both
    # members of the pair for the draws to equal the full head's, and both parities get drawn)
    ids = [i for rows in twins.values() for r in rows for i in r]
    assert len({i % 2 for i in ids}) == 2


def test_every_surface_draws_the_same_ids():
    got, full = _run(None, "tts1-2l"), _run("TTS_HEAD_SCREEN=0", "tts1-2l")
    assert got["stream_chunks"] > 2
    for key in ("batch3", "stream3", "slots"):
        assert got[key] == full[key], key
    assert got["stream3"] == got["batch3"]
    assert [len(r) for r in got["slots"]][0] <= 12 and len(got["slots"]) == 4


def _plan(arch_name, rows, top_k):
    import dataclasses

    from tts_amd import configs
    from tts_amd.speechlm import step_plan

    arch = configs.LM_ARCHS[arch_name]
    return step_plan(dataclasses.replace(arch, num_layers=2), rows, top_k=top_k)


def test_sampled_step_plan():
    from tts_amd import _lib

    _lib.load_library().tts_debug_step_plan_sampled  # (the symbol: missing before this feature)
    for arch, rows in [("tts1", 1), ("tts1", 8), ("tts1", 16), ("tts1-max", 1), ("tts1-max", 8)]:
        p = _plan(arch, rows, 50)
        assert any(k.startswith("head_screen_kernel<") and k.endswith(", true>") for k in p), (arch, rows, p)
        assert "sample_list_kernel" in p and "sample_kernel" not in p, (arch, rows, p)
        assert not [k for k in p if k.startswith("wgemm_kernel<") and k.split(", ")[7] == "3"], (arch, rows, p)  # EPI_LOGITS
    for arch, rows, k in [("tts1", 17, 50), ("tts1", 8, 65), ("tts1-max", 9, 50), ("tts1", 32, 50)]:
        p = _plan(arch, rows, k)
        assert not [x for x in p if x.startswith("head_screen_kernel<")], (arch, rows, k, p)
        assert "sample_kernel" in p and [x for x in p if x.startswith("wgemm_kernel<") and x.split(", ")[7] == "3"]


def test_bench_entries():
    import dataclasses

    from tts_amd import configs
    from tts_amd.speechlm import MI355XSpeechLM

    arch = dataclasses.replace(configs.LM_ARCHS["tts1"], name="tts1-2l", num_layers=2)
    m = MI355XSpeechLM.synthetic(arch, max_batch=8, max_seq_len=128)
    for rows in (1, 8):
        ms10, b10 = m.bench_kernel("sample_screened", rows=rows, ctx=64, iters=3)
        ms11, b11 = m.bench_kernel("sample_full", rows=rows, ctx=64, iters=3)
        assert ms10 > 0 and ms11 > 0 and 0 < b10 < b11, (rows, b10, b11)
    m.close()


# ---------------------------------------------------------------- the list sampler alone ----
@pytest.fixture(scope="module")
def lib():
    from tts_amd import _lib

    return _lib.load_library()


def _dense(lib, logits, T, k, p, seed=7, step=0, parts=0):
    from tts_amd import _lib

    B, V = logits.shape
    d = logits.cuda().contiguous()
    probs = torch.zeros_like(d)
    tok = torch.empty(B, dtype=torch.int32, device="cuda")
    pm = None
    if parts:  # the maxima of `parts` column blocks, the top-k bound the engine's lm_head gives
        x = torch.nn.functional.pad(d, (0, (-V) % parts), value=float("-inf")).view(B, parts, -1)
        pm = x.max(dim=2).values.contiguous()
    _lib.check(lib.tts_op_sample(d.data_ptr(), B, V, T, k, p, seed, step, pm.data_ptr() if parts else None, parts,
                                 probs.data_ptr(), tok.data_ptr(), None))
    torch.cuda.synchronize()
    return probs.cpu(), tok.cpu()


def _list(lib, scores, ids, counts, V, T, k, p, seed=7, step=0):
    from tts_amd import _lib

    B, cap = scores.shape
    s, i, c = scores.cuda().contiguous(), ids.to(torch.int32).cuda().contiguous(), counts.to(torch.int32).cuda()
    probs = torch.zeros(B, V, device="cuda")
    tok = torch.empty(B, dtype=torch.int32, device="cuda")
    _lib.check(lib.tts_op_sample_list(s.data_ptr(), i.data_ptr(), c.data_ptr(), B, cap, V, T, k, p, seed, step,
                                      probs.data_ptr(), tok.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(c.cpu(), counts.to(torch.int32))  # (only read)
    return probs.cpu(), tok.cpu()


def _compare(lib, logits, keep, T, k, p, parts=0):
    """Lists of the `keep[b]` largest entries of each row, in a scrambled order, against the dense
    rows that hold those entries and -inf elsewhere."""
    B, V = logits.shape
    cap = max(keep) + 3
    g = torch.Generator().manual_seed(11)
    scores, ids = torch.full((B, cap), 123.0), torch.full((B, cap), -1, dtype=torch.int64)  # (the tails: never read)
    dense = torch.full((B, V), float("-inf"))
    for b in range(B):
        top = torch.topk(logits[b], keep[b]).indices
        top = top[torch.randperm(keep[b], generator=g)]
        scores[b, :keep[b]], ids[b, :keep[b]] = logits[b, top], top
        dense[b, top] = logits[b, top]
    pd, td = _dense(lib, dense, T, k, p, parts=parts)
    pl, tl = _list(lib, scores, ids, torch.tensor(keep), V, T, k, p)
    assert torch.equal(tl, td), (tl, td)
    assert torch.equal(pl.view(torch.int32), pd.view(torch.int32))  # bit-equal
    assert all(float(pd[b].sum()) > 0.99 for b in range(B))
    return pl


@pytest.mark.parametrize("T,k,p", [(0.8, 50, 1.0), (0.7, 20, 0.9), (1.0, 1, 1.0), (1.3, 5, 0.5), (0.6, 1024, 0.95)])
@pytest.mark.parametrize("parts", [0, 256])
def test_list_sampler_equals_the_dense_sampler(lib, T, k, p, parts):
    """The rows of test_gpu_sampling.py::test_sample_distribution_matches_oracle."""
    V = 193856
    g = torch.Generator().manual_seed(k * 10 + parts)
    logits = (torch.randn(4, V, generator=g) * 3).to(torch.bfloat16).float()  # bf16 ties
    logits[1, :60] = 11.0  # a tie block at the top
    logits[2, 5] = float("-inf")  # masked EOS
    logits[3] = torch.randn(V, generator=g) * 0.01  # nearly flat row
    _compare(lib, logits, [1500, 1200 + parts, 2048, 1100], T, k, p, parts)


def test_list_sampler_long_list_takes_the_radix_select(lib):
    g = torch.Generator().manual_seed(2)
    logits = torch.stack([(torch.arange(20000) * 0.001 - 12.0)[torch.randperm(20000, generator=g)] for _ in range(2)])
    assert all(len(set(logits[b].tolist())) == 20000 for b in range(2))
    _compare(lib, logits, [5000, 2049], 0.8, 50, 0.95)


def test_list_sampler_keeps_the_tied_pair_at_the_kth_value(lib):
    """Every value twice: k = 5 cuts between the two of a pair, and both must be kept (6 ids)."""
    g = torch.Generator().manual_seed(6)
    half = torch.stack([(torch.arange(1500) * 0.01 - 7.0)[torch.randperm(1500, generator=g)] for _ in range(2)])
    logits = half.repeat_interleave(2, dim=1)  # ids 2i and 2i + 1 tie
    for keep in ([40, 3000], [6, 7]):
        pl = _compare(lib, logits, keep, 1.0, 5, 1.0)
        for b in range(2):
            kept = torch.nonzero(pl[b]).ravel().tolist()
            top = torch.topk(half[b], 3).indices.tolist()
            assert sorted(kept) == sorted([2 * i for i in top] + [2 * i + 1 for i in top]), (b, kept)


def test_list_sampler_empty_list_gives_token_zero(lib):
    """No candidate (the producer found none: all-NaN scores, or its recompute switched off by the
    timing probe): nothing to draw from — token 0 and no probs, never an index read from the list."""
    scores, ids = torch.full((3, 64), float("nan")), torch.full((3, 64), 0x7FFFFFF0, dtype=torch.int64)
    scores[1, :4], ids[1, :4] = torch.tensor([1.0, 3.0, 2.0, 0.5]), torch.tensor([9, 7, 5, 3])
    probs, tok = _list(lib, scores, ids, torch.tensor([0, 4, 0]), 100, 0.8, 50, 1.0)
    assert tok.tolist()[0] == 0 and tok.tolist()[2] == 0 and tok.tolist()[1] in (9, 7, 5, 3)
    assert float(probs[0].sum()) == 0 and float(probs[2].sum()) == 0 and abs(float(probs[1].sum()) - 1) < 1e-5


def test_list_sampler_list_shorter_than_k(lib):
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(2, 2000, generator=g)
    _compare(lib, logits, [30, 1], 0.9, 50, 1.0)
