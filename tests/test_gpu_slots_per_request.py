"""Per-request sampling settings in the continuous batch (tts_slots_open_per_request /
tts_slots_add_params; serving.ContinuousBatcher(per_request=True)).

Requests with different temperature, top_k, top_p, penalties, min_new_tokens and stop id share one
captured decode step, whose kernels read each row's settings from a device table.  Rows never mix,
so every request's tokens must equal, id for id, the uniform path's: a one-slot ContinuousBatcher
opened with that request's settings, given the same prompt and seed.

The dense form (per-row full lm_head + per-row dense sampler) runs in-process on the small golden
model; the screened form (the screen's per-row top-k variant + the per-row list sampler) runs in
child processes, one per switch setting, as tests/test_gpu_head_screen_sample.py does.  There the
uniform reference of a request is a uniform batcher of the same slot count that serves it alone:
the decode GEMMs choose their form by the batch's row count (at hidden 2048 the down projection
runs K-sliced from 8 rows, another order of the same sums), so a row's logits carry the batch
shape's rounding and a sampled draw can differ between an 8-row and a one-row batch of the tree
as it stands, whatever the settings; measured here: the same requests differed with every head
switch, the full lm_head included, at 8 slots of hidden 2048 only."""

import functools
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _model():
    from tts_amd import configs
    from tts_amd.speechlm import MI355XSpeechLM

    z = np.load(os.path.join(GOLDEN, "lm_small.npz"))
    arch = configs.LM_ARCHS[str(z["arch"])]
    return MI355XSpeechLM.synthetic(arch, seed=int(z["seed"]), max_batch=4, max_seq_len=512), z


def _settings(eos, eos2):
    from tts_amd.serving import RequestSettings as RS

    return [
        RS(temperature=0.0, repetition_penalty=1.1, eos_token_id=eos),
        RS(temperature=0.0, repetition_penalty=1.0, eos_token_id=eos2, min_new_tokens=2),
        RS(temperature=0.8, top_k=50, top_p=1.0, repetition_penalty=1.1, eos_token_id=eos),
        RS(temperature=0.7, top_k=20, top_p=0.9, repetition_penalty=1.4, frequency_penalty=0.3, eos_token_id=eos),
        RS(temperature=1.0, top_k=1, top_p=1.0, repetition_penalty=1.0, eos_token_id=eos),
    ]


def _uniform(m, st, prompt, n, seed):
    """The uniform path: a one-slot batcher opened with the request's settings."""
    from tts_amd.serving import ContinuousBatcher

    b = ContinuousBatcher(m, n_slots=1, eos_token_id=st.eos_token_id, min_new_tokens=st.min_new_tokens,
                          repetition_penalty=st.repetition_penalty, do_sample=st.do_sample,
                          temperature=st.temperature if st.do_sample else 1.0, top_k=st.top_k, top_p=st.top_p,
                          frequency_penalty=st.frequency_penalty, seed=1, chunk=5)
    return b.generate([prompt], n, seed=seed)[0]


@pytest.fixture(scope="module")
def dense():
    """The model, 7 requests over 5 settings, and each request's uniform-path tokens (computed once)."""
    m, z = _model()
    rng = np.random.default_rng(3)
    base = z["prompt_ids"][:int(z["prompt_lens"][0])].tolist()
    V = m.arch.vocab_size
    prompts = [base[:n] + rng.integers(0, V, 5).tolist() for n in (10, 40, 7, 25, 60, 3, 33)]
    max_new = [12, 30, 5, 18, 9, 26, 14]
    free = m.generate_batch([prompts[0]], max_length=len(prompts[0]) + 30, eos_token_id=-1, repetition_penalty=1.1)[0]
    eos = free[len(free) // 2]  # some rows stop on EOS before their max_new
    free2 = m.generate_batch([prompts[1]], max_length=len(prompts[1]) + 30, eos_token_id=-1, repetition_penalty=1.0)[0]
    eos2 = free2[len(free2) // 2]
    S = _settings(eos, eos2)
    which = [0, 1, 2, 3, 4, 2, 0]
    seeds = [100 + i for i in range(7)]
    reqs = [(prompts[i], max_new[i], seeds[i], S[which[i]]) for i in range(7)]
    ref = [_uniform(m, st, p, n, sd) for p, n, sd, st in reqs]
    assert any(len(r) < n for r, n in zip(ref, max_new)), "no request stopped on its EOS"
    assert len({tuple(r) for r in ref}) == 7
    yield m, reqs, ref, S
    m.close()


def test_keywords_and_symbols_exist():
    """(fails without the feature by construction)"""
    import inspect

    from tts_amd import _lib, serving

    lib = _lib.load_library()
    for s in ("tts_slots_open_per_request", "tts_slots_add_params"):
        assert hasattr(lib, s), s
    assert "per_request" in inspect.signature(serving.ContinuousBatcher.__init__).parameters
    assert "settings" in inspect.signature(serving.ContinuousBatcher.submit).parameters
    assert "per_request" in inspect.signature(serving.LLM.__init__).parameters
    assert serving.RequestSettings(temperature=0.5).do_sample and not serving.RequestSettings().do_sample


def test_per_request_batch_equals_the_uniform_path(dense):
    from tts_amd.serving import ContinuousBatcher

    m, reqs, ref, _ = dense
    b = ContinuousBatcher(m, n_slots=3, chunk=4, per_request=True, seed=5)
    got = b.generate([r[0] for r in reqs], [r[1] for r in reqs], seed=[r[2] for r in reqs],
                     settings=[r[3] for r in reqs])  # 7 requests over 5 settings through 3 rows
    assert got == ref


def test_background_thread_with_requests_submitted_while_others_run(dense):
    from tts_amd.serving import ContinuousBatcher

    m, reqs, ref, _ = dense
    b = ContinuousBatcher(m, n_slots=2, chunk=3, per_request=True, seed=5)
    b.start()
    try:
        futs = []
        for i, (p, n, sd, st) in enumerate(reqs):
            futs.append(b.submit(p, n, seed=sd, settings=st))
            if i == 2:
                futs[0].result(timeout=60)  # (the rest are submitted while others run)
        assert [f.result(timeout=60) for f in futs] == ref
    finally:
        b.close()


def test_requests_without_settings_take_the_batch_defaults(dense):
    from tts_amd.serving import ContinuousBatcher

    m, reqs, ref, S = dense
    st = S[3]
    b = ContinuousBatcher(m, n_slots=2, chunk=4, per_request=True, eos_token_id=st.eos_token_id,
                          repetition_penalty=st.repetition_penalty, do_sample=True, temperature=st.temperature,
                          top_k=st.top_k, top_p=st.top_p, frequency_penalty=st.frequency_penalty, seed=9)
    p, n, sd, _ = reqs[3]
    got = b.generate([p, reqs[0][0]], [n, reqs[0][1]], seed=[sd, reqs[0][2]], settings=[None, reqs[0][3]])
    assert got == [ref[3], ref[0]]


def test_llm_facade_with_a_list_of_sampling_params(dense):
    from tts_amd.serving import LLM

    m, reqs, ref, _ = dense

    def sp(n, sd, st):
        return type("SP", (), dict(max_tokens=n, seed=sd, temperature=st.temperature, top_k=st.top_k if st.do_sample else -1,
                                   top_p=st.top_p, repetition_penalty=st.repetition_penalty,
                                   frequency_penalty=st.frequency_penalty, min_tokens=st.min_new_tokens,
                                   stop_token_ids=[st.eos_token_id]))()

    llm = LLM(m, n_slots=3, chunk=4, per_request=True)
    outs = llm.generate(prompt_token_ids=[r[0] for r in reqs], sampling_params=[sp(*r[1:]) for r in reqs])
    assert [o.outputs[0].token_ids for o in outs] == ref
    one = llm.generate(prompt_token_ids=reqs[2][0], sampling_params=sp(*reqs[2][1:]))  # (no new batcher, no reopen)
    assert one[0].outputs[0].token_ids == ref[2] and len(llm._batchers) == 1
    with pytest.raises(NotImplementedError):
        llm.generate(prompt_token_ids=reqs[0][0], sampling_params=type("SP", (), dict(temperature=0.8, top_k=-1))())


def test_http_app_passes_the_settings_through(dense):
    import dataclasses

    from fastapi.testclient import TestClient

    from tts_amd.serving import ContinuousBatcher, create_app

    m, reqs, ref, _ = dense
    b = ContinuousBatcher(m, n_slots=3, chunk=4, per_request=True, seed=5)
    with TestClient(create_app(b)) as client:
        results = [None] * len(reqs)

        def post(i):
            p, n, sd, st = reqs[i]
            results[i] = client.post("/generate", json=dict(prompt_token_ids=p, max_tokens=n, seed=sd,
                                                            **dataclasses.asdict(st)))

        threads = [threading.Thread(target=post, args=(i,)) for i in range(len(reqs))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert [r.status_code for r in results] == [200] * len(reqs)
        assert [r.json()["token_ids"] for r in results] == ref
        bad = client.post("/generate", json=dict(prompt_token_ids=reqs[0][0], max_tokens=4, temperature=0.5, top_k=0))
        assert bad.status_code == 400
    b.close()
    uniform = ContinuousBatcher(m, n_slots=1, repetition_penalty=1.1)
    with TestClient(create_app(uniform)) as client:
        r = client.post("/generate", json=dict(prompt_token_ids=reqs[0][0], max_tokens=4, temperature=0.5))
        assert r.status_code == 400
    uniform.close()


def test_invalid_requests_fail_alone(dense):
    from tts_amd import _lib
    from tts_amd.serving import ContinuousBatcher, RequestSettings as RS

    m, reqs, ref, S = dense
    eos = S[0].eos_token_id
    bad = [RS(temperature=-0.5, eos_token_id=eos), RS(temperature=0.8, top_k=0, eos_token_id=eos),
           RS(temperature=0.8, top_k=50, top_p=0.0, eos_token_id=eos), RS(temperature=0.0, repetition_penalty=0.0)]
    b = ContinuousBatcher(m, n_slots=3, chunk=4, per_request=True, seed=5)
    futs, bad_futs = [], []
    for i, (p, n, sd, st) in enumerate(reqs):
        futs.append(b.submit(p, n, seed=sd, settings=st))
        if i < len(bad):
            bad_futs.append(b.submit(p, n, seed=sd, settings=bad[i]))
    while not all(f.done() for f in futs + bad_futs):
        b._run_guarded()
    assert b.error is None
    for f in bad_futs:
        with pytest.raises(_lib.TtsError):
            f.result()
    assert [f.result() for f in futs] == ref
    with pytest.raises(ValueError):
        ContinuousBatcher(m, n_slots=1).submit(reqs[0][0], 4, settings=S[0])


def test_add_params_on_a_uniform_batch_is_a_state_error(dense):
    import ctypes

    from tts_amd import _lib

    m, reqs, _, S = dense
    L, h = m._lib, m._h
    gp = S[0].gen_params()
    pi32 = ctypes.POINTER(ctypes.c_int32)
    arr = np.asarray(reqs[0][0], dtype=np.int32)
    with m.lock:
        m._slot_batcher = None
        _lib.check(L.tts_slots_open(h, ctypes.byref(gp), 2, None))
        st = L.tts_slots_add_params(h, 0, arr.ctypes.data_as(pi32), len(arr), 4, ctypes.byref(gp), None)
        assert st == _lib.TTS_E_STATE, st
        _lib.check(L.tts_slots_add_params(h, 0, arr.ctypes.data_as(pi32), len(arr), 4, None, None))  # (NULL p: fine)
        _lib.check(L.tts_slots_release(h, 0))


# ------------------------------------------------------------------ the screened form ----
SLOTS = {"tts1-2l": (3, 8, 16), "tts1-max-2l": (3, 8)}

CHILD = r'''
import dataclasses, json, os, sys
import torch
sys.path.insert(0, os.path.join(sys.argv[1], "tts-max_amd"))
from tts_amd import configs, synth
from tts_amd.serving import ContinuousBatcher, RequestSettings as RS
from tts_amd.speechlm import MI355XSpeechLM
name, slots = sys.argv[2], json.loads(sys.argv[3])
arch = dataclasses.replace(configs.LM_ARCHS["tts1"], name="tts1-2l", num_layers=2) if name == "tts1-2l" \
    else configs.LM_ARCHS[name]
vocab = configs.vocab_for(arch)
m = MI355XSpeechLM.synthetic(arch, seed=0x5EED, max_batch=max(slots), max_seq_len=128)
eos = vocab.speech_end_id
S = [RS(temperature=0.0, repetition_penalty=1.1, eos_token_id=eos, min_new_tokens=30),
     RS(temperature=0.0, repetition_penalty=1.0, eos_token_id=eos + 1, min_new_tokens=2),
     RS(temperature=0.8, top_k=50, top_p=1.0, repetition_penalty=1.1, eos_token_id=eos, min_new_tokens=30),
     RS(temperature=0.7, top_k=20, top_p=0.9, repetition_penalty=1.4, frequency_penalty=0.3, eos_token_id=eos, min_new_tokens=8),
     RS(temperature=1.0, top_k=1, top_p=1.0, repetition_penalty=1.0, eos_token_id=eos, min_new_tokens=30),
     RS(temperature=1.0, top_k=64, top_p=0.95, repetition_penalty=1.2, eos_token_id=eos, min_new_tokens=30)]
WIDE = RS(temperature=0.9, top_k=100, top_p=1.0, repetition_penalty=1.1, eos_token_id=eos, min_new_tokens=30)
N = max(slots) + 2
prompts = [synth.synthetic_prompt(vocab, 7 + u, 8 + u % 5, 10 + 2 * u) for u in range(N + 1)]
max_new = [24 + (5 * u) % 13 for u in range(N + 1)]
sets = [S[u % len(S)] for u in range(N)] + [WIDE]
seeds = [900 + u for u in range(N + 1)]
def uniform(u, n_slots):
    st = sets[u]
    b = ContinuousBatcher(m, n_slots=n_slots, eos_token_id=st.eos_token_id, min_new_tokens=st.min_new_tokens,
                          repetition_penalty=st.repetition_penalty, do_sample=st.do_sample,
                          temperature=st.temperature if st.do_sample else 1.0, top_k=st.top_k, top_p=st.top_p,
                          frequency_penalty=st.frequency_penalty, seed=1, chunk=6)
    return b.generate([prompts[u]], max_new[u], seed=seeds[u])[0]
out = {"ref1": [uniform(u, 1) for u in range(N + 1)]}
for n_slots in slots:
    # the uniform path at this batch shape: each request alone in a uniform batch of n_slots rows
    out[f"{n_slots}/ref"] = {str(u): uniform(u, n_slots) for u in list(range(n_slots + 2)) + [N]}
    # n_slots + 2 requests through n_slots rows, every top_k <= 64: the screened per-row step
    b = ContinuousBatcher(m, n_slots=n_slots, chunk=4, per_request=True, seed=3)
    idx = list(range(n_slots + 2))
    out[f"{n_slots}/mixed"] = b.generate([prompts[u] for u in idx], [max_new[u] for u in idx],
                                         seed=[seeds[u] for u in idx], settings=[sets[u] for u in idx])
    # a top_k = 100 request admitted while the others are mid-flight: one recapture to the dense form
    b = ContinuousBatcher(m, n_slots=n_slots, chunk=4, per_request=True, seed=3)
    first = list(range(n_slots - 1))
    futs = {u: b.submit(prompts[u], max_new[u], seed=seeds[u], settings=sets[u]) for u in first}
    b._run_guarded(); b._run_guarded()
    assert not any(f.done() for f in futs.values())
    futs[N] = b.submit(prompts[N], max_new[N], seed=seeds[N], settings=sets[N])
    futs[n_slots - 1] = b.submit(prompts[n_slots - 1], max_new[n_slots - 1], seed=seeds[n_slots - 1], settings=sets[n_slots - 1])
    while not all(f.done() for f in futs.values()):
        b._run_guarded()
    assert b.error is None, b.error
    out[f"{n_slots}/wide"] = {str(u): f.result() for u, f in futs.items()}
m.close()
print(json.dumps(out))
'''

SWITCHES = [None, "TTS_HEAD_SCREEN=0", "TTS_HEAD_SCREEN_WAIT=0", "TTS_HEAD_SCREEN_WAIT=1", "TTS_HEAD_SCREEN_CHECK=1"]


@functools.lru_cache(maxsize=None)
def _run(setting, arch):
    env = dict(os.environ)
    for k in ("TTS_HEAD_SCREEN", "TTS_HEAD_SCREEN_CHECK", "TTS_HEAD_SCREEN_WAIT", "TTS_HEAD_SCREEN_DIAG"):
        env.pop(k, None)
    if setting:
        k, v = setting.split("=")
        env[k] = v
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, arch, json.dumps(SLOTS[arch])], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, f"{setting or 'default'} ({arch}): rc {r.returncode}\n{r.stderr[-2000:]}"
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("setting", SWITCHES)
@pytest.mark.parametrize("arch", ["tts1-2l", "tts1-max-2l"])
def test_screened_per_row_step_equals_the_uniform_path(arch, setting):
    got = _run(setting, arch)
    ref1 = got["ref1"]
    assert all(len(r) >= 2 for r in ref1) and sum(len(r) for r in ref1) >= 20 * len(ref1)
    assert len({tuple(r) for r in ref1}) == len(ref1)
    for n_slots in SLOTS[arch]:
        ref = got[f"{n_slots}/ref"]
        if n_slots < 8:  # (one GEMM form up to 7 rows: the one-row batch's ids)
            assert all(ref[u] == ref1[int(u)] for u in ref), f"{arch} {n_slots} slots ({setting})"
        mixed = got[f"{n_slots}/mixed"]
        bad = [u for u in range(n_slots + 2) if mixed[u] != ref[str(u)]]
        assert not bad, f"{arch} {n_slots} slots ({setting}): requests {bad} differ from the uniform path"
        wide = got[f"{n_slots}/wide"]
        assert len(wide) == n_slots + 1 and str(len(ref1) - 1) in wide
        for u, ids in wide.items():
            assert ids == ref[u], f"{arch} {n_slots} slots, request {u} around the recapture ({setting})"
    if setting != "TTS_HEAD_SCREEN=0":  # (the switches change no id)
        full = _run("TTS_HEAD_SCREEN=0", arch)
        assert all(got[k] == full[k] for k in got if k == "ref1" or k.endswith("/ref"))
