"""Same-box A/B of the per-request slot batch's decode step (tts_slots_open_per_request: every
row's sampling settings read from a device table) against the uniform sampled step, and of this
build's uniform steps against an earlier build's (TTS_LIB_PATH: the parent commit's library).

Each library in its own child process, alternating, two rounds: the spread between two identical
runs is the noise a difference must beat.  Per child, on a slot batch of ROWS rows that all decode
(300 tokens a row, min_new_tokens = the length, so no row stops):
  slots_sampled_us   the replayed uniform sampled step (T 0.8 / top_k 50 / penalty 1.4), wall clock over
                     the tts_slots_step calls: the baseline of the per-row figures
  rows_sampled_us    the per-row step, every row with those settings          (this build only)
  rows_half_us       the per-row step, every second row greedy (penalty 1.1)  (this build only)
  rows_dense_us      the per-row step after a top_k 100 request moved it to the full lm_head
  greedy_step_us / sampled_step_us   the uniform steps of tts_generate (device timing): parent vs this build
and md5s of the ids: the uniform ids must match between the builds, and the per-row all-sampled ids
must match the uniform sampled ones (same settings, same keys).
usage: python scripts/per_request_probe.py [--parent-lib PATH] [ARCH:ROWS ...] | tee profiles/per_request_probe.txt
       (default workloads: tts1:1 tts1:8 tts1:16 tts1-max:8; without --parent-lib only this build runs)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import ctypes, hashlib, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tts-max_amd"))
from tts_amd import _lib, configs, synth
from tts_amd.speechlm import MI355XSpeechLM
arch, rows, new = configs.LM_ARCHS[sys.argv[2]], int(sys.argv[3]), int(sys.argv[4])
m = MI355XSpeechLM.synthetic(arch, max_batch=rows, max_seq_len=720)
L, h = m._lib, m._h
vocab = configs.vocab_for(arch)
eos = vocab.speech_end_id
ps = [synth.synthetic_prompt(vocab, u, 39, 150) for u in range(rows)]
pi32 = ctypes.POINTER(ctypes.c_int32)
def gp(T, k, pen):
    return _lib.GenParams(max_length=0, min_new_tokens=new, eos_token_id=eos, do_sample=1 if T > 0 else 0,
                          repetition_penalty=pen, temperature=T if T > 0 else 1.0, top_p=1.0, top_k=k, seed=7,
                          frequency_penalty=0.0)
SAMPLED, GREEDY, WIDE = gp(0.8, 50, 1.4), gp(0.0, 50, 1.1), gp(0.8, 100, 1.4)
def slots(per_request, settings):
    """Opens a slot batch, admits one request per row, times the replayed steps (wall clock)."""
    opener = L.tts_slots_open_per_request if per_request else L.tts_slots_open
    _lib.check(opener(h, ctypes.byref(SAMPLED), rows, None))
    for u in range(rows):
        arr = np.asarray(ps[u], dtype=np.int32)
        seed = ctypes.c_uint64(1000 + u)
        if per_request:
            _lib.check(L.tts_slots_add_params(h, u, arr.ctypes.data_as(pi32), len(arr), new, ctypes.byref(settings[u]),
                                              ctypes.byref(seed)))
        else:
            _lib.check(L.tts_slots_add_seeded(h, u, arr.ctypes.data_as(pi32), len(arr), new, seed))
    act = ctypes.c_int32(0)
    _lib.check(L.tts_slots_step(h, 20, ctypes.byref(act)))  # warm
    n = new - 1 - 20 - 4
    t0 = time.perf_counter()
    _lib.check(L.tts_slots_step(h, n, ctypes.byref(act)))
    dt = time.perf_counter() - t0
    assert act.value == rows, act.value
    _lib.check(L.tts_slots_step(h, 8, ctypes.byref(act)))
    buf = np.zeros(new + 8, dtype=np.int32)
    cnt, fin = ctypes.c_int32(0), ctypes.c_int32(0)
    ids = []
    for u in range(rows):
        _lib.check(L.tts_slots_read(h, u, buf.ctypes.data_as(pi32), len(buf), ctypes.byref(cnt), ctypes.byref(fin)))
        ids.append(buf[:cnt.value].tolist())
        _lib.check(L.tts_slots_release(h, u))
    return round(dt / n * 1e6, 1), hashlib.md5(str(ids).encode()).hexdigest()[:10]
r = {}
with m.lock:
    r["slots_sampled_us"], r["slots_md5"] = slots(False, None)
    if hasattr(L, "tts_slots_open_per_request"):
        r["rows_sampled_us"], r["rows_md5"] = slots(True, [SAMPLED] * rows)
        if rows > 1:
            r["rows_half_us"], _ = slots(True, [SAMPLED if u % 2 == 0 else GREEDY for u in range(rows)])
        r["rows_dense_us"], r["rows_dense_md5"] = slots(True, [WIDE] + [SAMPLED] * (rows - 1))
kw = dict(max_length=len(ps[0]) + new, min_new_tokens=new, eos_token_id=eos)
for _ in range(2):
    out = m.generate_batch(ps, do_sample=True, temperature=0.8, top_k=50, repetition_penalty=1.4, seed=2024, **kw)
a, b, k = m.last_timing()
r["sampled_step_us"] = round(b / k * 1000, 1)
r["sampled_md5"] = hashlib.md5(str(out).encode()).hexdigest()[:10]
for _ in range(2):
    out = m.generate_batch(ps, repetition_penalty=1.1, **kw)
a, b, k = m.last_timing()
r["greedy_step_us"] = round(b / k * 1000, 1)
r["greedy_md5"] = hashlib.md5(str(out).encode()).hexdigest()[:10]
m.close()
print(json.dumps(r))
'''


def child(arch, rows, env, new=300):
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT, arch, str(rows), str(new)], env=env, capture_output=True,
                         text=True, timeout=420)
    if out.returncode != 0:
        print(f"FAILED rc={out.returncode} {out.stderr[-600:]}", flush=True)
        sys.exit(1)
    return json.loads(out.stdout.strip().splitlines()[-1])


args = sys.argv[1:]
parent = None
if args and args[0] == "--parent-lib":
    parent = os.path.abspath(args[1])
    args = args[2:]
base = {k: v for k, v in os.environ.items() if k != "TTS_LIB_PATH"}
builds = ([("parent", dict(base, TTS_LIB_PATH=parent))] if parent else []) + [("this", base)]
for w in args or ["tts1:1", "tts1:8", "tts1:16", "tts1-max:8"]:
    arch, rows = w.split(":")[0], int(w.split(":")[1])
    got = {}
    for rd in range(2):
        for name, env in builds:
            r = child(arch, rows, env)
            got.setdefault(name, []).append(r)
            print(f"{arch} rows={rows} round {rd} {name}: {json.dumps(r)}", flush=True)
    t = got["this"]
    ok = all(x["rows_md5"] == x["slots_md5"] for x in t)
    for key in ("slots_md5", "sampled_md5", "greedy_md5"):
        ok = ok and len({x[key] for runs in got.values() for x in runs}) == 1
    line = f"{arch} rows={rows}: {'ids match' if ok else 'IDS DIFFER'}"
    for key in ("slots_sampled_us", "sampled_step_us", "greedy_step_us"):
        line += f"; {key} " + " / ".join(f"{name} {min(x[key] for x in runs)} (spread {abs(runs[0][key] - runs[-1][key]):.1f})"
                                         for name, runs in got.items())
    base_us = min(x["slots_sampled_us"] for x in t)
    for key in ("rows_sampled_us", "rows_half_us", "rows_dense_us"):
        if key in t[0]:
            v = min(x[key] for x in t)
            line += f"; {key} {v} ({v - base_us:+.1f} us over the uniform sampled slot step)"
    print(line, flush=True)
    if not ok:
        sys.exit(1)
