"""Same-box measurement of the wide decode step (65..256 rows: tile GEMMs + the tile lm_head) beside
the narrow steps, and of this build's 32- and 64-row steps against an earlier build's
(TTS_LIB_PATH: the parent commit's library).

Each configuration in its own child process, alternating, two rounds: the spread between two
identical runs is the noise a difference must beat.  Configurations per row count: "this" (the
default), "chunked" (TTS_WIDE_HEAD=0: the wide step's lm_head as the 32-row decode head in chunks;
above 64 rows only) and "parent" (--parent-lib; up to 64 rows only, the parent's limit).  Per child,
a batch of ROWS rows that all decode (NEW tokens a row, min_new_tokens = the length, so no row stops):
  greedy_step_us / sampled_step_us   the replayed decode step of tts_generate (device timing), greedy
                                     (penalty 1.1) and sampled (T 0.8 / top_k 50 / penalty 1.4)
  codes_per_s                        rows / greedy step
  head_us / sample_head_us           the step's lm_head alone, and with its logits store + the dense
                                     sampler (tts_lm_bench_kernel 4 and 11: at > 64 rows what the
                                     step at that row count runs, so "chunked" times the chunked form)
  attn_us                            the decode attention of one layer at the mean context
  mem_gib                            device memory in use after load
and md5s of the ids: they must match between "this" and "parent" (the narrow steps are untouched).
usage: python scripts/wide_step_probe.py [--parent-lib PATH] [--new N] [ARCH:ROWS ...] | tee profiles/wide_step_probe.txt
       (default workloads: tts1:32 tts1:64 tts1:96 tts1:128 tts1:192 tts1:256 tts1-max:8 tts1-max:32
        tts1-max:64 tts1-max:128; without --parent-lib only this build runs)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import hashlib, json, os, sys
import torch
sys.path.insert(0, os.path.join(sys.argv[1], "tts-max_amd"))
from tts_amd import configs, synth
from tts_amd.speechlm import MI355XSpeechLM
arch, rows, new = configs.LM_ARCHS[sys.argv[2]], int(sys.argv[3]), int(sys.argv[4])
m = MI355XSpeechLM.synthetic(arch, max_batch=rows, max_seq_len=256 + new)
free, total = torch.cuda.mem_get_info()
r = {"mem_gib": round((total - free) / 2**30, 2)}
vocab = configs.vocab_for(arch)
eos = vocab.speech_end_id
ps = [synth.synthetic_prompt(vocab, u, 39, 150) for u in range(rows)]
kw = dict(max_length=len(ps[0]) + new, min_new_tokens=new, eos_token_id=eos)
for _ in range(2):
    out = m.generate_batch(ps, repetition_penalty=1.1, **kw)
a, b, k = m.last_timing()
r["greedy_step_us"] = round(b / k * 1000, 1)
r["codes_per_s"] = round(rows / (b / k / 1000))
r["greedy_md5"] = hashlib.md5(str(out).encode()).hexdigest()[:10]
for _ in range(2):
    out = m.generate_batch(ps, do_sample=True, temperature=0.8, top_k=50, repetition_penalty=1.4, seed=2024, **kw)
a, b, k = m.last_timing()
r["sampled_step_us"] = round(b / k * 1000, 1)
r["sampled_md5"] = hashlib.md5(str(out).encode()).hexdigest()[:10]
ctx = len(ps[0]) + new // 2
r["head_us"] = round(m.bench_kernel("lm_head", rows, ctx, 30)[0] * 1000, 1)
r["sample_head_us"] = round(m.bench_kernel("sample_full", rows, ctx, 30)[0] * 1000, 1)
r["attn_us"] = round(m.bench_kernel("attention", rows, ctx, 30)[0] * 1000, 1)
m.close()
print(json.dumps(r))
'''


def child(arch, rows, env, new):
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT, arch, str(rows), str(new)], env=env, capture_output=True,
                         text=True, timeout=420)
    if out.returncode != 0:
        print(f"FAILED rc={out.returncode} {out.stderr[-600:]}", flush=True)
        sys.exit(1)
    return json.loads(out.stdout.strip().splitlines()[-1])


args = sys.argv[1:]
parent, new = None, 120
while args and args[0] in ("--parent-lib", "--new"):
    if args[0] == "--parent-lib":
        parent = os.path.abspath(args[1])
    else:
        new = int(args[1])
    args = args[2:]
base = {k: v for k, v in os.environ.items() if k not in ("TTS_LIB_PATH", "TTS_WIDE_HEAD")}
for w in args or ["tts1:32", "tts1:64", "tts1:96", "tts1:128", "tts1:192", "tts1:256", "tts1-max:8", "tts1-max:32",
                  "tts1-max:64", "tts1-max:128"]:
    arch, rows = w.split(":")[0], int(w.split(":")[1])
    builds = [("this", base)]
    if rows > 64:
        builds.append(("chunked", dict(base, TTS_WIDE_HEAD="0")))
    elif parent:
        builds.insert(0, ("parent", dict(base, TTS_LIB_PATH=parent)))
    got = {}
    for rd in range(2):
        for name, env in builds:
            r = child(arch, rows, env, new)
            got.setdefault(name, []).append(r)
            print(f"{arch} rows={rows} round {rd} {name}: {json.dumps(r)}", flush=True)
    ok = all(len({x[key] for x in runs}) == 1 for runs in got.values() for key in ("greedy_md5", "sampled_md5"))
    if "parent" in got:
        ok = ok and all(got["parent"][0][key] == got["this"][0][key] for key in ("greedy_md5", "sampled_md5"))
    line = f"{arch} rows={rows}: {'ids reproduce' if ok else 'IDS DIFFER'}"
    for key in ("greedy_step_us", "sampled_step_us", "head_us", "sample_head_us"):
        line += f"; {key} " + " / ".join(f"{name} {min(x[key] for x in runs)} (spread {abs(runs[0][key] - runs[-1][key]):.1f})"
                                         for name, runs in got.items())
    t = got["this"]
    line += f"; codes/s {max(x['codes_per_s'] for x in t)}; attn_us {min(x['attn_us'] for x in t)}; mem_gib {t[0]['mem_gib']}"
    print(line, flush=True)
    if not ok:
        sys.exit(1)
