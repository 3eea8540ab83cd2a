"""Same-box A/B of the sampled decode step: the full bf16 lm_head + dense sampler
(TTS_HEAD_SCREEN=0, what every sampled step ran before the screen's top-k mode) against the
screened sampling head (default).  Each setting in its own child process, alternating, two
rounds (the spread between two identical runs is the noise the comparison must beat).  Per child:
the graph-replayed sampled step (T 0.8, top_k 50, repetition penalty 1.4; 300 tokens a row) and an
md5 of its ids (must match between the settings), the greedy step as context, and the isolated
heads: bench selectors sample_screened (10) / sample_full (11) / head_screened (8).  A last child
per workload counts the units the screen recomputed per launch (TTS_HEAD_SCREEN_DIAG=2: the sum
over every launch of the sampled head, the first tokens' after prefill included, by their number).
usage: python scripts/sample_head_probe.py [ARCH:ROWS ...]   (default: tts1:1 tts1:8 tts1:16 tts1-max:8)"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import json, os, sys, hashlib
sys.path.insert(0, os.path.join(sys.argv[1], "tts-max_amd"))
from tts_amd import configs, synth
from tts_amd.speechlm import MI355XSpeechLM
arch, rows, new = configs.LM_ARCHS[sys.argv[2]], int(sys.argv[3]), int(sys.argv[4])
m = MI355XSpeechLM.synthetic(arch, max_batch=rows, max_seq_len=720)
r = {}
if new >= 300:
    for k in ("sample_screened", "sample_full", "head_screened"):
        if k != "sample_full" and os.environ.get("TTS_HEAD_SCREEN") == "0":
            continue  # (the screened forms do not exist without the int8 copy)
        r[k] = round(m.bench_kernel(k, rows=rows, ctx=450, iters=64)[0] * 1000, 2)
vocab = configs.vocab_for(arch)
ps = [synth.synthetic_prompt(vocab, u, 39, 150) for u in range(rows)]
kw = dict(max_length=len(ps[0]) + new, min_new_tokens=new, eos_token_id=vocab.speech_end_id)
for _ in range(2):
    out = m.generate_batch(ps, do_sample=True, temperature=0.8, top_k=50, repetition_penalty=1.4, seed=2024, **kw)
a, b, k = m.last_timing()
r["sampled_step_us"] = round(b / k * 1000, 1)
r["steps"] = 2 * (k + 1)  # head launches of the two runs: each row's first token takes the same head
r["units"] = arch.vocab_size // 16
r["ids_md5"] = hashlib.md5(str(out).encode()).hexdigest()[:10]
if new >= 300:
    for _ in range(2):
        m.generate_batch(ps, repetition_penalty=1.1, **kw)
    a, b, k = m.last_timing()
    r["greedy_step_us"] = round(b / k * 1000, 1)
m.close()
print(json.dumps(r))
'''


def child(arch, rows, env, new=300):
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT, arch, str(rows), str(new)], env=env, capture_output=True,
                         text=True, timeout=420)
    if out.returncode != 0:
        print(f"FAILED rc={out.returncode} {out.stderr[-600:]}", flush=True)
        sys.exit(1)
    return json.loads(out.stdout.strip().splitlines()[-1]), out.stderr


base = {k: v for k, v in os.environ.items() if not k.startswith("TTS_HEAD_SCREEN")}
for w in sys.argv[1:] or ["tts1:1", "tts1:8", "tts1:16", "tts1-max:8"]:
    arch, rows = w.split(":")[0], int(w.split(":")[1])
    md5 = set()
    for rd in range(2):
        for name, extra in (("TTS_HEAD_SCREEN=0", {"TTS_HEAD_SCREEN": "0"}), ("default", {})):
            r, _ = child(arch, rows, dict(base, **extra))
            md5.add(r["ids_md5"])
            print(f"{arch} rows={rows} round {rd} {name}: {json.dumps(r)}", flush=True)
    r, err = child(arch, rows, dict(base, TTS_HEAD_SCREEN_DIAG="2"), new=60)
    md5ok = "ids match" if len(md5) == 1 else f"IDS DIFFER {sorted(md5)}"
    units = sum(int(n) for n in re.findall(r"head screen: (\d+) units recomputed", err))
    print(f"{arch} rows={rows}: {md5ok}; {units / r['steps']:.0f} of {r['units']} units recomputed per launch of the "
          f"sampled head (all rows together; {units} over {r['steps']} launches, the first tokens' included)", flush=True)
    if len(md5) != 1:
        sys.exit(1)
