"""Where the dispatcher puts the workgroups of the one-row fused QKV + attention + o_proj launch
and of the gate/up launch behind it (run on the MI355X box; diagnostic library: make -C
tts-max_amd/csrc stamps).  The stamps build counts, per launch kind and block index, the XCC id
(HW_REG_XCC_ID) each workgroup ran on, and the distance mod 8 between the XCC ids of block 0 of a
gate/up launch and of the fused launch before it (lm_gemm_kernel.h xcc_record).  This script
replays the captured one-row step a few hundred times per trial (one greedy generation) and
answers, for the warm role's placement rule (lm_kernels.h WarmArgs):
  (a) does a block index of the gate/up launch land on the same XCD in every launch?
  (b) is that distance constant, and is it the fused grid size mod 8?
  (c) does each XCD get exactly every eighth block?
usage: python scripts/warm_xcd_probe.py [NEW_TOKENS] [TRIALS]"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tts-max_amd"))
from tts_amd import _lib, configs, synth  # noqa: E402

_lib.LIB_PATH = os.environ.get("TTS_LIB_PATH") or os.path.join(ROOT, "tts-max_amd", "tts_amd", "libtts_mi355x_stamps.so")
lib = _lib.load_library()
from tts_amd.speechlm import MI355XSpeechLM  # noqa: E402

n_new = int(sys.argv[1]) if len(sys.argv) > 1 else 300
trials = int(sys.argv[2]) if len(sys.argv) > 2 else 3
HIST, BLOCKS, DIST = 49152, 512, 49152 + 2 * 512 * 8  # (lm_gemm_kernel.h kXccHist, kXccBlocks, kXccDist)
N = 1 << 16
buf = np.zeros(N, dtype=np.uint64)
f = lib.tts_debug_stamps
f.argtypes = [ctypes.c_void_p, ctypes.c_int]

arch = configs.TTS1
p = synth.synthetic_prompt(configs.vocab_for(arch), 5, 39, 150)
m = MI355XSpeechLM.synthetic(arch, seed=0x5EED, max_batch=1, max_seq_len=len(p) + n_new + 20)
m.bench_kernel("gate_up", rows=1, ctx=64, iters=1)  # (allocates the stamps buffer outside any capture)
assert f(buf.ctypes.data, N) == 0  # (reads and clears)
print(f"TTS-1, one row, {n_new} new tokens per trial ({n_new} x {arch.num_layers} launches of each kind), {trials} trials")
homes = []
for t in range(trials):
    m.generate_batch([p], max_length=len(p) + n_new, min_new_tokens=n_new, eos_token_id=-1, repetition_penalty=1.1)
    assert f(buf.ctypes.data, N) == 0
    h = buf[HIST:HIST + 2 * BLOCKS * 8].astype(np.int64).reshape(2, BLOCKS, 8)
    dist = buf[DIST:DIST + 8].astype(np.int64)
    print(f"trial {t}: distance (gate/up block 0 XCC - fused block 0 XCC) mod 8, launches per value: {dist.tolist()}")
    for kind, name in ((0, "fused"), (1, "gate/up")):
        used = h[kind].sum(1) > 0
        nb = int(used.sum())
        hk = h[kind][used]
        single = int(((hk > 0).sum(1) == 1).sum())
        home = hk.argmax(1)
        every8 = int((((home - home[0]) % 8) == (np.arange(nb) % 8)).sum())
        per_xcd = np.bincount(home, minlength=8).tolist()
        print(f"  {name:8s} {nb} blocks, {int(hk[0].sum())} launches: blocks always on one XCD {single}/{nb}; "
              f"block b on XCD (home of block 0 + b) mod 8: {every8}/{nb}; blocks per XCD {per_xcd}; "
              f"block 0's XCC histogram {hk[0].tolist()}")
        if kind == 1:
            homes.append(home)
print("gate/up homes equal across trials:", all((x == homes[0]).all() for x in homes))
m.close()
