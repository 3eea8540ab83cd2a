"""The decode attention core (lm_attn_core.h) keeps its bits: the md5 of score_decode's outputs
at contexts that put the tail wave (the one holding the new position) at every place the
core treats specially, against tests/golden/attn_tail_bits.json, which was recorded from the
build of the commit before the tail of the core was trimmed (the file says how).

The cases: the tail wave moving across a wave boundary and ending exactly on one, a second
pass, a context below one wave, rows with different tails in the 2..16-row fused launch, the
standalone kernel at 17 rows, and head dim 128 across its 512-position pass and at one row.

The md5 is a change detector: it pins the core to its own earlier bits.  That those bits are
RIGHT is checked by tests/test_gpu_attn_ops.py, which runs the attention kernels alone against
the float64 reference of oracle/attn_oracle.py."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_tail_bits.json")

# (arch, rows, L, n_last)
CASES = [
    ("tts1", 1, 140, 24),         # the tail wave moves across position 128 and hits base + PW == ctx
    ("tts1", 1, 1036, 24),        # a second pass begins at 1,024
    ("tts1", 2, 40, 24),          # ctx below one wave
    ("tts1", 3, 140, 24),         # rows with different tails in the 2..16-row fused launch
    ("tts1", 17, 160, 12),        # standalone kernel, rows from 160 down to 48
    ("tts1-max-2l", 8, 524, 24),  # head dim 128 across its 512-position pass
    ("tts1-max-2l", 1, 76, 24),   # head dim 128 at one row
]

# (the child of tests/test_gpu_fused_launch.py's fused = separate tests, same seeds)
CHILD = r'''
import hashlib, os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tts-max_amd"))
from tts_amd import configs
from tts_amd.speechlm import MI355XSpeechLM
arch = configs.LM_ARCHS[sys.argv[2]]
rows, L, n_last = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
m = MI355XSpeechLM.synthetic(arch, seed=0x5EED, max_batch=rows, max_seq_len=L + 8)
rng = np.random.default_rng(rows)
seqs = [rng.integers(0, arch.vocab_size, L - 7 * r).tolist() for r in range(rows)]
idx = rng.integers(0, arch.vocab_size, (rows, n_last, 64)).astype(np.int32)
out = m.score_decode(seqs, n_last, idx).numpy()
print(hashlib.md5(out.tobytes()).hexdigest(), float(np.abs(out).max()))
'''


def case_key(arch, rows, L, n_last):
    return f"{arch}:{rows}:{L}:{n_last}"


def run_case(arch, rows, L, n_last, env=None):
    """md5 of the case's score_decode outputs, computed in a fresh process."""
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, arch, str(rows), str(L), str(n_last)],
                       env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-2000:]
    md5, amax = r.stdout.strip().splitlines()[-1].split()
    assert float(amax) > 0.0
    return md5


@pytest.mark.parametrize("arch,rows,L,n_last", CASES)
def test_attention_tail_bits_unchanged(arch, rows, L, n_last):
    with open(GOLDEN) as f:
        golden = json.load(f)["md5"]
    assert run_case(arch, rows, L, n_last) == golden[case_key(arch, rows, L, n_last)]
