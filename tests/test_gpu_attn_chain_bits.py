"""The decode attention chain (lm_attn_core.h: the new position's score taken without patching
K, the maximum / sum / partial-O exchanges over the active waves only; lm_gemm_kernel.h: the
one-row split-K combine) keeps its bits: the md5 of score_decode's outputs against
tests/golden/attn_chain_bits.json, which was recorded from the build of the commit before
those changes (the file says how; `python tests/test_gpu_attn_chain_bits.py` prints it).

The cases are the contexts the code treats specially, not the workload's: the new position as
the last and the first slot of a wave (the select of its separately computed score), the
context crossing 256, 512 and 768 (the edges of the 4 / 8 / 12 / 16-wave ladder at head dim
64; 128, 256, 384 at head dim 128), 1,024 -> 1,025 (all 16 waves, then a second pass), a
context below one wave, rows with different tails in the 2..16-row launch, the standalone
kernel at 17 rows, and head dim 128 at 8 rows and at one row.  The positions scored are
ctx - 1 = L - n_last .. L - 1 (row r: L - 7 r).

Same child process, seeds and md5 as tests/test_gpu_attn_tail.py; that the bits are RIGHT is
tests/test_gpu_attn_ops.py's job."""

import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_attn_tail import case_key, run_case  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_chain_bits.json")

# (arch, rows, L, n_last)
CASES = [
    ("tts1", 1, 40, 8),            # ctx 33..40: below one wave
    ("tts1", 1, 70, 12),           # ctx - 1 = 63 (last slot of wave 0) and 64 (first slot of wave 1)
    ("tts1", 1, 260, 8),           # ctx crosses 256: 4 -> 5 active waves (ladder 4 -> 8)
    ("tts1", 1, 516, 8),           # ctx crosses 512: ladder 8 -> 12
    ("tts1", 1, 772, 8),           # ctx crosses 768: ladder 12 -> 16
    ("tts1", 1, 1028, 8),          # ctx 1,021..1,028: all 16 waves, then the second pass at 1,025
    ("tts1", 2, 262, 12),          # two rows, tails 251..262 and 244..255 (across 256)
    ("tts1", 3, 520, 12),          # three rows, tails 509..520, 502..513, 495..506 (across 512)
    ("tts1", 17, 270, 8),          # standalone kernel, rows from 270 down to 158 (ladder 4 and 8)
    ("tts1-max-2l", 8, 540, 8),    # head dim 128, 8 rows from 540 down to 491: across its 512-position pass
    ("tts1-max-2l", 8, 280, 8),    # head dim 128, 8 rows from 280 down to 231: across 256 (ladder 8 -> 12)
    ("tts1-max-2l", 1, 100, 8),    # head dim 128, one row: ctx - 1 = 96 is the first slot of wave 3
    ("tts1-max-2l", 1, 390, 8),    # head dim 128, one row across 384 (ladder 12 -> 16)
]


@pytest.mark.parametrize("arch,rows,L,n_last", CASES)
def test_attention_chain_bits_unchanged(arch, rows, L, n_last):
    with open(GOLDEN) as f:
        golden = json.load(f)["md5"]
    assert run_case(arch, rows, L, n_last) == golden[case_key(arch, rows, L, n_last)]


if __name__ == "__main__":  # record: run with the library built from the parent commit
    print(json.dumps({"md5": {case_key(*c): run_case(*c) for c in CASES}}, indent=1))
