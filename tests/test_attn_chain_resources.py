"""The kernels that carry the decode attention chain keep inside their parent's registers: the
standalone attn_decode_kernel and the FATT instantiations of wgemm_kernel (the QKV launches
with the attention, and with o_proj behind it).  Compiles lm_attn.hip and lm_gemm_store.hip
for gfx950 with the Makefile's flags and the compiler's resource remarks and asserts that none
uses scratch memory or spills, and that none uses more VGPRs than at commit 0c6267a, the
parent of the change that shortened the chain (the numbers below, from a build of that commit
with the same compiler).  CPU only; in the manner of tests/test_attn_core_resources.py, whose
helpers it shares."""

import os
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_attn_core_resources as core  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(core.HIPCC), reason="hipcc not installed")

# VGPRs at the parent commit.  wgemm_kernel<WAVES, KU, MT_MAX, NG, KSPLIT, ASRC, NORM, EPI, R,
# EARLY, KSW, FROWS>: the keys are its template arguments.
PARENT_ATTN = {"attn_decode_kernel<64>": 116, "attn_decode_kernel<128>": 124}
PARENT_FATT = {
    # one row (EARLY), head dim 64
    (16, 2, 1, 1, 16, 1, 0, 0, 1, 1, 16, 0): 116,
    (16, 2, 1, 1, 16, 1, 0, 0, 2, 1, 16, 0): 116,
    (16, 2, 1, 1, 16, 1, 1, 0, 1, 1, 16, 0): 116,
    (16, 2, 1, 1, 16, 1, 1, 0, 2, 1, 16, 0): 116,
    # 2..16 rows (FROWS), head dim 64
    (16, 2, 1, 1, 16, 1, 0, 0, 1, 0, 16, 1): 116,
    (16, 2, 1, 1, 16, 1, 0, 0, 2, 0, 16, 1): 116,
    (16, 2, 1, 1, 16, 1, 1, 0, 1, 0, 16, 1): 116,
    (16, 2, 1, 1, 16, 1, 1, 0, 2, 0, 16, 1): 116,
    # 2..16 rows (FROWS), head dim 128
    (16, 4, 1, 1, 16, 1, 0, 0, 1, 0, 16, 1): 124,
    (16, 4, 1, 1, 16, 1, 0, 0, 2, 0, 16, 1): 124,
    (16, 4, 1, 1, 16, 1, 1, 0, 1, 0, 16, 1): 126,
    (16, 4, 1, 1, 16, 1, 1, 0, 2, 0, 16, 1): 126,
}


@pytest.fixture(scope="module")
def resources():
    import re

    with ThreadPoolExecutor(2) as ex:
        attn, store = ex.map(core._remarks, ["lm_attn.hip", "lm_gemm_store.hip"])
    got_attn = {f"attn_decode_kernel<{d}>": attn[f"_ZN3tts18attn_decode_kernelILi{d}EEEvNS_8AttnArgsE"]
                for d in (64, 128)}
    got_fatt = {}
    for name, res in store.items():
        m = re.match(r"_ZN3tts12wgemm_kernelI(.*)EEvNS_9WgemmArgsE$", name)
        if m:
            t = tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1)))
            if len(t) == 12 and core._is_fatt(t):
                got_fatt[t] = res
    return got_attn, got_fatt


def _check(key, r, parent):
    print(key, r, "parent", parent)
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (key, r)
    assert r["VGPRs"] <= parent, (key, r, parent)


def test_attention_kernels_stay_inside_the_parents_registers(resources):
    got_attn, _ = resources
    for k, parent in PARENT_ATTN.items():
        _check(k, got_attn[k], parent)


def test_fused_attention_launches_stay_inside_the_parents_registers(resources):
    _, got_fatt = resources
    # every fused instantiation of the parent is still there, and a new one has to be recorded
    assert set(got_fatt) == set(PARENT_FATT), sorted(set(got_fatt) ^ set(PARENT_FATT))
    for t, parent in PARENT_FATT.items():
        _check(t, got_fatt[t], parent)
