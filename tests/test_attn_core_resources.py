"""The decode attention core (lm_attn_core.h) runs at the edge of the 128-VGPR budget of its
16-wave workgroups: the standalone attn_decode_kernel and the QKV launches that carry the
attention (the FATT instantiations of wgemm_kernel).  Compiles lm_attn.hip and
lm_gemm_store.hip for gfx950 with the Makefile's flags and the compiler's resource remarks and
asserts that none of them uses more VGPRs than at commit a1c161b (the numbers below, from a
build of that commit with the same compiler), and that none spills.  CPU only."""

import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tts-max_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# CXXFLAGS of tts-max_amd/csrc/Makefile
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result",
         "-Wno-unused-variable", "-munsafe-fp-atomics"]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# VGPRs at the parent commit.  wgemm_kernel<WAVES, KU, MT_MAX, NG, KSPLIT, ASRC, NORM, EPI, R,
# EARLY, KSW, FROWS>: the keys are its template arguments.
PARENT_ATTN = {"attn_decode_kernel<64>": 127, "attn_decode_kernel<128>": 128}
PARENT_FATT = {
    # one row (EARLY), head dim 64
    (16, 2, 1, 1, 16, 1, 0, 0, 1, 1, 16, 0): 124,
    (16, 2, 1, 1, 16, 1, 0, 0, 2, 1, 16, 0): 124,
    (16, 2, 1, 1, 16, 1, 1, 0, 1, 1, 16, 0): 124,
    (16, 2, 1, 1, 16, 1, 1, 0, 2, 1, 16, 0): 124,
    # 2..16 rows (FROWS), head dim 64
    (16, 2, 1, 1, 16, 1, 0, 0, 1, 0, 16, 1): 124,
    (16, 2, 1, 1, 16, 1, 0, 0, 2, 0, 16, 1): 124,
    (16, 2, 1, 1, 16, 1, 1, 0, 1, 0, 16, 1): 124,
    (16, 2, 1, 1, 16, 1, 1, 0, 2, 0, 16, 1): 124,
    # 2..16 rows (FROWS), head dim 128
    (16, 4, 1, 1, 16, 1, 0, 0, 1, 0, 16, 1): 126,
    (16, 4, 1, 1, 16, 1, 0, 0, 2, 0, 16, 1): 126,
    (16, 4, 1, 1, 16, 1, 1, 0, 1, 0, 16, 1): 128,
    (16, 4, 1, 1, 16, 1, 1, 0, 2, 0, 16, 1): 128,
}


def _remarks(unit):
    cmd = [HIPCC, *FLAGS, "--cuda-device-only", "-c", os.path.join(CSRC, unit), "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def _is_fatt(t):
    """wgemm_kernel's FATT condition (lm_gemm_kernel.h) on the template arguments."""
    waves, ku, mt_max, ng, ksplit, asrc, norm, epi, r, early, ksw, frows = t
    return (epi == 0 and asrc == 1 and waves == 16 and ksw == ksplit and mt_max == 1 and
            ((early and not frows and ku == 2) or (not early and frows)))


@pytest.fixture(scope="module")
def resources():
    with ThreadPoolExecutor(2) as ex:
        attn, store = ex.map(_remarks, ["lm_attn.hip", "lm_gemm_store.hip"])
    got_attn = {}
    for d in (64, 128):
        got_attn[f"attn_decode_kernel<{d}>"] = attn[f"_ZN3tts18attn_decode_kernelILi{d}EEEvNS_8AttnArgsE"]
    got_fatt = {}
    for name, res in store.items():
        m = re.match(r"_ZN3tts12wgemm_kernelI(.*)EEvNS_9WgemmArgsE$", name)
        if m:
            t = tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1)))
            if len(t) == 12 and _is_fatt(t):
                got_fatt[t] = res
    return got_attn, got_fatt


def test_attention_kernels_use_no_more_vgprs_than_the_parent(resources):
    got_attn, _ = resources
    for k, parent in PARENT_ATTN.items():
        r = got_attn[k]
        print(k, r, "parent", parent)
        assert r["VGPRs"] <= parent, (k, r, parent)
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (k, r)


def test_fused_qkv_attention_launches_use_no_more_vgprs_than_the_parent(resources):
    _, got_fatt = resources
    # every fused instantiation of the parent is still there, and a new one has to be recorded
    assert set(got_fatt) == set(PARENT_FATT), sorted(set(got_fatt) ^ set(PARENT_FATT))
    for t, parent in PARENT_FATT.items():
        r = got_fatt[t]
        print(t, r, "parent", parent)
        assert r["VGPRs"] <= parent, (t, r, parent)
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (t, r)
