"""The one-row gate/up launch on the four-stage ring (TTS_GU_RING=4, csrc/lm_gemm_kernel.h
launch_shape) as compiled: wgemm_kernel<8, 2, 1, 2, 4, 1, true, 2, 4, true, 4, false>.

It must meet what tests/test_wgemm_prologue_isa.py asks of the two-stage instantiation — a
straight-line prologue for every lane, at most one s_waitcnt lgkmcnt and at most 110 instructions
(that file's counting rule) up to and including the first weight load — and it must hold its
four stages (64 VGPRs of ring) without scratch or spills, as tests/test_attn_core_resources.py
reads them from the compiler's resource remarks.  The two-stage instantiation stays compiled (the
default ring, and what the older test reads).  The dry-run step plan names the instantiation the
one-row step launches under either setting.  CPU only; helpers shared by import."""

import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_attn_core_resources as core  # noqa: E402
import test_wgemm_prologue_isa as isa  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(core.HIPCC), reason="hipcc not installed")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "lm_gemm_swiglu.hip"
RING4 = "8, 2, 1, 2, 4, 1, true, 2, 4, true, 4, false"
RING2 = isa.GATE_UP[1]


@pytest.fixture(scope="module")
def asm():
    return isa._functions(UNIT)


def test_ring4_prologue_is_a_straight_line_with_one_wait_before_the_first_weight_load(asm):
    assert isa._mangled(RING2) in asm  # (the two-stage ring stays compiled)
    ins = isa._instructions(asm[isa._mangled(RING4)])
    first = next(i for i, s in enumerate(ins) if s.startswith("buffer_load"))
    head = ins[:first + 1]
    waits = [s for s in head if s.startswith("s_waitcnt") and "lgkmcnt" in s]
    print(f"wgemm_kernel<{RING4}>: {len(head)} instructions up to the first buffer_load, {len(waits)} s_waitcnt lgkmcnt")
    assert not any(s.startswith("s_cbranch") and "execz" in s for s in head)
    assert len(waits) <= 1, waits
    assert len(head) <= isa.MAX_INSTRUCTIONS, len(head)
    # the four primed stages (KU 2 x NG 2 loads each) are issued before the prologue's first barrier
    body = ins[first:]
    barrier = next(i for i, s in enumerate(body) if s.startswith("s_barrier"))
    assert sum(1 for s in body[:barrier] if s.startswith("buffer_load_dwordx4")) >= 16


def test_ring4_holds_its_stages_without_spills():
    res = core._remarks(UNIT)
    r = res[isa._mangled(RING4)]
    print(RING4, r)
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, r
    assert r["VGPRs"] <= 256, r  # (8-wave workgroups: one workgroup a CU needs no more occupancy)


_PLAN_CHILD = r'''
import os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tts-max_amd"))
from tts_amd import configs
from tts_amd.speechlm import step_plan
print("\n".join(step_plan(configs.TTS1, 1, 256)))
'''


@pytest.mark.parametrize("ring,args", [("2", RING2), ("4", RING4)])
def test_step_plan_names_the_ring(ring, args):
    r = subprocess.run([sys.executable, "-c", _PLAN_CHILD, ROOT], env=dict(os.environ, TTS_GU_RING=ring),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"wgemm_kernel<{args}>" in r.stdout, r.stdout
