"""The decode GEMM's prologue as compiled: one argument fetch before the loads, no integer
division (csrc/lm_kernels.h WgemmArgs, csrc/fastdiv.h).

Compiles lm_gemm_{swiglu,resid,store}.hip for gfx950 with the Makefile's flags and -S, in the
manner of the resource tests, and reads the assembly of wgemm_kernel's instantiations:

* none contains v_rcp_iflag (the compiler's expansion of an integer division, ~35
  instructions with v_readfirstlane + s_nop each);
* the one-row gate/up and down instantiations of the flagship step, whose prologues are a
  straight line, reach their first weight load (the first buffer_load) behind at most one
  s_waitcnt lgkmcnt and at most 110 instructions: half of the 219 / 203 of the commit before this
  layout (e123977), counted with the same rule;
* the one-row fused QKV + attention + o_proj instantiation fetches WgemmArgs::x and ::w in the
  first batch of the function (every s_load before the first s_waitcnt), i.e. ahead of the role
  branch.

COUNTING RULE: from the function's label up to and including its first buffer_load, every line
that is not blank, not a comment (first non-blank character ';') and not a directive or local
label (first non-blank character '.') is one instruction.  That rule gives 219 (gate/up) and 203
(down) on a build of e123977.  CPU only (hipcc cross-compiles)."""

import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tts-max_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
UNITS = ["lm_gemm_swiglu.hip", "lm_gemm_resid.hip", "lm_gemm_store.hip"]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# wgemm_kernel<WAVES, KU, MT_MAX, NG, KSPLIT, ASRC, NORM, EPI, R, EARLY, KSW, FROWS> of the one-row
# TTS-1 step (tests/test_kernel_resources.py reads the same names from the step's dry run)
GATE_UP = ("lm_gemm_swiglu.hip", "8, 2, 1, 2, 4, 1, true, 2, 2, true, 4, false")
DOWN = ("lm_gemm_resid.hip", "16, 4, 1, 1, 16, 1, false, 1, 2, true, 16, false")
FUSED = ("lm_gemm_store.hip", "16, 2, 1, 1, 16, 1, true, 0, 2, true, 16, false")
MAX_INSTRUCTIONS = 110
# byte offsets of WgemmArgs::x and ::w in the kernel-argument segment (static_asserts in lm_kernels.h)
OFF_X, OFF_W = 0x0, 0x8


def _mangled(args):
    parts = [{"false": "Lb0E", "true": "Lb1E"}.get(a.strip(), f"Li{a.strip()}E") for a in args.split(",")]
    return "_ZN3tts12wgemm_kernelI" + "".join(parts) + "EEvNS_9WgemmArgsE"


def _functions(unit):
    """{mangled name: body lines} of every wgemm_kernel instantiation in the unit's assembly."""
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics",
           "--cuda-device-only", "-S", os.path.join(CSRC, unit), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stdout.splitlines():
        m = re.match(r"(_ZN3tts12wgemm_kernelI\w+):", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                name = None
            else:
                out[name].append(line)
    return out


@pytest.fixture(scope="module")
def asm():
    with ThreadPoolExecutor(len(UNITS)) as ex:
        return dict(zip(UNITS, ex.map(_functions, UNITS)))


def _instructions(body):
    return [s for s in (line.strip() for line in body) if s and s[0] not in ";."]


def test_no_integer_division_in_any_instantiation(asm):
    n = 0
    for unit, fns in asm.items():
        assert fns, unit
        for name, body in fns.items():
            n += 1
            assert not any("v_rcp_iflag" in line for line in body), (unit, name)
    print("wgemm_kernel instantiations read:", n)
    assert n >= 100, n  # (the three units hold well over a hundred)


@pytest.mark.parametrize("unit,args", [GATE_UP, DOWN], ids=["gate_up", "down"])
def test_straight_line_prologue_one_wait_before_the_first_weight_load(asm, unit, args):
    ins = _instructions(asm[unit][_mangled(args)])
    first = next(i for i, s in enumerate(ins) if s.startswith("buffer_load"))
    head = ins[:first + 1]  # (the first buffer_load included)
    waits = [s for s in head if s.startswith("s_waitcnt") and "lgkmcnt" in s]
    print(f"wgemm_kernel<{args}>: {len(head)} instructions up to the first buffer_load, {len(waits)} s_waitcnt "
          f"lgkmcnt among them (parent: 219 gate/up, 203 down; 2 waits)")
    assert not any(s.startswith("s_cbranch") and "execz" in s for s in head)  # (a straight line for every lane)
    assert len(waits) <= 1, waits
    assert len(head) <= MAX_INSTRUCTIONS, len(head)


def test_fused_launch_fetches_x_and_w_in_its_first_batch(asm):
    unit, args = FUSED
    ins = _instructions(asm[unit][_mangled(args)])
    first_wait = next(i for i, s in enumerate(ins) if s.startswith("s_waitcnt"))
    covered = set()
    for s in ins[:first_wait]:
        m = re.match(r"s_load_dword(x(\d+))?\s+\S+\s+s\[0:1\],\s+(0x[0-9a-f]+|\d+)", s)
        if m:
            off, n = int(m.group(3), 0), int(m.group(2) or 1)
            covered.update(range(off, off + 4 * n))
    print(f"wgemm_kernel<{args}>: first batch covers {len(covered)} argument bytes, "
          f"{first_wait} instructions before its wait")
    for off in (OFF_X, OFF_W):
        assert set(range(off, off + 8)) <= covered, (hex(off), sorted(covered)[:4])
    # and the role branch comes behind that wait
    assert not any(s.startswith("s_cbranch") for s in ins[:first_wait])
