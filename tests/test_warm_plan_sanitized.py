"""The warm plan (csrc/lm_kernels.h wgemm_warm_plan / warm_walk) walked by a stand-alone host
program under the address and undefined-behaviour sanitizers.

Builds tests/warm_plan_check.cpp — its own main, around lm_kernels.h and the library's
plan_wgemm — in the manner of tests/test_fastdiv.py, and feeds it the shapes of
tests/test_warm_plan.py with every stage count, warm workgroup count and shift: the program marks
what each warm workgroup reads in a map exactly as long as the tiled matrix.  CPU only."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tts-max_amd")
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "tts_amd")
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"

# (the library is the project's own build: without it the link step below fails, loudly)
pytestmark = pytest.mark.skipif(not (os.path.exists(CXX) and os.path.isdir("/opt/rocm/include")),
                                reason="needs a host compiler and the HIP headers")

CASES = [(16384, 2048, 256), (16384, 2048, 64), (2880, 2048, 256), (4096, 512, 256), (2912, 1024, 256),
         (28672, 4096, 256)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("warm") / "warm_plan_check")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           os.path.join(ROOT, "tests", "warm_plan_check.cpp"), "-o", exe,
           "-L" + LIBDIR, "-ltts_mi355x", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_every_warm_workgroup_reads_inside_the_matrix_and_the_union_is_the_first_stages(program):
    lines = []
    for N, K, ncu in CASES:
        for W in (0, 1, 2, 3, 5, 100):
            for wgs in (0, 5, 8, 9, 120, 1000):
                for shift in (0, 3, -5, 328):
                    lines.append(f"{N} {K} {ncu} {W} {wgs} {shift}")
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "OK" and int(last[1]) == len(lines), last
    assert int(last[2]) > 10_000, last  # (blocks walked: the sweeps ran)
    assert "refused" in r.stdout  # (1..7 warm workgroups: a class of blocks would have none)
