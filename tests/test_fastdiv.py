"""Division by launch constants in the decode GEMM (csrc/fastdiv.h): the multiply-high pairs are
exact for every dividend the kernel can form, and the host refuses a pair that is not.

Builds tests/fastdiv_check.cpp — a stand-alone host program with its own main, around
fastdiv.h and the library's plan_wgemm / wgemm_derive — with the address and undefined-behaviour
sanitizers, and runs it on the projection launches of TTS-1, TTS-1-Max and the tiny / small
golden architectures at every row count where the plan changes, 1..64 (a wide step of 65..256
rows runs its layer GEMMs on the prefill tile kernel, which has no such division; its row chunks of
up to 64 are the same launches as here).  For each launch and each divisor (ur, kch, Sc, and KVH /
the riding o_proj's Sc of the fused QKV launch) the program compares fastdiv(n) with n / d for every
n from 0 to the bound the pair was made for.  CPU only."""

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tts-max_amd")
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "tts_amd")
LIB = os.path.join(LIBDIR, "libtts_mi355x.so")
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"

# (the library is the project's own build: without it the link step below fails, loudly)
pytestmark = pytest.mark.skipif(not (os.path.exists(CXX) and os.path.isdir("/opt/rocm/include")),
                                reason="needs a host compiler and the HIP headers")

EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_LOGITS = 0, 1, 2, 3
ROWS = (1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 24, 32, 33, 48, 64)


def _launches():
    sys.path.insert(0, PKG)
    from tts_amd import configs

    out = []
    for name in ("tts1", "tts1-max", "tiny", "small", "tiny128"):
        c = configs.LM_ARCHS[name]
        hid, hd, ff = c.hidden_size, c.num_heads * c.head_dim, c.intermediate_size
        qkv = hd + 2 * c.num_kv_heads * c.head_dim
        for m in ROWS:
            out.append((m, qkv, hid, EPI_STORE, 0, 0, 0, 0, 0))
            out.append((m, hid, hd, EPI_RESID, 0, 0, 0, 0, 0))
            out.append((m, 2 * ff, hid, EPI_SWIGLU, 0, 0, 0, 0, 0))
            out.append((m, hid, ff, EPI_RESID, 0, 0, 0, 0, 0))
            out.append((m, c.vocab_size, hid, EPI_LOGITS, 0, 0, 0, 0, 0))
            if m <= 16 and hid % 512 == 0:  # the QKV launch carrying the attention (and o_proj)
                out.append((m, qkv, hid, EPI_STORE, c.num_kv_heads, c.num_heads, c.head_dim, 0, 0))
                out.append((m, qkv, hid, EPI_STORE, c.num_kv_heads, c.num_heads, c.head_dim, hid, hd))
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fastdiv") / "fastdiv_check")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           os.path.join(ROOT, "tests", "fastdiv_check.cpp"), "-o", exe,
           "-L" + LIBDIR, "-ltts_mi355x", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_pairs_exact_on_every_dividend_and_inexact_pairs_refused(program):
    cases = _launches()
    text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "OK", last
    # every plain launch was planned and swept (fused ones are skipped where the plan cannot carry them)
    assert int(last[1]) >= sum(1 for c in cases if c[4] == 0), last
    assert int(last[2]) > 1_000_000, last  # (divisions compared: the sweeps ran, not an empty loop)
    out = r.stdout
    assert "kch 1792" in out  # TTS-1-Max down: not a power of two
    assert "refused: pair" in out
