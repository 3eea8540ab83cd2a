"""The decode GEMM keeps its bits across the new argument layout and the host-side index
arithmetic (csrc/lm_kernels.h WgemmArgs, csrc/fastdiv.h): the md5 of tts_op_wgemm's outputs
(and of tts_op_head_pick's, form 1: the same kernel with the lm_head epilogue) against
tests/golden/wgemm_prologue_bits.json.

The golden file was recorded from a build of the commit before that change (e123977), on an
MI355X:  TTS_LIB_PATH=<that build's libtts_mi355x.so> python tests/test_gpu_wgemm_prologue_bits.py
prints it.  Nothing that computes a value changed, so every bit stays; that the bits are RIGHT is
the op tests' job (tests/test_gpu_ops.py).

The shapes are the smallest that reach each index path, not the workload's:
  K 1536 and 3584 (16-byte chunks per row 192 and 448: not powers of two) beside K 2048;
  (N 4800 at K 1536: 300 units in one round of 300, on the 4-wave plan K / 32 = 48 falls back to);
  N 4816 at K 2048 (store) and N 16448 at K 2048 (lm_head): 301 / 1,028 units in rounds of 151 /
  516, i.e. a partial last round (test_shapes_reach_their_index_paths asserts it from the plan);
  N 2048 at K 2048: 128 units, run as 8-column halves (csplit 2) up to 16 rows;
  K 8192 (four K chunks, kc > 1; K-sliced from 8 rows on) with the residual epilogue;
  rows 1, 3, 4 (register-staged prologue across rows), 5 and 16 (LDS-DMA prologue), 17 and 32
  (two m-tiles); store, residual, SwiGLU and lm_head epilogues; with and without the RMSNorm."""

import ctypes
import hashlib
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wgemm_prologue_bits.json")
ROWS = (1, 3, 4, 5, 16, 17, 32)
EPI = {"store": 0, "resid": 1, "swiglu": 2}

# (epilogue, N, K, norm)
SHAPES = [
    ("store", 4800, 1536, False),
    ("store", 4800, 1536, True),
    ("store", 1024, 3584, False),
    ("store", 1024, 3584, True),
    ("store", 2048, 2048, False),
    ("store", 2048, 2048, True),
    ("resid", 2048, 2048, False),
    ("resid", 2048, 8192, False),
    ("swiglu", 1024, 2048, False),
    ("swiglu", 1024, 2048, True),
    ("logits", 16384, 2048, False),
    ("logits", 16384, 2048, True),
    ("store", 4816, 2048, False),
    ("store", 4816, 2048, True),
    ("logits", 16448, 2048, False),
]
PARTIAL_ROUND = [("store", 4816, 2048), ("logits", 16448, 2048)]  # units > ur, units % ur != 0


def shape_key(epi, N, K, norm):
    return f"{epi}_N{N}_K{K}_{'norm' if norm else 'plain'}"


def _md5(*tensors):
    import torch

    h = hashlib.md5()
    for t in tensors:
        h.update(t.cpu().contiguous().view(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_shape(lib, epi, N, K, norm):
    """{rows: md5 of the outputs} of one shape, every row count a prefix of the same rows."""
    import torch

    from tts_amd import _lib

    g = torch.Generator().manual_seed(N * 31 + K)
    w = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).cuda()
    x = (torch.randn(max(ROWS), K, generator=g) * 0.5).to(torch.bfloat16).cuda()
    nw = (1 + 0.2 * torch.randn(K, generator=g)).to(torch.bfloat16).cuda()
    r0 = (torch.randn(max(ROWS), N, generator=g) * 0.5).to(torch.bfloat16).cuda()
    wt = torch.empty_like(w)
    _lib.check(lib.tts_op_retile(w.data_ptr(), wt.data_ptr(), N, K, EPI.get(epi, 0), None))
    nwp = nw.data_ptr() if norm else None
    out = {}
    for M in ROWS:
        xm = x[:M].contiguous()
        if epi == "logits":
            words = N // 32
            seen = (torch.arange(M * words, dtype=torch.int64).reshape(M, words) * 2654435761 % (1 << 31)).to(torch.int32).cuda()
            eos = torch.full((M,), 7, dtype=torch.int32, device="cuda")
            pv = torch.zeros(M, 1024, device="cuda")
            pi = torch.zeros(M, 1024, dtype=torch.int32, device="cuda")
            lg = torch.zeros(M, N, device="cuda")
            n = ctypes.c_int32(0)
            _lib.check(lib.tts_op_head_pick(xm.data_ptr(), M, K, nwp, 1e-5, wt.data_ptr(), N, seen.data_ptr(), words, 1.3,
                                            None, 0.0, eos.data_ptr(), None, None, pv.data_ptr(), pi.data_ptr(),
                                            ctypes.byref(n), lg.data_ptr(), 1, None))
            torch.cuda.synchronize()
            out[str(M)] = _md5(lg, pv[:, :n.value], pi[:, :n.value])
            continue
        nout = N // 2 if epi == "swiglu" else N
        o = torch.zeros(M, nout, dtype=torch.bfloat16, device="cuda")
        res = r0[:M].clone() if epi == "resid" else None
        _lib.check(lib.tts_op_wgemm(xm.data_ptr(), M, K, K, wt.data_ptr(), N, nwp, 1e-5,
                                    o.data_ptr() if res is None else None, nout,
                                    res.data_ptr() if res is not None else None, EPI[epi], None))
        torch.cuda.synchronize()
        out[str(M)] = _md5(res if res is not None else o)
    return out


@pytest.fixture(scope="module")
def lib():
    import torch

    from tts_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load_library()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["md5"]


def _plan(lib, M, N, K, epi):
    """tts_debug_wgemm_plan on this GPU's CU count -> dict"""
    import torch

    from tts_amd import _lib

    out = (ctypes.c_int32 * 8)()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    _lib.check(lib.tts_debug_wgemm_plan(M, N, K, {"store": 0, "resid": 1, "swiglu": 2, "logits": 3}[epi], ncu, out))
    return dict(zip(("units", "ur", "grid", "kc", "csplit", "sliced", "a_lds", "cfg"), out))


def test_shapes_reach_their_index_paths(lib):
    """What the docstring says of the shapes, from the library's own plan on this GPU."""
    for epi, N, K in PARTIAL_ROUND:  # more than one layout round, the last one partial
        for M in ROWS:
            p = _plan(lib, M, N, K, epi)
            print(epi, N, K, M, p)
            assert p["units"] > p["ur"] and p["units"] % p["ur"] != 0, (epi, N, K, M, p)
    for M in (1, 3, 4, 5, 16):  # 8-column halves up to 16 rows
        assert _plan(lib, M, 2048, 2048, "store")["csplit"] == 2
        assert _plan(lib, M, 2048, 2048, "resid")["csplit"] == 2
    for M in ROWS:  # K chunks; K-sliced from 8 rows on
        p = _plan(lib, M, 2048, 8192, "resid")
        assert p["kc"] > 1 and (p["sliced"] == 1) == (M >= 8), (M, p)


@pytest.mark.parametrize("epi,N,K,norm", SHAPES, ids=[shape_key(*s) for s in SHAPES])
def test_wgemm_bits_unchanged(lib, golden, epi, N, K, norm):
    got = run_shape(lib, epi, N, K, norm)
    want = golden[shape_key(epi, N, K, norm)]
    assert set(got) == set(want)
    diff = {m: (got[m], want[m]) for m in got if got[m] != want[m]}
    assert not diff, diff


if __name__ == "__main__":  # record: run with TTS_LIB_PATH = the library built from the parent commit
    sys.path.insert(0, os.path.join(ROOT, "tts-max_amd"))
    from tts_amd import _lib as _l

    _lb = _l.load_library()
    print(json.dumps({"recorded_from": "build of commit e123977 (the parent of the argument-layout change), MI355X",
                      "how": "TTS_LIB_PATH=<parent libtts_mi355x.so> python tests/test_gpu_wgemm_prologue_bits.py",
                      "md5": {shape_key(*s): run_shape(_lb, *s) for s in SHAPES}}, indent=1))
