"""The attention kernels alone (rope_append_kernel, attn_prefill_kernel, attn_decode_kernel of
lm_attn.hip on the core lm_attn_core.h, through tts_op_attn_prefill / tts_op_attn_decode)
against oracle/attn_oracle.py:

* the caches and q_rot to the bit (RoPE, the K rows, the V^T tiles, the K-sliced partials'
  sum), the poison around the appended positions untouched;
* census cases (q = 0, V a 0/1 code of the position): out = the count of attended positions
  with each bit / ctx, within 1 bf16 ulp — any dropped, doubled or substituted position shows;
* spike cases (one key leads by a score of 50): out = that position's v within 1e-6 + 1 ulp,
  p* swept over 0, every wave edge +- 1 (the pass edges among them), ctx - 2 and the new
  position ctx - 1;
* random cases (the real archs' RoPE tables, N(0,1) q / k / v, q scales 1 and 3) against the
  float64 reference within BAR units u = ulp_bf16(|ref|) / 2 + 2^-20 A.

tests/test_attn_reference.py shows on the CPU that these cases under these bars fail every
fault the oracle can inject, and where BAR comes from.  The fused launches inherit the result
through the bit-identity tests (test_gpu_fused_launch.py, test_gpu_switches.py).

The worst figure per family is printed and, when TTS_TEST_RECORD_DIR names a directory, written
there as attn_ops_dev.json (a copy is committed as profiles/attn_ops_dev.json).  Measured on the MI355X: census 0.499 ulp (decode)
/ 0.493 (prefill), spike 0, random 3.14 u (decode, dec_random_d64_q1) / 2.30 u (prefill) — the
figures of the CPU restatement in the kernels' exp2 form at the same cases, bar 8."""

import ctypes
import functools
import json
import os

import pytest
import torch

from oracle import attn_oracle as ao

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@functools.lru_cache(maxsize=None)
def _cases():
    return {c.name: c for c in ao.decode_cases() + ao.prefill_cases()}


@functools.lru_cache(maxsize=None)
def _ref(name):
    return ao.reference(_cases()[name])


@functools.lru_cache(maxsize=None)
def _chains():
    return dict(ao.chains())


DECODE = [c.name for c in _cases().values() if c.kind == "decode"]
PREFILL = [c.name for c in _cases().values() if c.kind == "prefill"]
CHAINS = [f"{k}_{f}_d{D}" for D in (64, 128) for f in ("census", "random")
          for k in ("prefill_continued", "prefill_then_decode")]


@pytest.fixture(scope="module")
def lib():
    from tts_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load_library()


@pytest.fixture(scope="module")
def record():
    """Worst figure per (kind, family): ulps (census, spike: beyond 1e-6) or u (random)."""
    rec = {}
    yield rec
    out = {"bars": {"census_ulps": ao.CENSUS_ULPS, "spike_abs_plus_ulps": [ao.SPIKE_ABS, 1.0], "random_u": ao.BAR},
           "worst": {k: {"figure": v[0], "case": v[1]} for k, v in sorted(rec.items())}}
    print("attention ops, worst figure per family:", json.dumps(out["worst"]))
    rec_dir = os.environ.get("TTS_TEST_RECORD_DIR")
    if rec_dir:
        os.makedirs(rec_dir, exist_ok=True)
        with open(os.path.join(rec_dir, "attn_ops_dev.json"), "w") as f:
            json.dump(out, f, indent=1)


def _i32(xs):
    return (ctypes.c_int32 * len(xs))(*xs)


def call(lib, c, Kd=None, Vd=None):
    """Runs the case's op on the device.  Kd / Vd: device caches to continue from (a chain),
    else the case's own.  Returns (status, out, K, V^T buffer, q_rot | None), device tensors."""
    qkv = None if c.part is not None else c.qkv.cuda()
    part = c.part.cuda() if c.part is not None else None
    Kd = c.K0.cuda() if Kd is None else Kd
    Vd = ao.vt_encode(c.V0).cuda() if Vd is None else Vd
    cos, sin = c.cos.cuda(), c.sin.cuda()
    out = torch.full((c.rows, c.H * c.D), float("nan"), dtype=BF16, device="cuda")
    common = (c.nslots, Kd.data_ptr(), Vd.data_ptr(), c.S, cos.data_ptr(), sin.data_ptr(), c.H, c.KVH, c.D,
              c.scale)
    if c.kind == "decode":
        slot = torch.tensor(c.row_slot, dtype=torch.int32, device="cuda")
        pos = torch.tensor(c.row_pos, dtype=torch.int32, device="cuda")
        q_rot = None
        st = lib.tts_op_attn_decode(qkv.data_ptr() if qkv is not None else None,
                                    part.data_ptr() if part is not None else None,
                                    part.shape[0] if part is not None else 0, c.ld, c.rows, slot.data_ptr(),
                                    pos.data_ptr(), *common, out.data_ptr(), None)
    else:
        q_rot = torch.full((c.rows, c.H * c.D), float("nan"), dtype=BF16, device="cuda")
        st = lib.tts_op_attn_prefill(qkv.data_ptr(), c.ld, _i32([s for s, _, _ in c.seqs]),
                                     _i32([p for _, p, _ in c.seqs]), _i32([n for _, _, n in c.seqs]),
                                     len(c.seqs), *common, q_rot.data_ptr(), out.data_ptr(), None)
    torch.cuda.synchronize()
    return st, out, Kd, Vd, q_rot


def check(lib, c, ref, record, Kd=None, Vd=None):
    from tts_amd import _lib

    st, out, Kd, Vd, q_rot = call(lib, c, Kd, Vd)
    _lib.check(st)
    fig, fails = ao.judge(c, ref, out.cpu(), Kd.cpu(), ao.vt_decode(Vd.cpu(), c.S, c.D),
                          None if q_rot is None else q_rot.cpu())
    print(f"{c.name}: {c.family} figure {fig:.3f}")
    key = f"{c.kind}_{c.family}"
    if key not in record or not fig <= record[key][0]:
        record[key] = (fig, c.name)
    assert not fails, (c.name, fails)
    return Kd, Vd


@pytest.mark.parametrize("name", DECODE)
def test_decode_step(lib, record, name):
    check(lib, _cases()[name], _ref(name), record)


@pytest.mark.parametrize("name", PREFILL)
def test_prefill(lib, record, name):
    check(lib, _cases()[name], _ref(name), record)


@pytest.mark.parametrize("name", CHAINS)
def test_call_on_top_of_an_earlier_calls_cache(lib, record, name):
    """A prefill continued from a 40-position prefix, and a decode step on a prefill-written
    cache: the second call runs on the device buffers the first one left."""
    a, b = _chains()[name]
    Kd, Vd = check(lib, a, ao.reference(a), record)
    check(lib, b, ao.reference(b), record, Kd, Vd)


def test_unsupported_arguments_are_rejected_without_a_launch(lib):
    c = _cases()["dec_random_rows3"]
    p = _cases()["pre_random_h32"]
    import dataclasses

    bad = [
        dataclasses.replace(c, D=96),
        dataclasses.replace(c, H=6),
        dataclasses.replace(c, S=c.S - 32),
        dataclasses.replace(c, row_pos=[c.row_pos[0], c.row_pos[1], c.S]),
        dataclasses.replace(c, row_slot=[c.row_slot[0], c.row_slot[1], c.nslots]),
        dataclasses.replace(c, row_slot=[c.row_slot[0], c.row_slot[0], c.row_slot[2]]),
        dataclasses.replace(p, D=32),
        dataclasses.replace(p, H=36, KVH=9),
        dataclasses.replace(p, KVH=4),
        dataclasses.replace(p, S=96),
        dataclasses.replace(p, seqs=[(p.seqs[0][0], p.S - 16, 17), p.seqs[1]]),
    ]
    for x in bad:
        st, out, Kd, Vd, q_rot = call(lib, x)
        assert st != 0, x
        assert lib.tts_last_error()
        # nothing ran: the output keeps its fill, the caches their bits
        assert bool(torch.isnan(out).all())
        assert ao.bits_equal(Kd.cpu(), x.K0) and ao.bits_equal(Vd.cpu(), ao.vt_encode(x.V0))
