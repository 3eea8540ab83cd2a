"""The C-ABI library loads and exports every symbol include/*.h declares (no compute)."""

import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    names = set()
    for h in ("tts_mi355x.h", "tts_mi355x_ops.h"):
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names |= set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", src))
    return names


def test_library_exports_every_declared_symbol():
    from tts_amd import _lib

    lib = _lib.load_library()
    declared = _declared()
    assert declared, "no declarations parsed"
    missing = [n for n in sorted(declared) if not hasattr(lib, n)]
    assert not missing, missing
    assert set(_lib.EXPORTED_SYMBOLS) == declared


def test_abi_version_and_error_path():
    from tts_amd import _lib

    lib = _lib.load_library()
    assert lib.tts_abi_version() == 4
    # invalid argument path: no GPU work, error message set, status non-zero
    st = lib.tts_engine_create(0, None)
    assert st != 0
    assert b"null" in lib.tts_last_error()


def test_attention_ops_reject_unsupported_shapes_before_any_gpu_call():
    """tts_op_attn_prefill / tts_op_attn_decode check the geometry on the host first: head dim
    64 or 128, H = 4 KVH, at most 8 kv heads (prefill), max_seq a multiple of 64, ld_qkv wide
    enough.  (The pointers are never dereferenced; the position checks need the device arrays:
    tests/test_gpu_attn_ops.py.)"""
    from tts_amd import _lib

    lib = _lib.load_library()
    p = 0x1000
    one = (ctypes.c_int32 * 1)(0)
    length = (ctypes.c_int32 * 1)(3)

    def prefill(ld, max_seq, H, KVH, D):
        return lib.tts_op_attn_prefill(p, ld, one, one, length, 1, 1, p, p, max_seq, p, p, H, KVH, D, 0.125, p, p, None)

    def decode(ld, max_seq, H, KVH, D):
        return lib.tts_op_attn_decode(p, None, 0, ld, 1, p, p, 1, p, p, max_seq, p, p, H, KVH, D, 0.125, p, None)

    for fn in (prefill, decode):
        for args, word in (((768, 64, 8, 2, 96), b"head dim"), ((768, 64, 6, 2, 64), b"num_heads"),
                           ((768, 100, 8, 2, 64), b"max_seq"), ((760, 64, 8, 2, 64), b"ld_qkv")):
            assert fn(*args) != 0, args
            assert word in lib.tts_last_error(), (args, lib.tts_last_error())
    assert prefill(54 * 64, 64, 36, 9, 64) != 0
    assert b"8 kv heads" in lib.tts_last_error()
    assert lib.tts_op_attn_decode(p, p, 4, 768, 1, p, p, 1, p, p, 64, p, p, 8, 2, 64, 0.125, p, None) != 0
    assert b"exactly one" in lib.tts_last_error()


def test_struct_layouts_match_header():
    from tts_amd import _lib

    # sizes follow the C declarations (all 4-byte fields except the uint64 seed / int64 shape)
    assert ctypes.sizeof(_lib.LmConfig) == 17 * 4
    assert ctypes.sizeof(_lib.GenParams) == 8 * 4 + 8 + 2 * 4  # + frequency_penalty, reserved (ABI 2)
    assert ctypes.sizeof(_lib.CodecConfig) == (4 + 8 + 5) * 4
    assert ctypes.sizeof(_lib.TensorDesc) == 8 + 8 + 4 + 4 + 32 + 8
