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


def test_codec_gemm_op_rejects_what_a_form_cannot_run_before_any_gpu_call():
    """tts_op_gemm_planes names one kernel instantiation; a combination that instantiation cannot
    run is an error on the host, with nothing launched (the pointers are never dereferenced)."""
    from oracle import codec_gemm_oracle as go
    from tts_amd import _lib

    lib = _lib.load_library()
    assert {"tts_op_split_planes", "tts_op_gemm_planes"} <= set(_lib.EXPORTED_SYMBOLS)
    p = 0x1000

    def gemm(form, A=p, Ap=p, B=p, Bp=p, M=70, N=68, K=64, lda=64, C=p, Cp=None, ap_plane=8192):
        return lib.tts_op_gemm_planes(A, Ap, ap_plane, M, K, lda, B, Bp, N, None, C, Cp, 8192, N, None, 0, form, None)

    x3p, bx3, f32 = go.FORMS["x3p_t1_ilv1"][0], go.FORMS["bx3_64x64"][0], go.FORMS["f32_64x64_k64"][0]
    for kw, form, word in (
            (dict(), go.x3p_form(1, 1, pp=True), b"PP needs the 8-wave"),       # PP off the 8-wave tile
            (dict(), go.x3p_form(0, 0, pp=True), b"PP needs the 8-wave"),       # PP without ILV
            (dict(), go.x3p_form(3, -1, four=True), b"four stages"),
            (dict(), go.x3p_form(5, 0), b"one-stage-ahead schedule only"),
            (dict(), 6, b"tile 0..5"),
            (dict(Ap=None), x3p, b"planes missing"),
            (dict(Bp=None), x3p, b"planes missing"),
            (dict(K=48, lda=48), x3p, b"K % 32"),
            (dict(lda=36), x3p, b"lda % 8"),
            (dict(Ap=p + 2), x3p, b"unaligned"),
            (dict(ap_plane=8196), x3p, b"ap_plane % 8"),
            (dict(K=48, lda=48), bx3, b"32-element steps"),
            (dict(B=None), bx3, b"fp32 B"),
            (dict(A=None), go.FORMS["bx3_64x64_Bp"][0], b"fp32 A"),
            (dict(Ap=None), go.FORMS["bx3_128x128_ApBp"][0], b"A's planes"),
            (dict(Bp=None), go.FORMS["bx3_256x128_Bp"][0], b"B's planes"),
            (dict(K=96, lda=96), f32, b"K step"),
            (dict(K=40, lda=40), go.FORMS["f32_128x128_k16"][0], b"K step"),
            (dict(A=None), f32, b"fp32 A and B"),
            (dict(lda=62), bx3, b"lda % 4"),
            (dict(C=None), bx3, b"no output"),
            (dict(M=0), bx3, b"bad shape"),
            (dict(), 0x300, b"unknown form"), (dict(), 0x108, b"unknown form"), (dict(), -2, b"unknown form"),
            (dict(A=None, Bp=None), -1, b"planes missing")):
        assert gemm(form, **kw) != 0, (kw, form)
        assert word in lib.tts_last_error(), (kw, form, lib.tts_last_error())
    assert lib.tts_op_split_planes(None, p, 8, None) != 0 and lib.tts_op_split_planes(p, p, 0, None) != 0


def test_struct_layouts_match_header():
    from tts_amd import _lib

    # sizes follow the C declarations (all 4-byte fields except the uint64 seed / int64 shape)
    assert ctypes.sizeof(_lib.LmConfig) == 17 * 4
    assert ctypes.sizeof(_lib.GenParams) == 8 * 4 + 8 + 2 * 4  # + frequency_penalty, reserved (ABI 2)
    assert ctypes.sizeof(_lib.CodecConfig) == (4 + 8 + 5) * 4
    assert ctypes.sizeof(_lib.TensorDesc) == 8 + 8 + 4 + 4 + 32 + 8
