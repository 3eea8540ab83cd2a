"""The wide decode step (65..256 rows) without a GPU: what it launches (the engine's own step code
in dry-run mode), its limits, the new op's export, and the tile lm_head's register budget.

A wide step runs its four projections on the tile GEMMs (pgemm_kernel), the row-generic decode
attention, and the lm_head as ONE tile launch with the pick's epilogue (head_tile_kernel,
lm_pgemm.hip) instead of one 32-row decode head launch per 32 rows."""

import os
import re

import pytest

from tts_amd import _lib, configs
from tts_amd.speechlm import lm_config, step_plan

WIDE = [("tts1", 65), ("tts1", 128), ("tts1", 256), ("tts1-max", 65), ("tts1-max", 128)]
TILE_HEAD = re.compile(r"head_tile_kernel<(2|4), (true|false)>$")
# wgemm_kernel<WAVES, KU, MT_MAX, NG, KSPLIT, ASRC, NORM, EPI, ...>: the lm_head epilogues are EPI 3 / 4
WGEMM_HEAD = re.compile(r"wgemm_kernel<\d+, \d+, \d+, \d+, \d+, \d+, (true|false), (3|4),")
HIPCC = "/opt/rocm/bin/hipcc"


def _tile_heads(plan):
    return [k for k in plan if TILE_HEAD.match(k)]


@pytest.mark.parametrize("arch,rows", WIDE)
def test_greedy_plan(arch, rows):
    plan = step_plan(configs.LM_ARCHS[arch], rows)
    assert _tile_heads(plan) == [f"head_tile_kernel<{2 if 129 <= rows <= 192 else 4}, false>"], plan
    assert plan.count(_tile_heads(plan)[0]) == 1
    assert not [k for k in plan if WGEMM_HEAD.match(k)], plan
    assert not [k for k in plan if k.startswith("wgemm_kernel<")], plan  # every projection on the tile GEMMs
    assert any(k.startswith("pgemm_kernel<") for k in plan), plan
    assert f"attn_decode_kernel<{configs.LM_ARCHS[arch].head_dim}>" in plan, plan
    assert not [k for k in plan if k.startswith("head_screen_kernel")], plan
    assert plan[-1] == "finalize_greedy_kernel" and plan[-2] == _tile_heads(plan)[0], plan


@pytest.mark.parametrize("arch,rows", WIDE)
def test_sampled_plan(arch, rows):
    plan = step_plan(configs.LM_ARCHS[arch], rows, top_k=50)
    assert len(_tile_heads(plan)) == 1 and _tile_heads(plan)[0].endswith("false>"), plan
    assert plan[-3:] == [_tile_heads(plan)[0], "sample_kernel", "finalize_greedy_kernel"], plan
    assert not [k for k in plan if WGEMM_HEAD.match(k) or k.startswith("head_screen_kernel")], plan


@pytest.mark.parametrize("arch,rows", WIDE)
def test_per_row_plan(arch, rows):
    plan = step_plan(configs.LM_ARCHS[arch], rows, top_k=50, per_row=True)
    assert len(_tile_heads(plan)) == 1 and _tile_heads(plan)[0].endswith("true>"), plan
    assert plan[-3:] == [_tile_heads(plan)[0], "sample_rows_kernel", "finalize_greedy_kernel"], plan
    assert not [k for k in plan if WGEMM_HEAD.match(k) or k.startswith("head_screen_kernel")], plan


def test_129_to_192_rows_take_64_row_blocks():
    """Three 64-row m-blocks pad fewer rows than two of 128."""
    assert _tile_heads(step_plan(configs.LM_ARCHS["tts1"], 130)) == ["head_tile_kernel<2, false>"]
    assert _tile_heads(step_plan(configs.LM_ARCHS["tts1"], 192)) == ["head_tile_kernel<2, false>"]
    assert _tile_heads(step_plan(configs.LM_ARCHS["tts1"], 193)) == ["head_tile_kernel<4, false>"]


@pytest.mark.parametrize("arch", ["tts1", "tts1-max"])
def test_64_row_plans_keep_the_two_chunk_decode_heads(arch):
    """The narrow regime is untouched: 64 rows run two 32-row decode GEMV launches per matrix,
    the lm_head included; no tile kernel."""
    for kw in ({}, {"top_k": 50}, {"top_k": 50, "per_row": True}):
        plan = step_plan(configs.LM_ARCHS[arch], 64, **kw)
        assert not _tile_heads(plan) and not [k for k in plan if k.startswith("pgemm_kernel<")], plan
        heads = [k for k in plan if WGEMM_HEAD.match(k)]
        assert len(heads) == 1 and f", {4 if kw.get('per_row') else 3}," in heads[0], plan
        assert heads[0].startswith("wgemm_kernel<4, 8, 2,"), plan  # (two m-tiles: a 32-row chunk)


def test_rows_beyond_256_are_invalid():
    lib = _lib.load_library()
    import ctypes

    buf = ctypes.create_string_buffer(1 << 16)
    cfg = lm_config(configs.LM_ARCHS["tts1"], max_batch=256)
    for fn, extra in ((lib.tts_debug_step_plan, ()), (lib.tts_debug_step_plan_sampled, (50,)),
                      (lib.tts_debug_step_plan_rows, (50,))):
        assert fn(ctypes.byref(cfg), 256, 256, *extra, buf, len(buf)) == _lib.TTS_OK
        assert fn(ctypes.byref(cfg), 257, 256, *extra, buf, len(buf)) == _lib.TTS_E_INVALID
        assert fn(ctypes.byref(cfg), 0, 256, *extra, buf, len(buf)) == _lib.TTS_E_INVALID
    with pytest.raises(_lib.TtsError):
        step_plan(configs.LM_ARCHS["tts1"], 257)


def test_head_pick_op_is_exported_and_the_abi_stays_4():
    lib = _lib.load_library()
    assert "tts_op_head_pick" in _lib.EXPORTED_SYMBOLS
    assert lib.tts_op_head_pick.argtypes is not None and len(lib.tts_op_head_pick.argtypes) == 21
    assert lib.tts_abi_version() == 4
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "tts_op_head_pick" in open(os.path.join(root, "include", "tts_mi355x_ops.h")).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tile_head_instantiations_do_not_spill():
    """Every head_tile_kernel<MW, per-row> compiles for gfx950 without a VGPR spill (the resource
    remarks test_kernel_resources.py parses)."""
    from test_kernel_resources import _remarks

    spills = {k: n for k, n in _remarks("lm_pgemm.hip").items() if "head_tile_kernel" in k}
    want = {f"head_tile_kernelILi{mw}ELb{r}EEE" for mw in (2, 4) for r in (0, 1)}
    assert {w for w in want if any(w in k for k in spills)} == want, sorted(spills)
    assert len(spills) == 4 and all(n == 0 for n in spills.values()), spills
