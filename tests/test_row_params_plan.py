"""The per-request slot batch's decode step (tts_slots_open_per_request) reads every row's
sampling settings from a device table.  Its launch list, from the engine's own step code in
dry-run mode (tts_debug_step_plan_rows), must name the per-row kernels — the screen's per-row
top-k variant + the per-row list sampler where the rows and the largest admitted top_k fit the
screen, else the full lm_head with the per-row epilogue + the per-row dense sampler — and those
instantiations must compile for gfx950 without VGPR spills.  CPU only (hipcc cross-compiles)."""

import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tts-max_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(ROOT, "tts-max_amd"))

EPI_LOGITS, EPI_LOGITS_ROWS = 3, 4
# (arch, rows, largest admitted top_k)
SCREENED = [("tts1", 1, 50), ("tts1", 8, 50), ("tts1", 16, 64), ("tts1-max", 8, 50)]
DENSE = [("tts1", 17, 50), ("tts1-max", 9, 50), ("tts1", 8, 65)]
NEW_SYMBOLS = ("tts_slots_open_per_request", "tts_slots_add_params", "tts_op_sample_rows", "tts_debug_step_plan_rows")


def _plan(arch, rows, top_k):
    from tts_amd import configs
    from tts_amd.speechlm import step_plan

    return step_plan(configs.LM_ARCHS[arch], rows, top_k=top_k, per_row=True)


def _screen_is_per_row(name):
    """head_screen_kernel<MT, KT8, RPWF, PRE, TOPK>: the per-row variant of the top-k mode carries its
    flag in the third argument (rows per wave + 8)."""
    args = [a.strip() for a in name[len("head_screen_kernel<"):-1].split(",")]
    return len(args) == 5 and int(args[2]) >= 8 and args[3:] == ["false", "true"]


def _wgemm_epi(name):
    """The EPI template argument (the 8th) of a wgemm_kernel<...> plan entry."""
    return int(name[len("wgemm_kernel<"):-1].split(",")[7])


def test_new_symbols_are_exported():
    from tts_amd import _lib

    lib = _lib.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTED_SYMBOLS, s
    assert lib.tts_abi_version() == 4


@pytest.mark.parametrize("arch,rows,top_k", SCREENED)
def test_per_row_plan_takes_the_screen(arch, rows, top_k):
    plan = _plan(arch, rows, top_k)
    screen = [k for k in plan if k.startswith("head_screen_kernel<")]
    assert len(screen) == 1 and _screen_is_per_row(screen[0]), plan
    assert "sample_list_rows_kernel" in plan, plan
    assert "sample_list_kernel" not in plan and "sample_kernel" not in plan and "sample_rows_kernel" not in plan, plan
    epis = [_wgemm_epi(k) for k in plan if k.startswith("wgemm_kernel<")]
    assert EPI_LOGITS not in epis and EPI_LOGITS_ROWS not in epis, plan
    assert plan[-1] == "finalize_greedy_kernel", plan


def test_screen_row_variants():
    """1, 8 and 16 rows at hidden 2048 and 3 / 8 rows at 4096 are different instantiations."""
    assert "head_screen_kernel<1, 32, 9, false, true>" in _plan("tts1", 1, 1)
    assert "head_screen_kernel<1, 32, 10, false, true>" in _plan("tts1", 8, 1)
    assert "head_screen_kernel<2, 32, 12, false, true>" in _plan("tts1", 16, 1)
    assert "head_screen_kernel<1, 64, 9, false, true>" in _plan("tts1-max", 3, 1)
    assert "head_screen_kernel<1, 64, 10, false, true>" in _plan("tts1-max", 8, 1)


@pytest.mark.parametrize("arch,rows,top_k", DENSE)
def test_per_row_plan_takes_the_full_head(arch, rows, top_k):
    plan = _plan(arch, rows, top_k)
    assert not [k for k in plan if k.startswith("head_screen_") or k == "head_rowquant_kernel"], plan
    epis = [_wgemm_epi(k) for k in plan if k.startswith("wgemm_kernel<")]
    assert epis.count(EPI_LOGITS_ROWS) == 1 and EPI_LOGITS not in epis, plan
    assert "sample_rows_kernel" in plan and "sample_kernel" not in plan, plan
    assert "sample_list_rows_kernel" not in plan and "sample_list_kernel" not in plan, plan
    assert plan[-1] == "finalize_greedy_kernel", plan


def test_uniform_plans_do_not_name_the_per_row_kernels():
    from tts_amd import configs
    from tts_amd.speechlm import step_plan

    for top_k in (None, 50):
        for rows in (1, 8, 17):
            plan = step_plan(configs.LM_ARCHS["tts1"], rows, top_k=top_k)
            assert not [k for k in plan if "rows_kernel" in k], plan
            assert not [k for k in plan if k.startswith("head_screen_kernel<") and _screen_is_per_row(k)], plan
            assert EPI_LOGITS_ROWS not in [_wgemm_epi(k) for k in plan if k.startswith("wgemm_kernel<")], plan


def _remarks(unit):
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics", "--cuda-device-only", "-c",
           os.path.join(CSRC, unit), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"remark:\s+VGPRs Spill: (\d+)", line)
        if m and name:
            out[name] = int(m.group(1))
    return out


def _mangled(args):
    """Itanium mangling of tts::wgemm_kernel<...>(tts::WgemmArgs) for the template arguments."""
    parts = []
    for a in (x.strip() for x in args.split(",")):
        parts.append({"false": "Lb0E", "true": "Lb1E"}.get(a, f"Li{a}E"))
    return "_ZN3tts12wgemm_kernelI" + "".join(parts) + "EEvNS_9WgemmArgsE"


@pytest.fixture(scope="module")
def spills():
    units = ["lm_gemm_logits.hip", "lm_sample.hip", "lm_head_screen.hip"]
    with ThreadPoolExecutor(len(units)) as ex:
        return dict(zip(units, ex.map(_remarks, units)))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_per_row_instantiations_do_not_spill(spills):
    hot = {}
    for arch, rows, top_k in DENSE + [("tts1", 32, 50), ("tts1", 1, 65)]:
        for k in _plan(arch, rows, top_k):
            if k.startswith("wgemm_kernel<") and _wgemm_epi(k) == EPI_LOGITS_ROWS:
                hot[k[len("wgemm_kernel<"):-1]] = f"{arch} {rows} rows"
    assert len(hot) >= 3, hot
    logits = spills["lm_gemm_logits.hip"]
    missing = [h for h in hot if _mangled(h) not in logits]
    assert not missing, f"per-row lm_head instantiations not compiled: {missing}"
    bad = {h: logits[_mangled(h)] for h in hot if logits[_mangled(h)] > 0}
    assert not bad, f"VGPR spills in the per-row lm_head: {bad}"
    # the samplers (uniform and per-row, dense and list) and every screen variant
    sample = spills["lm_sample.hip"]
    for k in ("sample_kernel", "sample_list_kernel", "sample_rows_kernel", "sample_list_rows_kernel"):
        assert [n for n in sample if k in n], (k, sorted(sample))
    bad = {k: n for unit in ("lm_sample.hip", "lm_head_screen.hip") for k, n in spills[unit].items() if n > 0}
    assert not bad, f"VGPR spills: {bad}"
    rows_screens = [n for n in spills["lm_head_screen.hip"] if re.search(r"head_screen_kernelILi\dELi\d+ELi(9|10|12)ELb0ELb1EE", n)]
    assert len(rows_screens) == 5, sorted(spills["lm_head_screen.hip"])
