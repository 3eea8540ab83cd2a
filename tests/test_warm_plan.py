"""The warm plan of the one-row fused launch (csrc/lm_kernels.h wgemm_warm_plan / warm_walk, read
through tts_debug_warm_plan): which bytes of the tiled gate/up matrix each warm workgroup reads.

The expected blocks are recomputed here in numpy from tts_debug_wgemm_plan's description of the
gate/up launch (layout units, units per round, launch shape) and the stage-major tile order of
csrc/lm_kernels.h: stage st of gate/up workgroup g of the first round (where every workgroup's
stream starts) is the tiles [(st * nr + g * UPW) * T, (st * nr + min((g + 1) * UPW, nr)) * T),
T = KSPLIT * NG * KU tiles of 1 KiB a unit, nr = the round's units.

For every shape and every warm workgroup count: every range lies inside the matrix, the ranges
are disjoint, their union is exactly stages 0 .. min(W, S) - 1 (and what 3 MiB per XCD hold) of
every gate/up workgroup, and each range's warm workgroup b and its consuming gate/up block g
satisfy g mod 8 == (b + shift) mod 8.  CPU only."""

import ctypes

import numpy as np
import pytest

# launch shapes (waves, ku, ksplit) by index: csrc/lm_gemm_kernel.h kShapes
SHAPES = {0: (4, 8, 1), 1: (8, 4, 8), 2: (16, 2, 16), 3: (16, 4, 16), 4: (8, 4, 4), 5: (8, 2, 4), 6: (16, 2, 8)}
EPI_SWIGLU, NG = 2, 2
CAP_PER_XCD = 3 << 20

# (N, K, num_cu): TTS-1's gate/up; two rounds (units 512 > ur 128 on 64 CUs); a unit count that is
# no multiple of 8 x UPW (units 90: 45 workgroups); S = 2 stages an item (S < W); an odd unit
# count (the last workgroup's block is half a block)
CASES = [(16384, 2048, 256), (16384, 2048, 64), (2880, 2048, 256), (4096, 512, 256), (2912, 1024, 256)]
WGS = (0, 8, 120, 1000)
STAGES = (0, 1, 2, 3, 5)


def _lib():
    from tts_amd import _lib

    return _lib, _lib.load_library()


def _gate_up(lib, mod, N, K, ncu):
    out = (ctypes.c_int32 * 8)()
    mod.check(lib.tts_debug_wgemm_plan(1, N, K, EPI_SWIGLU, ncu, out))
    units, ur, grid, kc, csplit, sliced, a_lds, cfg = list(out)
    waves, ku, ksplit = SHAPES[cfg]
    return dict(units=units, ur=ur, grid=grid, upw=waves // ksplit, unit_tiles=ksplit * NG * ku,
                S=(K // 32) // (ksplit * ku), csplit=csplit, sliced=sliced)


def _warm(lib, mod, N, K, ncu, W, wgs, shift):
    info = (ctypes.c_int32 * 8)()
    cap = 1 << 16
    out = np.zeros((cap, 5), dtype=np.int64)
    n = ctypes.c_int32()
    mod.check(lib.tts_debug_warm_plan(N, K, ncu, W, wgs, shift, info, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                      cap, ctypes.byref(n)))
    return list(info), out[:n.value]


@pytest.mark.parametrize("N,K,ncu", CASES)
def test_ranges_are_the_first_stages_of_every_gate_up_workgroup(N, K, ncu):
    mod, lib = _lib()
    g = _gate_up(lib, mod, N, K, ncu)
    assert g["csplit"] == 1 and not g["sliced"]
    nr = min(g["ur"], g["units"])
    nblk = -(-nr // g["upw"])
    assert nblk <= g["grid"]
    T = g["unit_tiles"] * 1024  # bytes of one unit's stage
    total = (N // 16) * (K // 32) * 1024
    blk = g["upw"] * T
    for wgs in WGS:
        for W in STAGES:
            for shift in (0, 3, -5, 328):
                info, rows = _warm(lib, mod, N, K, ncu, W, wgs, shift)
                fit = CAP_PER_XCD // (-(-nblk // 8) * blk)
                w_eff = min(W, g["S"], fit) if wgs else 0
                assert info[0] == w_eff and info[2] == nblk and info[7] == g["S"], (info, w_eff)
                assert info[1] == (wgs if w_eff else 0)
                expect = {}
                for st in range(w_eff):
                    for b in range(nblk):
                        lo = (st * nr + b * g["upw"]) * T
                        hi = (st * nr + min((b + 1) * g["upw"], nr)) * T
                        expect[(b, st)] = (lo, hi - lo)
                got = {}
                for wb, off, ln, gb, st in rows.tolist():
                    assert 0 <= wb < wgs
                    assert 0 <= off and ln > 0 and off + ln <= total, (off, ln, total)
                    assert off % 1024 == 0 and ln % 1024 == 0
                    assert (gb, st) not in got, "a block read twice"
                    got[(gb, st)] = (off, ln)
                    assert gb % 8 == (wb + shift) % 8, (wb, gb, shift)
                assert got == expect, (N, K, ncu, wgs, W, shift, len(got), len(expect))
                # disjoint as byte ranges too
                iv = sorted(got.values())
                assert all(a[0] + a[1] <= b[0] for a, b in zip(iv, iv[1:]))


def test_shapes_cover_what_they_are_meant_to():
    mod, lib = _lib()
    g = _gate_up(lib, mod, 16384, 2048, 256)  # TTS-1: 256 workgroups of two units, 8 stages of 32 KiB
    assert (g["units"], g["ur"], g["upw"], g["S"], g["upw"] * g["unit_tiles"]) == (512, 512, 2, 8, 32)
    g = _gate_up(lib, mod, 16384, 2048, 64)
    assert g["units"] > g["ur"]  # two rounds and more
    g = _gate_up(lib, mod, 2880, 2048, 256)
    assert g["units"] % (8 * g["upw"]) != 0
    g = _gate_up(lib, mod, 4096, 512, 256)
    assert g["S"] < max(STAGES)
    g = _gate_up(lib, mod, 2912, 1024, 256)
    assert g["units"] % g["upw"] == 1  # the last workgroup has one unit
    info, rows = _warm(lib, mod, 16384, 2048, 256, 2, 120, 0)
    assert info[:6] == [2, 120, 256, 32768, 32768, 8 << 20]
    assert int(rows[:, 2].sum()) == 16 << 20  # 2 MiB per XCD


def test_fewer_than_eight_warm_workgroups_are_refused():
    mod, lib = _lib()
    info = (ctypes.c_int32 * 8)()
    out = np.zeros((16, 5), dtype=np.int64)
    n = ctypes.c_int32()
    rc = lib.tts_debug_warm_plan(16384, 2048, 256, 2, 5, 0, info, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 16,
                                 ctypes.byref(n))
    assert rc != 0
