"""Every codec GEMM kernel form alone (tts_op_gemm_planes) against the float64 reference of
oracle/codec_gemm_oracle.py, at its own tile's edges: one test per form, so a failure names it.

Per form and shape (oracle.shapes: single element, ragged tiles, scalar and vector epilogue,
1 / 2 / 3 / 5 / 64 K steps, eight tiles, the lda < K conv window), per epilogue configuration
(act 0 / 1, bias, resid) and output (C, Cp, both), each launch is judged by the oracle's `judge`
(bit equality of the exact cases; the two bars of the random cases; Cp == split(stored C)), the
guard patterns around C / Cp must survive, the operands end in NaN guard rows, and every
bf16-split form must give the bits of the anchor form (bx3 64x64 from fp32 operands) on the same
inputs.  tests/test_codec_gemm_reference.py proves on the CPU that this judge fails every mutant.

Measured on an MI355X (profiles/codec_gemm_parity.txt): all 21 bf16-split forms give the same
bits; their rms(e) is 0.76 .. 0.86 x the CPU fp32 matmul's up to K = 160 and 2.63 x at K = 2048,
the fp32 MFMA forms' 1.00 .. 1.42 x up to K = 320 and 3.13 x at K = 2048 (the bar is 4); the largest
e is 0.09 / 0.21 of the hard bound.  A form runs its 420 launches in about 0.2 s."""

import os

import numpy as np
import pytest
import torch

from oracle import codec_gemm_oracle as go

pytestmark = pytest.mark.gpu

# forms of one tile next to each other: the oracle keeps the last two tiles' problems
ORDER = sorted(go.FORMS, key=lambda n: (go.kstep_of(n), go.FORMS[n][1], go.FORMS[n][2], n))


@pytest.fixture(scope="module")
def lib():
    from tts_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load_library()


def _check(st):
    from tts_amd import _lib

    _lib.check(st)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Operands:
    """A problem's operands on the device, each followed by NaN guard rows."""

    def __init__(self, p):
        nan_f = np.full(2 * max(p.lda, p.K), np.nan, np.float32)
        a = np.concatenate([p.abuf, nan_f])
        self.ap_plane = (a.size + 7) // 8 * 8
        ap = np.full((3, self.ap_plane), go.GUARD_BF16, np.uint16)
        ap[:, :p.abuf.size] = go.planes_bits(p.abuf)
        self.A, self.Ap = _dev(a), _dev(ap.view(np.int16))
        self.B = _dev(np.concatenate([p.B.reshape(-1), np.full(2 * p.K, np.nan, np.float32)]))
        bp = np.concatenate([go.planes_bits(p.B).reshape(-1), np.full(2 * p.K, go.GUARD_BF16, np.uint16)])
        self.Bp = _dev(bp.view(np.int16))
        self.bias, self.resid = _dev(p.bias), _dev(p.resid)
        self.rows = p.M + 2                                  # C / Cp with two guard rows
        self.cp_plane = self.rows * p.ldc
        self.C = torch.empty(self.cp_plane, dtype=torch.int32, device="cuda")
        self.Cp = torch.empty(3 * self.cp_plane, dtype=torch.int16, device="cuda")


_ops: dict = {}
_anchor: dict = {}


def _operands(p):
    if p.name not in _ops:
        if len(_ops) > 64:
            _ops.clear()
        _ops[p.name] = _Operands(p)
    return _ops[p.name]


def _launch(lib, c, form, a_kind, b_kind, out):
    """One launch into freshly poisoned outputs -> (C [M, N] or None, Cp [3, M, N] or None)."""
    p, o = c.p, _operands(c.p)
    o.C.fill_(go.GUARD_F32)
    o.Cp.fill_(-1)
    want_c, want_p = out in ("C", "both"), out in ("Cp", "both")
    _check(lib.tts_op_gemm_planes(
        _ptr(o.A) if a_kind == "A" else None, _ptr(o.Ap) if a_kind == "Ap" else None, o.ap_plane, p.M, p.K, p.lda,
        _ptr(o.B) if b_kind == "B" else None, _ptr(o.Bp) if b_kind == "Bp" else None, p.N,
        _ptr(o.bias) if c.bias else None, _ptr(o.C) if want_c else None, _ptr(o.Cp) if want_p else None,
        o.cp_plane, p.ldc, _ptr(o.resid) if c.resid else None, c.act, form, None))
    torch.cuda.synchronize()
    Cb = o.C.cpu().numpy().view(np.uint32).reshape(o.rows, p.ldc)
    Pb = o.Cp.cpu().numpy().view(np.uint16).reshape(3, o.rows, p.ldc)
    # guards: rows >= M and columns [N, ldc) keep their patterns, and an output not asked for
    # is not written at all
    assert (Cb[p.M:] == go.GUARD_F32).all() and (Cb[:, p.N:] == go.GUARD_F32).all(), (c.name, out, "C guard")
    assert (Pb[:, p.M:] == go.GUARD_BF16).all() and (Pb[:, :, p.N:] == go.GUARD_BF16).all(), (c.name, out, "Cp guard")
    if not want_c:
        assert (Cb == go.GUARD_F32).all(), (c.name, out, "C written")
    if not want_p:
        assert (Pb == go.GUARD_BF16).all(), (c.name, out, "Cp written")
    C = np.ascontiguousarray(Cb[:p.M, :p.N]).view(np.float32) if want_c else None
    Cp = np.ascontiguousarray(Pb[:, :p.M, :p.N]) if want_p else None
    return C, Cp


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("name", ORDER)
def test_form_against_fp64(lib, name):
    form, TM, TN, kernel, a_kind, b_kind = go.FORMS[name]
    ks = go.kstep_of(name)
    aform = go.FORMS[go.ANCHOR][0]
    worst = {"rms_ratio": 0.0, "max_e_over_bound": 0.0}
    by_k: dict = {}
    fails = []
    launches = 0
    for p in go.problems(TM, TN, ks):
        for c in go.cases_of(p):
            got = {}
            for out in ("C", "Cp", "both"):
                C, Cp = _launch(lib, c, form, a_kind, b_kind, out)
                launches += 1
                fig, f = go.judge(c, C if C is not None else got["C"][0], Cp)
                fails += [f"{c.name} [{out}]: {m}" for m in f]
                for k in worst:
                    worst[k] = max(worst[k], fig.get(k, 0.0))
                if "rms_ratio" in fig:
                    by_k[p.K] = max(by_k.get(p.K, 0.0), fig["rms_ratio"])
                got[out] = (C, Cp)
            # one value whatever the outputs asked for
            if not (np.array_equal(_bits(got["C"][0]), _bits(got["both"][0])) and np.array_equal(got["Cp"][1], got["both"][1])):
                fails.append(f"{c.name}: C / Cp differ between the C, Cp and both launches")
            if kernel != "f32":   # the same bits from every bf16-split form
                key = (c.name, TM, TN)
                if key not in _anchor:
                    if len(_anchor) > 400:
                        _anchor.clear()
                    _anchor[key] = got["C"][0] if name == go.ANCHOR else _launch(lib, c, aform, "A", "B", "C")[0]
                if not np.array_equal(_bits(got["C"][0]), _bits(_anchor[key])):
                    n = int((_bits(got["C"][0]) != _bits(_anchor[key])).sum())
                    fails.append(f"{c.name}: {n} elements differ from {go.ANCHOR}'s bits")
    print(f"PARITY {name}: rms ratio to CPU fp32 {worst['rms_ratio']:.3f}, largest e / ((K+4) 2^-24) "
          f"{worst['max_e_over_bound']:.4f}, {launches} launches; rms ratio by K "
          + ", ".join(f"{k}: {v:.2f}" for k, v in sorted(by_k.items())))
    assert not fails, fails[:12]
    assert worst["rms_ratio"] > 0 and worst["max_e_over_bound"] > 0   # (the random cases were judged)


def test_split_planes_kernel(lib):
    """split_planes_kernel == the host split, bit for bit: magnitudes 2^-20 .. 2^20, both signs,
    +-0, bf16 ties, more elements than one pass of the grid, and a guard behind the planes."""
    n = 8192 * 256 + 77
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(n) * np.exp2(rng.uniform(-20, 20, n))).astype(np.float32)
    x[:6] = [0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(2.0 ** 20), 2.0 ** -20]
    assert (x < 0).mean() > 0.4 and np.abs(x[x != 0]).min() < 2.0 ** -19 and np.abs(x).max() > 2.0 ** 19
    xd = _dev(x)
    planes = torch.full((3 * n + 64,), -1, dtype=torch.int16, device="cuda")
    _check(lib.tts_op_split_planes(xd.data_ptr(), planes.data_ptr(), n, None))
    torch.cuda.synchronize()
    got = planes.cpu().numpy().view(np.uint16)
    assert (got[3 * n:] == go.GUARD_BF16).all()
    assert np.array_equal(got[:3 * n].reshape(3, n), go.planes_bits(x))


# one shape per branch of the engine's two wrappers (launch_gemm_x3p, launch_gemm_f32) with the
# form each must name: (M, N, K, A operand, B operands given, form)
ENGINE_CHOICE = [
    (8192, 2048, 32, "Ap", "Bp", "x3p_t0_ilv1"), (2048, 2048, 32, "Ap", "Bp", "x3p_t1_ilv1"),
    (1024, 2048, 32, "Ap", "Bp", "x3p_t2_ilv0"), (512, 2048, 32, "Ap", "Bp", "x3p_t3_ilv1"),
    (100, 130, 64, "Ap", "Bp", "x3p_t4_ilv0"),
    (8192, 2048, 32, "A+Ap", "B+Bp", "bx3_256x128_ApBp"), (2048, 2048, 32, "A+Ap", "B+Bp", "bx3_128x128_ApBp"),
    (8192, 2048, 32, "A", "B+Bp", "bx3_256x128_Bp"), (2048, 2048, 32, "A", "B+Bp", "bx3_128x128_Bp"),
    (100, 130, 64, "A", "B+Bp", "bx3_64x64_Bp"), (2048, 2048, 32, "A", "B", "bx3_128x128"),
    (100, 130, 64, "A", "B", "bx3_64x64"), (100, 130, 48, "A", "B", "f32_64x64_k16"),
    (2048, 2048, 16, "A", "B", "f32_128x128_k16"),
]


@pytest.mark.parametrize("M,N,K,a_kind,b_kind,name", ENGINE_CHOICE, ids=[f"{e[5]}_{e[3]}_{e[4]}" for e in ENGINE_CHOICE])
def test_engine_choice_is_the_named_form(lib, M, N, K, a_kind, b_kind, name):
    """form -1 (the wrappers the engine calls, default switches) gives the bits of the explicit
    form its heuristic names."""
    set_ = sorted(k for k in os.environ if k.startswith("TTS_CODEC_"))
    assert not set_, f"the wrappers' defaults are under test: unset {set_}"
    g = torch.Generator().manual_seed(M + N + K)
    A, B = torch.randn(M, K, generator=g).cuda(), torch.randn(N, K, generator=g).cuda()
    bias = torch.randn(N, generator=g).cuda()
    Ap = torch.empty(3 * M * K, dtype=torch.int16, device="cuda")
    Bp = torch.empty(3 * N * K, dtype=torch.int16, device="cuda")
    _check(lib.tts_op_split_planes(A.data_ptr(), Ap.data_ptr(), M * K, None))
    _check(lib.tts_op_split_planes(B.data_ptr(), Bp.data_ptr(), N * K, None))
    form, _, _, _, fa, fb = go.FORMS[name]
    outs = []
    for f, ak, bk in ((-1, a_kind, b_kind), (form, fa, fb)):
        C = torch.full((M, N), float("nan"), device="cuda")
        _check(lib.tts_op_gemm_planes(
            _ptr(A) if "A" in ak.split("+") else None, _ptr(Ap) if "Ap" in ak.split("+") else None, M * K, M, K, K,
            _ptr(B) if "B" in bk.split("+") else None, _ptr(Bp) if "Bp" in bk.split("+") else None, N,
            bias.data_ptr(), C.data_ptr(), None, 0, N, None, 1, f, None))
        torch.cuda.synchronize()
        outs.append(C)
    assert not torch.isnan(outs[0]).any()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    # (the forms' accuracy is test_form_against_fp64's; this only shows that both launches ran)
    ref = torch.nn.functional.silu(A[:64].double() @ B.double().t() + bias.double())
    assert (outs[0][:64].double() - ref).abs().max().item() < 1e-4
