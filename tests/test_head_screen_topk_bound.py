"""CPU restatement of the screened sampling head's threshold (lm_head_screen.hip's top-k mode,
DESIGN.md §3.6), on the bounds tests/test_head_screen_bound.py restates.

TopKLogitsWarper keeps {c : s_c >= k-th largest s} (ties at the k-th value kept).  The screen
gives lb_c <= s_c <= ub_c.  Every workgroup publishes the maximum of lb over its own columns
(disjoint sets), and T = the k-th largest of the published maxima a workgroup can see (-inf with
fewer than k of them).  Those are lb values of k distinct columns, so T <= the k-th largest s;
every kept column has ub_c >= s_c >= T, so it lies in a unit (16 columns) whose maximum of ub
reaches T — the units the kernel recomputes — and passes the kernel's `score >= T` when appended.
Checked in numpy at TTS-1's K on uniform, heavy-tailed and twin matrices, for fp32 sums in three
k orders, with every group visible and with a random half missing (a wait that gave up)."""

import importlib.util
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


B = _load("test_head_screen_bound")
K, V = B.K, B.V
UNITS = V // 16


def groups(grid):
    """Units of each workgroup: wave gw = 4 b + w streams units gw, gw + 4 grid, ... (interleaved)."""
    ur = 4 * grid
    return [np.array([u for w in range(4) for u in range(4 * b + w, UNITS, ur)]) for b in range(grid)]


def scores_and_bounds(W, x, seen, penalty, rng):
    W, x = B.bf16(W), B.bf16(x)
    scale, q, r, nW, nWh = B.quantise_columns(W)
    sx, X, nx, ndx = B.quantise_row(x)
    a = np.float64(sx) * scale.astype(np.float64) * (q @ X).astype(np.float64)
    e = nx * (r + 2.0 * K * 2.0 ** -24 * nW) + ndx * nWh + 1e-12 * np.abs(a) + 1e-30

    def proc(v):  # repetition penalty on the seen ids, in fp32 after the bf16 rounding
        v = B.bf16(v).astype(np.float32)
        pv = np.where(v < 0, v * np.float32(penalty), v / np.float32(penalty)).astype(np.float32)
        return np.where(seen, pv, v)

    orders = [np.arange(K), np.arange(K)[::-1], rng.permutation(K)]
    return [proc(B.fp32_dots(x, W, o)) for o in orders], proc(a - e), proc(a + e)


def threshold(lb, grp, visible, k):
    mx = sorted((float(lb[np.add.outer(grp[g] * 16, np.arange(16)).ravel()].max()) for g in visible), reverse=True)
    return mx[k - 1] if len(mx) >= k else -np.inf


def check(W, x, seen, penalty, seed):
    rng = np.random.default_rng(seed)
    ss, lb, ub = scores_and_bounds(W, x, seen, penalty, rng)
    assert all(np.all(lb <= s) and np.all(s <= ub) for s in ss)
    umax = ub.reshape(UNITS, 16).max(axis=1)
    flagged_counts = {}
    for grid in (16, 64):
        grp = groups(grid)
        assert sorted(np.concatenate(grp).tolist()) == list(range(UNITS))  # disjoint, complete
        half = sorted(rng.permutation(grid)[:grid // 2].tolist())
        for k in (1, 5, 50):
            for visible in (range(grid), half):
                T = threshold(lb, grp, visible, k)
                if len(visible) < k:
                    assert T == -np.inf
                flagged = np.repeat(umax >= T, 16)
                for s in ss:
                    kth = np.sort(s)[-k]
                    assert T <= kth
                    keep = s >= kth  # the top-k set, ties at the k-th value included
                    assert keep.sum() >= k
                    assert np.all(flagged[keep]) and np.all(s[keep] >= T)
                    # and nothing outside the recomputed units could have entered it
                    assert np.all(s[~flagged] < kth) or T == -np.inf
                if visible is not half:
                    flagged_counts[(grid, k)] = int((umax >= T).sum())
    return flagged_counts


def test_threshold_holds_for_uniform_weights():
    rng = np.random.default_rng(1)
    W = rng.uniform(-0.05, 0.05, size=(V, K)).astype(np.float32)
    x = rng.standard_normal(K).astype(np.float32) * np.float32(1.5)
    n = check(W, x, rng.random(V) < 0.02, 1.1, 11)
    assert n[(64, 50)] < UNITS and n[(64, 1)] <= n[(64, 5)] <= n[(64, 50)]
    assert n[(16, 50)] == UNITS  # 16 groups, k = 50: -inf, every unit


def test_threshold_holds_for_heavy_tailed_weights():
    rng = np.random.default_rng(2)
    W = rng.standard_normal((V, K)).astype(np.float32) * np.float32(0.02)
    W[::7] *= 8
    W[rng.random(W.shape) < 1.0 / 64] *= 40
    x = (rng.standard_t(3, K) * 0.7).astype(np.float32)
    check(W, x, rng.random(V) < 0.05, 1.4, 12)


def test_ties_at_the_kth_value_stay_in_the_candidate_set():
    rng = np.random.default_rng(3)
    W = rng.uniform(-0.05, 0.05, size=(V, K)).astype(np.float32)
    W[1::2] = W[0::2]  # every score has an exact twin: odd k cuts between the two of a pair
    x = rng.standard_normal(K).astype(np.float32)
    rng2 = np.random.default_rng(13)
    ss, lb, ub = scores_and_bounds(W, x, np.zeros(V, bool), 1.0, rng2)
    for s in ss:
        kth = np.sort(s)[-5]
        assert (s >= kth).sum() == 6  # the tied pair at the boundary is kept whole
    check(W, x, np.zeros(V, bool), 1.0, 13)


def test_fewer_groups_than_k_gives_no_threshold():
    lb = np.arange(V, dtype=np.float32)
    grp = groups(16)
    assert threshold(lb, grp, range(16), 17) == -np.inf
    assert threshold(lb, grp, range(16), 16) > -np.inf
    assert threshold(lb, grp, [0, 3, 5], 5) == -np.inf


# ------------------------------------------------------------------------ the spill gate ----
def test_sampled_plan_instantiations_do_not_spill():
    """The gate tests/test_kernel_resources.py applies to the greedy plan, on the kernels the
    sampled step's plan lists (the screen's top-k instantiations and the list sampler)."""
    R = _load("test_kernel_resources")
    if not os.path.exists(R.HIPCC):
        pytest.skip("hipcc not installed")
    import dataclasses
    import sys

    sys.path.insert(0, os.path.join(R.ROOT, "tts-max_amd"))
    from tts_amd import configs
    from tts_amd.speechlm import step_plan

    want = set()
    for arch, rows in [("tts1", r) for r in (1, 2, 4, 5, 8, 9, 16)] + [("tts1-max", r) for r in (1, 4, 5, 8)]:
        plan = step_plan(dataclasses.replace(configs.LM_ARCHS[arch], num_layers=2), rows, top_k=50)
        scr = [k for k in plan if k.startswith("head_screen_kernel<")]
        assert len(scr) == 1 and "sample_list_kernel" in plan, (arch, rows, plan)
        args = [a.strip() for a in scr[0][len("head_screen_kernel<"):-1].split(",")]
        assert args[-2:] == ["false", "true"], scr
        want.add("head_screen_kernelI" + "".join({"false": "Lb0E", "true": "Lb1E"}.get(a, f"Li{a}E") for a in args) + "E")
    assert len(want) == 5, want
    want.add("sample_list_kernel")
    spills = {}
    for unit in ("lm_head_screen.hip", "lm_sample.hip"):
        spills.update(R._remarks(unit))
    for w in want:
        hit = {n: v for n, v in spills.items() if re.search(re.escape(w), n)}
        assert hit, f"{w}: not compiled"
        assert all(v == 0 for v in hit.values()), f"VGPR spills: {hit}"
