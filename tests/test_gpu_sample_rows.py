"""The per-row samplers alone (tts_op_sample_rows: sample_rows_kernel / sample_list_rows_kernel).

Every row reads its own temperature, top_k, top_p and sample flag from device arrays.  A sampled
row must give, bit for bit, the token and the probs of the uniform sampler (tts_op_sample /
tts_op_sample_list) run on that row alone with the row's scalars and key; a greedy row gives the
argmax by float comparison, lowest id on ties, whatever temperature its table entry holds."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 4099
# (temperature, top_k, top_p) of the sampled rows; the sixth row is greedy (its entry: T 1.3, k 7, p 0.4)
SETTINGS = [(0.8, 50, 1.0), (0.7, 20, 0.9), (1.0, 1, 1.0), (1.3, 5, 0.5), (0.6, 1024, 0.95)]
GREEDY_ENTRY = (1.3, 7, 0.4)
SEEDS = [11, 2**63 + 5, 7, 123456789, 99, 42]
STEP = 3
PARTS = 64


@pytest.fixture(scope="module")
def lib():
    from tts_amd import _lib

    return _lib.load_library()


@pytest.fixture(scope="module")
def rows():
    """6 rows of V scores: a tie block at the top of row 0, one -inf entry in row 1, row 4 (k =
    1024) nearly flat, so no bound cuts it and the radix select runs with k = 1024."""
    g = torch.Generator().manual_seed(0xABC)
    x = torch.randn(6, V, generator=g) * 3.0
    top = x[0].max().item() + 0.5
    x[0, 100:108] = top
    x[1, 17] = float("-inf")
    x[4] = 1.0 + torch.randn(V, generator=g) * 1e-4
    return x.contiguous()


def _check(st):
    from tts_amd import _lib

    _lib.check(st)


def _parts(x, parts):
    """Maxima (and their ids, lowest on ties) of `parts` column blocks: what the lm_head leaves."""
    B, n = x.shape
    w = -(-n // parts)
    pad = np.full((B, parts * w), -np.inf, dtype=np.float32)
    pad[:, :n] = x.numpy()
    blk = pad.reshape(B, parts, w)
    idx = blk.argmax(axis=2)  # (first occurrence: the lowest id)
    val = np.take_along_axis(blk, idx[..., None], axis=2)[..., 0]
    return torch.from_numpy(val.copy()), torch.from_numpy((idx + np.arange(parts)[None] * w).astype(np.int32))


def _uniform_dense(lib, row, T, k, p, seed, parts=0):
    d = row[None].cuda().contiguous()
    probs = torch.zeros_like(d)
    tok = torch.empty(1, dtype=torch.int32, device="cuda")
    pm = _parts(row[None], parts)[0].cuda() if parts else None
    _check(lib.tts_op_sample(d.data_ptr(), 1, d.shape[1], T, k, p, seed, STEP, pm.data_ptr() if parts else None, parts,
                             probs.data_ptr(), tok.data_ptr(), None))
    torch.cuda.synchronize()
    return probs.cpu()[0], int(tok.cpu()[0])


def _uniform_list(lib, scores, ids, count, T, k, p, seed):
    s, i = scores[None].cuda().contiguous(), ids[None].to(torch.int32).cuda().contiguous()
    c = torch.tensor([count], dtype=torch.int32, device="cuda")
    probs = torch.zeros(1, V, device="cuda")
    tok = torch.empty(1, dtype=torch.int32, device="cuda")
    _check(lib.tts_op_sample_list(s.data_ptr(), i.data_ptr(), c.data_ptr(), 1, s.shape[1], V, T, k, p, seed, STEP,
                                  probs.data_ptr(), tok.data_ptr(), None))
    torch.cuda.synchronize()
    return probs.cpu()[0], int(tok.cpu()[0])


def _settings_arrays(settings, sample, seeds):
    T = torch.tensor([s[0] for s in settings], dtype=torch.float32, device="cuda")
    K = torch.tensor([s[1] for s in settings], dtype=torch.int32, device="cuda")
    P = torch.tensor([s[2] for s in settings], dtype=torch.float32, device="cuda")
    S = torch.tensor(sample, dtype=torch.int32, device="cuda")
    R = torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64)).cuda()
    return T, K, P, S, R


def _rows_op(lib, scores, settings, sample, seeds, ids=None, counts=None, parts=0, vocab=None):
    B, cap = scores.shape
    vocab = vocab or cap
    d = scores.cuda().contiguous()
    T, K, P, S, R = _settings_arrays(settings, sample, seeds)
    probs = torch.zeros(B, vocab, device="cuda")
    tok = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    di = ids.to(torch.int32).cuda().contiguous() if ids is not None else None
    dc = counts.to(torch.int32).cuda() if counts is not None else None
    pm = pi = None
    if parts:
        pm, pi = (t.cuda().contiguous() for t in _parts(scores, parts))
    _check(lib.tts_op_sample_rows(d.data_ptr(), di.data_ptr() if di is not None else None,
                                  dc.data_ptr() if dc is not None else None, B, cap, vocab, T.data_ptr(), K.data_ptr(),
                                  P.data_ptr(), S.data_ptr(), R.data_ptr(), STEP, pm.data_ptr() if parts else None,
                                  pi.data_ptr() if parts else None, parts, probs.data_ptr(), tok.data_ptr(), None))
    torch.cuda.synchronize()
    if dc is not None:
        assert torch.equal(dc.cpu(), counts.to(torch.int32))  # (only read)
    return probs.cpu(), tok.cpu().tolist()


def _first_argmax(row):
    return int(np.argmax(row.numpy()))  # (first occurrence = lowest id; +0.0 == -0.0)


@pytest.mark.parametrize("parts", [0, PARTS])
def test_dense_rows_equal_the_uniform_sampler_row_by_row(lib, rows, parts):
    settings = SETTINGS + [GREEDY_ENTRY]
    probs, tok = _rows_op(lib, rows, settings, [1] * 5 + [0], SEEDS, parts=parts)
    for b, (T, k, p) in enumerate(SETTINGS):
        rp, rt = _uniform_dense(lib, rows[b], T, k, p, SEEDS[b], parts)
        assert tok[b] == rt, (b, tok[b], rt)
        assert torch.equal(probs[b].view(torch.int32), rp.view(torch.int32)), b
        assert int((rp > 0).sum()) >= 1
    assert int((probs[0] > 0).sum()) >= 8  # (the tie block kept whole)
    assert int((probs[4] > 0).sum()) >= 100  # (the flat row: k = 1024 before top-p)
    assert tok[5] == _first_argmax(rows[5]) and float(probs[5].abs().sum()) == 0.0  # the greedy row: no probs


@pytest.mark.parametrize("n_list", [1500, 2049])
def test_list_rows_equal_the_uniform_list_sampler_row_by_row(lib, rows, n_list):
    """The same rows as scrambled lists of their top n_list entries (2049: above the kernel's
    2048 LDS candidates, the exact radix select over the list)."""
    g = torch.Generator().manual_seed(n_list)
    order = torch.argsort(rows, dim=1, descending=True, stable=True)[:, :n_list]
    perm = torch.stack([torch.randperm(n_list, generator=g) for _ in range(6)])
    ids = torch.gather(order, 1, perm)
    scores = torch.gather(rows, 1, ids).contiguous()
    counts = torch.full((6,), n_list)
    settings = SETTINGS + [GREEDY_ENTRY]
    probs, tok = _rows_op(lib, scores, settings, [1] * 5 + [0], SEEDS, ids=ids, counts=counts, vocab=V)
    for b, (T, k, p) in enumerate(SETTINGS):
        rp, rt = _uniform_list(lib, scores[b], ids[b], n_list, T, k, p, SEEDS[b])
        assert tok[b] == rt, (b, tok[b], rt)
        assert torch.equal(probs[b].view(torch.int32), rp.view(torch.int32)), b
        dp, dt = _uniform_dense(lib, rows[b], T, k, p, SEEDS[b])  # ... which is the dense row's draw
        assert rt == dt and torch.equal(rp.view(torch.int32), dp.view(torch.int32)), b
    assert tok[5] == _first_argmax(rows[5])


def _adjacent_floats_that_collide(T):
    """Adjacent float32 x < x' with fl(x / T) == fl(x' / T): x and x / T in one binade, where the
    quotients of neighbours lie less than an ulp apart."""
    t = np.float32(T)
    x = np.float32(6.0)
    for _ in range(10000):
        nx = np.nextafter(x, np.float32(np.inf))
        if np.float32(x / t) == np.float32(nx / t):
            return float(x), float(nx)
        x = nx
    raise AssertionError("no colliding pair found")


def _greedy_cases():
    g = torch.Generator().manual_seed(5)
    base = torch.randn(3, V, generator=g) - 8.0  # (everything else far below the planted maxima)
    want = []
    base[0, 2000:2060] = 4.25  # a 60-wide tie block at the maximum: its lowest id
    want.append(2000)
    x, nx = _adjacent_floats_that_collide(1.3)
    base[1, 300], base[1, 301] = x, nx  # x' > x at the higher id; v / 1.3 would make them a tie
    want.append(301)
    base[2].clamp_(max=-1.0)
    base[2, 1234], base[2, 3000] = -0.0, 0.0  # joint maximum: the lower id (the sort key has -0.0 < +0.0)
    want.append(1234)
    return base.contiguous(), want


@pytest.mark.parametrize("form", ["dense", "dense_parts", "list"])
def test_greedy_rows(lib, form):
    x, want = _greedy_cases()
    assert np.float32(x[1, 300].item()) < np.float32(x[1, 301].item())
    assert np.float32(np.float32(x[1, 300].item()) / np.float32(1.3)) == np.float32(np.float32(x[1, 301].item()) / np.float32(1.3))
    settings = [(1.3, 50, 0.9)] * 3  # (the table's temperature must not touch a greedy row)
    seeds = [1, 2, 3]
    if form == "list":
        g = torch.Generator().manual_seed(9)
        n = 1500
        order = torch.argsort(x, dim=1, descending=True, stable=True)[:, :n]
        ids = torch.gather(order, 1, torch.stack([torch.randperm(n, generator=g) for _ in range(3)]))
        for b, w in enumerate(want):
            assert w in ids[b].tolist()
        scores = torch.gather(x, 1, ids).contiguous()
        _, tok = _rows_op(lib, scores, settings, [0, 0, 0], seeds, ids=ids, counts=torch.full((3,), n), vocab=V)
    else:
        _, tok = _rows_op(lib, x, settings, [0, 0, 0], seeds, parts=PARTS if form == "dense_parts" else 0)
    assert tok == want, (form, tok, want)


def test_sampled_and_greedy_rows_do_not_disturb_each_other(lib, rows):
    """The same row sampled in two table positions with the same key draws the same token; a
    greedy row between them changes nothing."""
    x = torch.stack([rows[0], rows[5], rows[0]])
    settings = [SETTINGS[0], GREEDY_ENTRY, SETTINGS[0]]
    probs, tok = _rows_op(lib, x, settings, [1, 0, 1], [77, 1, 77])
    assert tok[0] == tok[2] and torch.equal(probs[0], probs[2])
    assert tok[1] == _first_argmax(rows[5])
