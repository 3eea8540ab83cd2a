"""bench.py --dump-outputs: the files a step's outputs become, on CPU (no engine involved)."""

import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _step_outputs():
    rng = np.random.default_rng(3)
    ids = [rng.integers(0, 193856, size=n).tolist() for n in (7, 5, 7)]
    wavs = [rng.standard_normal(n * 480).astype(np.float32) for n in (9, 7, 9)]
    return ids, wavs


def test_dump_writes_ids_and_whole_waveforms(tmp_path):
    ids, wavs = _step_outputs()
    bench.dump_outputs(str(tmp_path / "out"), ids, wavs)
    got = {f: np.load(tmp_path / "out" / f) for f in sorted(os.listdir(tmp_path / "out"))}
    assert sorted(got) == ["ids.npy", "waveform_lengths.npy", "waveforms.npy"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["ids.npy"].shape == (3, 7)
    for r, u in enumerate(ids):
        assert got["ids.npy"][r, :len(u)].tolist() == u and (got["ids.npy"][r, len(u):] == -1).all()
    assert got["waveform_lengths.npy"].tolist() == [w.size for w in wavs]
    assert got["waveforms.npy"].dtype == np.float32
    assert np.array_equal(got["waveforms.npy"], np.concatenate(wavs))


def test_dump_samples_large_waveforms_the_same_way_every_time(tmp_path):
    ids, wavs = _step_outputs()
    flat = np.concatenate(wavs)
    limit = flat.nbytes  # (the waveforms alone are past half of it)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), ids, wavs, max_bytes=limit)
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(a) == sorted(b) and all(np.array_equal(a[f], b[f]) for f in a)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= limit
    idx = a["waveform_sample_index.npy"]
    assert idx.dtype == np.float64 and (np.diff(idx) > 0).all() and 0 < idx.size < flat.size
    assert np.array_equal(a["waveforms.npy"], flat[idx.astype(np.int64)])
    # a later run whose waveforms fit leaves no stale index behind
    bench.dump_outputs(str(tmp_path / "a"), ids, wavs)
    assert not os.path.exists(tmp_path / "a" / "waveform_sample_index.npy")


def test_bench_has_the_full_and_dump_options():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout
