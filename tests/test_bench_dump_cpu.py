"""bench.dump_outputs on the CPU: what `bench.py --dump-outputs DIR` writes of a step's result, from made-up result buffers.
Two builds are compared file by file, so the files must not depend on where the kernels happened to put a read's words, must
hold every int32 word exactly and must stay within the size bound."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _result(seed, n=3000):
    """A result stream whose reads lie in the stream in a seeded order: (per-read words, stream, read_off, read_len, status)."""
    rng = np.random.default_rng(7)
    words = [rng.integers(-2**31, 2**31, int(rng.integers(0, 60)), dtype=np.int64).astype(np.int32) for _ in range(n)]
    words[0] = np.array([-2**31, 2**31 - 1], np.int32)
    status = (rng.random(n) < 0.01).astype(np.int32)
    r_off = np.zeros(n, np.int64)
    pos = 0
    for r in np.random.default_rng(seed).permutation(n):
        r_off[r] = pos
        pos += len(words[r])
    stream = np.zeros(max(pos, 1), np.int32)
    for r in range(n):
        stream[r_off[r]:r_off[r] + len(words[r])] = words[r]
    return words, stream, r_off, np.array([len(w) for w in words], np.int32), status


@pytest.fixture
def bench(monkeypatch):
    monkeypatch.setenv("LAMSA_NO_BUILD", "1")            # importing bench sets it; the other tests of the session keep what they had
    import bench
    return bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_independent_of_the_stream_layout_and_exact(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 19)
    words, *res = _result(seed=1)
    bench.dump_outputs(str(tmp_path / "a"), *res)
    bench.dump_outputs(str(tmp_path / "b"), *_result(seed=2)[1:])          # same reads, other completion order
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["read_len", "read_status", "stream", "stream_reads"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["read_len"], [len(w) for w in words]) and np.array_equal(a["read_status"], res[3])
    sel = a["stream_reads"].astype(np.int64)
    assert np.all(np.diff(sel) > 0) and 0 < len(sel) < len(words)
    assert np.array_equal(a["stream"], np.concatenate([words[r] for r in sel]).astype(np.float64))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES


def test_dump_keeps_every_read_when_the_words_fit(bench, tmp_path):
    words, *res = _result(seed=3, n=200)
    bench.dump_outputs(str(tmp_path), *res)
    a = _load(tmp_path)
    assert np.array_equal(a["stream_reads"], np.arange(200))
    assert np.array_equal(a["stream"], np.concatenate(words).astype(np.float64))
