"""bench.py on the MI355X at a toy size: a plain run prints the headline line and nothing of the --full legs, and --dump-outputs
writes the same arrays from two runs with the same arguments (the inputs are seeded, the outputs integer-exact)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_and_dumped_outputs(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--reads", "256", "--ref-bp", "48000000", "--threads", "8"]
    lines = []
    for k in range(2):
        p = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / str(k))], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        lines.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1]))
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "Gbase/s" and d["higher_is_better"] is True and d["dtype"] == "int32" and d["metric"].startswith("aligned Gbase/s")
    assert not {"roofline", "cpu_baseline", "pcie_inclusive_reads_per_s", "pcie_inclusive_streamed_reads_per_s"} & set(d)
    files = sorted(os.listdir(tmp_path / "0"))
    assert files == ["read_len.npy", "read_status.npy", "stream.npy", "stream_reads.npy"]
    a = {f: np.load(tmp_path / "0" / f) for f in files}
    for f in files:
        assert a[f].dtype == np.float64 and np.array_equal(a[f], np.load(tmp_path / "1" / f)), f
    assert len(a["read_len.npy"]) == 256 and len(a["stream_reads.npy"]) == 256          # a small batch: every read's words fit
    assert len(a["stream.npy"]) == a["read_len.npy"].sum()
    assert sum(os.path.getsize(tmp_path / "0" / f) for f in files) <= 64_000_000
