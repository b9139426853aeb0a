"""The mismatch lists of the result stream (lamsa_hp_set_result_tags) made by the HIP kernels on the MI355X, and the --MD / --SA
tags of the product binary built on them: every list equals the checker's recomputation (tests/tagcheck.py), and the stream with
the lists taken out is the flag-off stream and the oracle's, word for word.  The binding calls the product library, which always
lists the mismatches on the device: these tests are what shows the device's lists right."""
import os
import subprocess
import sys

import numpy as np
import pytest

import goldenlib as G
import tagcheck as T

ROOT = G.ROOT
BIN = os.path.join(ROOT, "lamsa_amd", "bin", "lamsa")
pytestmark = pytest.mark.gpu

SHAPES = {"ont10k": ("ont2d", "ont2d", 10000, {}), "sv10k": ("default", "sv10k", 10000, {"SV_len_thd": 10000}),
          "pb20k": ("pacbio", "pb20k", 20000, {"band_w": 200})}


def _check_events(tagged, plain, B):
    """tagged / plain: per-read streams with and without the lists; returns the number of lists checked."""
    n = 0
    for r in range(B.n_reads):
        s, ev = T.split_events(tagged[r])
        assert s == plain[r], "read %d: stream without the lists differs from the flag-off stream" % r
        read = B.read_seq[B.read_off[r]:B.read_off[r + 1]]
        want = T.stream_events(s, read, B.pac, B.seq_off)
        assert ev == want, "read %d: device mismatch lists differ from the recomputation" % r
        n += len(ev)
    return n


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_device_mismatch_lists(shape):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import reflib
    import simbatch
    from lamsa_amd import hp
    rt, prof, L, over = SHAPES[shape]
    ref = simbatch.SimRef(60_000_000, n_contigs=4, seed=9, threads=16)
    B = simbatch.SimBatch(ref, 4096 if L <= 10000 else 2048, L, prof, seed=21, threads=16)
    h = hp.LamsaHp(hp.make_para(rt, **over), ref=(ref.pac, ref.l_pac, ref.seq_off, ref.seq_len), device=0)
    plain, st0 = h.align_batch(B)
    assert plain == reflib.oracle_streams(B, reflib.lo_para(rt, **over), 16)
    h.set_result_tags(hp.TAG_MISMATCHES)
    tagged, st = h.align_batch(B)
    assert (st == st0).all()
    assert _check_events(tagged, plain, B) > B.n_reads
    # the streaming form: two batches in flight; the flag cannot change while they are
    half = list(range(B.n_reads // 2))
    h.submit_batch(simbatch.take(B, half)); h.submit_batch(B)
    with pytest.raises(RuntimeError):
        h.set_result_tags(0)
    a, _ = h.collect_batch(); b, _ = h.collect_batch()
    assert a == tagged[:len(half)] and b == tagged
    # every read through the second pass (one-kernel path, 8x capacities)
    h.set_scratch_limit(600 << 10)
    again, st2 = h.align_batch(B)
    assert h.last_kernel_ms(1) > 0 and again == tagged and (st2 == st0).all()
    h.set_scratch_limit(0)
    h.set_result_tags(0)
    assert h.align_batch(B)[0] == plain
    h.close()


def _tagged_run(args, tmp_path, name):
    ref, reads, a, gold = G.stage_scenario(name, str(tmp_path))
    p = subprocess.run([BIN, "aln", "-N", "--MD", "--SA"] + args + a + [ref, reads], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, gold


@pytest.mark.parametrize("name", G.SCENARIOS)
def test_product_binary_tags(name, tmp_path):
    assert os.path.exists(BIN), "lamsa_amd/bin/lamsa is not built"
    rf = T.load_ref(os.path.join(G.GOLD, "ref", "ref.fa"))
    out, gold = _tagged_run(["-R", "0"], tmp_path, name)
    assert G.strip_pg(T.strip_tags(out)) == G.strip_pg(gold)
    assert T.check_sam(out, *rf) == []
    full, _ = _tagged_run([], tmp_path, name)
    want = G.golden_full(name) if name in G.RESCUE_SCENARIOS else gold
    assert G.strip_pg(T.strip_tags(full)) == G.strip_pg(want)
    assert T.check_sam(full, *rf) == []
    small, _ = _tagged_run(["--batch", "4"], tmp_path, name)
    assert G.strip_pg(small) == G.strip_pg(full)
    ref, reads, a, _ = G.stage_scenario(name, str(tmp_path))
    parts = [subprocess.run([BIN, "aln", "-N", "--MD", "--SA", "--shard", "%d/2" % i] + a + [ref, reads], capture_output=True, text=True) for i in range(2)]
    assert all(q.returncode == 0 for q in parts)
    assert G.strip_pg(parts[0].stdout + parts[1].stdout) == G.strip_pg(full)


def test_end_to_end_files_at_scale_with_tags(tmp_path):
    """1024 simulated 6-kbp ONT-like reads in several GPU batches: --MD --SA pass the checker and change nothing else."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import simbatch
    import simfiles
    ref = simbatch.SimRef(200_000_000, n_contigs=6, seed=5, threads=8)
    B = simbatch.SimBatch(ref, 1024, 6000, "ont2d", seed=31, threads=8)
    d = str(tmp_path)
    simfiles.write_index(d + "/ref.fa", ref)
    simfiles.write_reads(d + "/reads.fa", B)
    base = [BIN, "aln", "-N", "-T", "ont2d", "-R", "0", "-t", "16", "--batch", "300"]
    plain = subprocess.run(base + [d + "/ref.fa", d + "/reads.fa"], capture_output=True, text=True)
    tagged = subprocess.run(base + ["--MD", "--SA", d + "/ref.fa", d + "/reads.fa"], capture_output=True, text=True)
    assert plain.returncode == 0 and tagged.returncode == 0, tagged.stderr[-2000:]
    assert G.strip_pg(T.strip_tags(tagged.stdout)) == G.strip_pg(plain.stdout)
    assert tagged.stdout.count("\tMD:Z:") >= 1000
    assert T.check_sam(tagged.stdout, *T.load_ref(d + "/ref.fa")) == []
