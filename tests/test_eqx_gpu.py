"""LAMSA_HP_TAG_EQX on the MI355X: the =/X words the HIP kernels write into the result stream equal the checker's conversion
(tests/eqxcheck.py) of the flag-off stream, word for word, through the phased main pass, the streaming form and the second pass; and
the product binary's --eqx / --cs output, whose CIGARs the device makes, passes the assertions of the emulated CLI's tests."""
import os
import subprocess
import sys

import pytest

import eqxcheck as X
import goldenlib as G
import tagcheck as T

ROOT = G.ROOT
BIN = os.path.join(ROOT, "lamsa_amd", "bin", "lamsa")
pytestmark = pytest.mark.gpu

SHAPES = {"ont2d": ("ont2d", "ont2d", {}), "sv10k": ("default", "sv10k", {"SV_len_thd": 10000})}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_device_eqx_streams(shape):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import reflib
    import simbatch
    from lamsa_amd import hp
    rt, prof, over = SHAPES[shape]
    ref = simbatch.SimRef(20_000_000, n_contigs=4, seed=9, threads=16)
    B = simbatch.SimBatch(ref, 256, 4000, prof, seed=21, threads=16)
    h = hp.LamsaHp(hp.make_para(rt, **over), ref=(ref.pac, ref.l_pac, ref.seq_off, ref.seq_len), device=0)
    plain, st0 = h.align_batch(B)
    assert plain == reflib.oracle_streams(B, reflib.lo_para(rt, **over), 16)
    reads = [B.read_seq[B.read_off[r]:B.read_off[r + 1]] for r in range(B.n_reads)]
    want = [X.stream_to_eqx(plain[r], reads[r], B.pac, B.seq_off) for r in range(B.n_reads)]
    assert want != plain
    h.set_result_tags(hp.TAG_EQX)
    eq, st = h.align_batch(B)
    assert (st == st0).all()
    assert [r for r in range(B.n_reads) if eq[r] != want[r]] == []
    # both items: the =/X stream with the lists behind the CIGARs
    h.set_result_tags(hp.TAG_EQX | hp.TAG_MISMATCHES)
    both, st = h.align_batch(B)
    assert (st == st0).all()
    n_ev = 0
    for r in range(B.n_reads):
        s, ev = T.split_events(both[r])
        assert s == want[r], "read %d" % r
        assert ev == T.stream_events(plain[r], reads[r], B.pac, B.seq_off), "read %d" % r
        n_ev += sum(len(e) for e in ev)
    assert n_ev > B.n_reads
    # the streaming form: two batches in flight; the flags cannot change while they are
    h.set_result_tags(hp.TAG_EQX)
    half = list(range(B.n_reads // 2))
    h.submit_batch(simbatch.take(B, half)); h.submit_batch(B)
    with pytest.raises(RuntimeError):
        h.set_result_tags(0)
    a, _ = h.collect_batch(); b, _ = h.collect_batch()
    assert a == want[:len(half)] and b == want
    # every read through the second pass (one-kernel path, 8x capacities): a line's output words alone (12 per read base) are 190 KB here
    h.set_scratch_limit(128 << 10)
    again, st2 = h.align_batch(B)
    assert h.last_kernel_ms(1) > 0 and again == want and (st2 == st0).all()
    h.set_scratch_limit(0)
    with pytest.raises(RuntimeError):
        h.set_result_tags(4)
    h.set_result_tags(0)
    assert h.align_batch(B)[0] == plain
    h.close()


def _run(args, tmp_path, name):
    ref, reads, a, gold = G.stage_scenario(name, str(tmp_path))
    p = subprocess.run([BIN, "aln", "-N"] + args + a + [ref, reads], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, gold, X.load_reads(reads)


def _check_output(out, want, rf, reads, eqx=True, cs=True):
    flat = X.collapse(out)
    assert G.strip_pg(T.strip_tags(flat)) == G.strip_pg(want)
    assert T.check_sam(flat, *rf) == []
    assert X.check_sam(out, rf[0], rf[1], reads, eqx=eqx, cs=cs) == []


@pytest.mark.parametrize("name", G.SCENARIOS)
def test_product_binary_eqx_cs(name, tmp_path):
    assert os.path.exists(BIN), "lamsa_amd/bin/lamsa is not built"
    rf = T.load_ref(os.path.join(G.GOLD, "ref", "ref.fa"))
    tags = ["--eqx", "--cs", "--MD", "--SA"]
    out, gold, reads = _run(["-R", "0"] + tags, tmp_path, name)
    _check_output(out, gold, rf, reads)
    full, _, _ = _run(tags, tmp_path, name)
    want = G.golden_full(name) if name in G.RESCUE_SCENARIOS else gold
    _check_output(full, want, rf, reads)
    small, _, _ = _run(["--batch", "4"] + tags, tmp_path, name)
    assert G.strip_pg(small) == G.strip_pg(full)
    ref, rd, a, _ = G.stage_scenario(name, str(tmp_path))
    parts = [subprocess.run([BIN, "aln", "-N", "--shard", "%d/2" % i] + tags + a + [ref, rd], capture_output=True, text=True) for i in range(2)]
    assert all(q.returncode == 0 for q in parts)
    assert G.strip_pg(parts[0].stdout + parts[1].stdout) == G.strip_pg(full)
    # --eqx alone: the device builds the lists and does not ship them; nothing but the CIGARs changes
    alone, _, _ = _run(["--eqx"], tmp_path, name)
    assert "cs:Z" not in alone and "MD:Z" not in alone
    assert G.strip_pg(X.collapse(alone)) == G.strip_pg(want)
    assert X.check_sam(alone, rf[0], rf[1], reads, eqx=True, cs=False) == []
