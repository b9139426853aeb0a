"""LAMSA_HP_TAG_LEFT_ALIGN on the MI355X: the CIGAR words the HIP kernels write with the flag equal the checker's (tests/lalcheck.py:
the definition run element by element on the flag-off stream), word for word, through the phased main pass, the streaming form and
the second pass, alone and with the mismatch lists and the =/X form; and the product binary's --left-align output, whose gaps the
device shifts, passes the assertions of the emulated CLI's tests.

The shapes are the smallest at which records still span several blocks of 64 CIGAR elements; the checker's counters must show that
the inputs exercise what can go wrong -- gaps bound by the room in front of them, gaps that move on what the gap before them freed,
and such a pair on two sides of a block boundary."""
import os
import subprocess
import sys

import pytest

import eqxcheck as X
import goldenlib as G
import lalcheck as LA
import tagcheck as T

ROOT = G.ROOT
BIN = os.path.join(ROOT, "lamsa_amd", "bin", "lamsa")
pytestmark = pytest.mark.gpu

SHAPES = {"pacbio": ("pacbio", "pacbio", {}), "ont2d": ("ont2d", "ont2d", {}), "sv10k": ("default", "sv10k", {"SV_len_thd": 10000})}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_device_left_aligned_streams(shape):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import reflib
    import simbatch
    from lamsa_amd import hp
    rt, prof, over = SHAPES[shape]
    ref = simbatch.SimRef(20_000_000, n_contigs=4, seed=9, threads=16)
    B = simbatch.SimBatch(ref, 64, 4000, prof, seed=21, threads=16)
    h = hp.LamsaHp(hp.make_para(rt, **over), ref=(ref.pac, ref.l_pac, ref.seq_off, ref.seq_len), device=0)
    plain, st0 = h.align_batch(B)
    assert plain == reflib.oracle_streams(B, reflib.lo_para(rt, **over), 16)
    reads = [B.read_seq[B.read_off[r]:B.read_off[r + 1]] for r in range(B.n_reads)]
    st = LA.new_stats()
    want = [LA.stream_left_aligned(plain[r], reads[r], B.pac, B.seq_off, st) for r in range(B.n_reads)]
    print(shape, st)
    assert st["moved"] > 0 and want != plain
    if shape != "sv10k":                                               # the inputs reach the carry: within a block and across two
        assert st["room"] > 0 and st["cascade"] > 0 and st["cascade_block"] > 0, st
    h.set_result_tags(hp.TAG_LEFT_ALIGN)
    la, s = h.align_batch(B)
    assert (s == st0).all()
    assert [r for r in range(B.n_reads) if la[r] != want[r]] == []
    # with the lists, and with the lists and the =/X form: both describe the shifted alignment
    want_ev = [T.stream_events(want[r], reads[r], B.pac, B.seq_off) for r in range(B.n_reads)]
    want_eq = [X.stream_to_eqx(want[r], reads[r], B.pac, B.seq_off) for r in range(B.n_reads)]
    for flags, cig in ((hp.TAG_LEFT_ALIGN | hp.TAG_MISMATCHES, want), (hp.TAG_LEFT_ALIGN | hp.TAG_EQX | hp.TAG_MISMATCHES, want_eq)):
        h.set_result_tags(flags)
        got, s = h.align_batch(B)
        assert (s == st0).all()
        for r in range(B.n_reads):
            w, ev = T.split_events(got[r])
            assert w == cig[r] and ev == want_ev[r], "flags %d, read %d" % (flags, r)
    # the streaming form: two batches in flight; the flags cannot change while they are
    h.set_result_tags(hp.TAG_LEFT_ALIGN)
    half = list(range(B.n_reads // 2))
    h.submit_batch(simbatch.take(B, half)); h.submit_batch(B)
    with pytest.raises(RuntimeError):
        h.set_result_tags(0)
    a, _ = h.collect_batch(); b, _ = h.collect_batch()
    assert a == want[:len(half)] and b == want
    # every read through the second pass (one-kernel path, 8x capacities)
    h.set_scratch_limit(128 << 10)
    again, st2 = h.align_batch(B)
    assert h.last_kernel_ms(1) > 0 and again == want and (st2 == st0).all()
    h.set_scratch_limit(0)
    with pytest.raises(RuntimeError):
        h.set_result_tags(4)
    with pytest.raises(RuntimeError):
        h.set_result_tags(16)
    h.set_result_tags(0)
    assert h.align_batch(B)[0] == plain
    h.close()


def _run(args, tmp_path, name):
    ref, reads, a, gold = G.stage_scenario(name, str(tmp_path))
    p = subprocess.run([BIN, "aln", "-N"] + args + a + [ref, reads], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, gold, X.load_reads(reads)


@pytest.mark.parametrize("name", G.SCENARIOS)
def test_product_binary_left_align(name, tmp_path):
    assert os.path.exists(BIN), "lamsa_amd/bin/lamsa is not built"
    rf = T.load_ref(os.path.join(G.GOLD, "ref", "ref.fa"))
    tags = ["--eqx", "--cs", "--MD", "--SA"]
    for mode in (["-R", "0"], []):
        out, gold, reads = _run(mode + ["--left-align"] + tags, tmp_path, name)
        want = G.golden_full(name) if not mode and name in G.RESCUE_SCENARIOS else gold
        # the three checkers on the output itself
        assert T.check_sam(X.collapse(out), *rf) == []
        assert X.check_sam(out, rf[0], rf[1], reads) == []
        # and against the golden: without the tags and in M form it is the golden with the checker's CIGARs
        moved, n = LA.replace_cigars(want, rf[0], rf[1], reads)
        assert n > 0 and G.strip_pg(T.strip_tags(X.collapse(out))) == G.strip_pg(moved)
        assert LA.check_sam(want, T.strip_tags(out), rf[0], rf[1], reads) == []
        if not mode and name in ("c2_pacbio", "c7_rescue"):            # (two runs more: only where there is most to move / stage 4)
            alone, _, _ = _run(["--left-align"], tmp_path, name)
            assert G.strip_pg(alone) == G.strip_pg(moved)
            small, _, _ = _run(["--batch", "4", "--left-align"] + tags, tmp_path, name)
            assert G.strip_pg(small) == G.strip_pg(out)
