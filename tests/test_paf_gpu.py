"""LAMSA_HP_TAG_SUMMARY on the MI355X: the 15-word records the HIP kernels write with the flag equal the checker's summaries
(tests/pafcheck.py) of the flag-off stream, word for word, through the phased main pass, the streaming form and the second pass; and
the product binary's --paf / --paf-cg output, whose summaries the device makes, equals the checker's PAF of the golden SAM.

The shapes are those of tests/test_lalign_gpu.py: the smallest at which records still span several blocks of 64 CIGAR elements and
lines of several records occur (sv10k); the checker's counters must show it."""
import os
import subprocess
import sys

import pytest

import goldenlib as G
import pafcheck as P

ROOT = G.ROOT
BIN = os.path.join(ROOT, "lamsa_amd", "bin", "lamsa")
pytestmark = pytest.mark.gpu

SHAPES = {"pacbio": ("pacbio", "pacbio", {}), "ont2d": ("ont2d", "ont2d", {}), "sv10k": ("default", "sv10k", {"SV_len_thd": 10000})}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_device_summary_streams(shape):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import reflib
    import simbatch
    from lamsa_amd import hp
    rt, prof, over = SHAPES[shape]
    ref = simbatch.SimRef(20_000_000, n_contigs=4, seed=9, threads=16)
    B = simbatch.SimBatch(ref, 64, 4000, prof, seed=21, threads=16)
    para = hp.make_para(rt, **over)
    h = hp.LamsaHp(para, ref=(ref.pac, ref.l_pac, ref.seq_off, ref.seq_len), device=0)
    # 1. plain == oracle
    plain, st0 = h.align_batch(B)
    assert plain == reflib.oracle_streams(B, reflib.lo_para(rt, **over), 16)
    L = [int(B.read_off[r + 1] - B.read_off[r]) for r in range(B.n_reads)]
    st = P.new_stats()
    want = [P.stream_summaries(plain[r], L[r], para, st) for r in range(B.n_reads)]
    print(shape, st, "words", sum(len(x) for x in plain), "->", sum(len(x) for x in want))
    assert want != plain and st["minus"] > 0 and st["long_cigar"] > 0, st
    if shape == "sv10k":                                               # lines of several records (their clips are on one end each: records clipped
        assert st["multi_rec"] > 0, st                                 # on both ends come with the golden scenarios below)
    # 2. with the flag: the checker's summaries, the statuses unchanged
    h.set_result_tags(hp.TAG_SUMMARY)
    got, s = h.align_batch(B)
    assert (s == st0).all()
    assert [r for r in range(B.n_reads) if got[r] != want[r]] == []
    # 3. with left alignment: word for word the same
    h.set_result_tags(hp.TAG_SUMMARY | hp.TAG_LEFT_ALIGN)
    both, s = h.align_batch(B)
    assert (s == st0).all() and both == want
    # 4. the refused flags
    for flags in (hp.TAG_SUMMARY | hp.TAG_MISMATCHES, hp.TAG_SUMMARY | hp.TAG_EQX, 4, 16, 64):
        with pytest.raises(RuntimeError):
            h.set_result_tags(flags)
    # 5. the streaming form: two batches in flight; the flags cannot change while they are
    h.set_result_tags(hp.TAG_SUMMARY)
    half = list(range(B.n_reads // 2))
    h.submit_batch(simbatch.take(B, half)); h.submit_batch(B)
    with pytest.raises(RuntimeError):
        h.set_result_tags(0)
    a, _ = h.collect_batch(); b, _ = h.collect_batch()
    assert a == want[:len(half)] and b == want
    # 6. every read through the second pass (one-kernel path, 8x capacities)
    h.set_scratch_limit(128 << 10)
    again, st2 = h.align_batch(B)
    assert h.last_kernel_ms(1) > 0 and again == want and (st2 == st0).all()
    h.set_scratch_limit(0)
    # 7. back to 0 == plain
    h.set_result_tags(0)
    assert h.align_batch(B)[0] == plain
    h.close()


def _run(args, tmp_path, name):
    ref, reads, a, gold = G.stage_scenario(name, str(tmp_path))
    p = subprocess.run([BIN, "aln", "-N"] + args + a + [ref, reads], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, gold


@pytest.mark.parametrize("name", G.SCENARIOS)
def test_product_binary_paf(name, tmp_path):
    assert os.path.exists(BIN), "lamsa_amd/bin/lamsa is not built"
    tags = ["--eqx", "--cs", "--MD", "--left-align"]
    st = P.new_stats()
    for mode in (["-R", "0"], []):
        out, gold = _run(mode + ["--paf"], tmp_path, name)
        want = G.golden_full(name) if not mode and name in G.RESCUE_SCENARIOS else gold
        assert out == P.sam_to_paf(want, P.contig_lengths(gold), False, st), mode
        if not mode:
            sam, _ = _run(tags, tmp_path, name)
            cg, _ = _run(tags + ["--paf-cg"], tmp_path, name)
            assert cg == P.sam_to_paf(sam, P.contig_lengths(sam), True) and "\tcg:Z:" in cg
            if name in ("c2_pacbio", "c7_rescue"):                     # (two runs more: only where the records are longest / stage 4 adds some)
                assert _run(["--batch", "4", "--paf"], tmp_path, name)[0] == out
                assert _run(["--batch", "4"] + tags + ["--paf-cg"], tmp_path, name)[0] == cg
    assert st["minus"] > 0, st
    if name == "c7_rescue":
        assert st["both_clips"] > 0 and st["xa"] > 0, st
