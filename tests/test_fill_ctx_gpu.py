"""The fill launches keep one read context per wave (hp_phase.h): a wave of k_fill / k_filllist reuses its block for every line
it takes from the queue.  The fixtures and the small simulated batches of the other GPU tests give a wave one or two lines;
here a batch has several times as many lines as the GPU holds waves of k_fill, so every wave fills many different reads, of
both strands, one after the other out of the same block."""
import os
import sys

import pytest

import reflib

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(reflib.ROOT, "tools"))

# waves of k_fill resident on an MI355X: 256 CUs x 4 SIMDs x 7 waves per SIMD (HP_FILL_WAVES_PER_SIMD)
RESIDENT_WAVES = 256 * 4 * 7


@pytest.mark.parametrize("read_type,profile,n,length", [("default", "default", 36000, 1000), ("ont2d", "ont2d", 24000, 1500)])
def test_many_lines_per_wave_match_the_oracle(read_type, profile, n, length):
    """Every read of a batch with more than four lines per resident wave: the oracle's stream, word for word, and again on a second
    run over the resident batch (the blocks then hold what the first run left)."""
    import simbatch
    from lamsa_amd import hp
    # a reference without planted repeat families: which of several equally good loci the chaining reports is not this test's subject
    ref = simbatch.SimRef(64_000_000, n_contigs=4, seed=9, threads=8, repeats=False)
    B = simbatch.SimBatch(ref, n, length, profile, seed=21, threads=8)
    lp = reflib.lo_para(read_type)
    want = reflib.oracle_streams(B, lp, 16)
    lines = sum(w[1] + w[2] for w in want if len(w) > 3)
    assert lines >= 4 * RESIDENT_WAVES
    assert {int(s) for s in B.t_strand} >= {1, -1}
    h = hp.LamsaHp(hp.make_para(read_type), ref=(ref.pac, ref.l_pac, ref.seq_off, ref.seq_len))
    try:
        h.upload_batch(B)
        got, st = h.run_uploaded()
        again, st2 = h.run_uploaded()
    finally:
        h.close()
    assert (st == 0).all() and (st2 == 0).all()
    assert [i for i in range(n) if got[i] != want[i]][:8] == []
    assert again == got
