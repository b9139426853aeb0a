"""SV junctions on the MI355X: the hand-made reads and the fuzz batches of tests/sv_cases.py (the same batches as tests/test_sv_cpu.py, whose path
counters show which branch of split_sv and of the k-mer split mapper each read takes) through LamsaHp.align_batch, in process.  Per group of reads
that share parameters and reference one handle, and per handle three runs against the oracle's streams word for word: the batch as it comes, the
resident batch once more (upload_batch + run_uploaded), and the batch with the first pass's scratch capped at 128 KiB, so that every read overflows
the phased pass and takes k_align_batch (the handle's diagnostics must show that the retry pass ran).  A failure names the reads.

Measured on an MI355X: profiles/sv_junction_gpu.txt."""
import time

import pytest

import crafted
import reflib
import sv_cases

pytestmark = pytest.mark.gpu

FUZZ_N, FUZZ_SEED = 300, 7                                   # the batches of tests/test_sv_cpu.py


def _three_runs(h, batch, want, keys):
    """The reads (by key) whose status or stream differs from the oracle's in any of the three runs."""
    bad = []

    def compare(run, got, st):
        for k, key in enumerate(keys):
            if want[k][0] != 0 or want[k][1] < 1:
                continue                                     # a fuzz read the oracle does not align (tests/test_sv_cpu.py bounds their number)
            if int(st[k]) != 0:
                bad.append((key, run, "status %d" % int(st[k])))
            elif got[k] != want[k]:
                bad.append((key, run, "differs from the oracle"))
    compare("first", *h.align_batch(batch))
    h.upload_batch(batch)
    compare("resident", *h.run_uploaded())
    h.set_scratch_limit(128 << 10)
    try:
        got, st = h.align_batch(batch)
        assert h.last_kernel_ms(1) > 0, "the retry pass did not run"
        compare("one-kernel", got, st)
    finally:
        h.set_scratch_limit(0)
    return bad


def _handle(read_type, over, R):
    from lamsa_amd import hp
    return hp.LamsaHp(hp.make_para(read_type, **dict(over)), ref=(R.pac, R.l_pac, R.seq_off, R.seq_len), device=0)


def test_hand_made_sv_reads_on_the_device():
    reflib.build_oracle()
    bad, t_gpu = [], 0.0
    for (read_type, over, ref_key), cs in sorted(crafted.groups(sv_cases.cases()).items()):
        batch = crafted.concat([c.batch for c in cs])
        want = reflib.oracle_streams(batch, reflib.lo_para(read_type, **dict(over)), 4)
        for c, s in zip(cs, want):
            assert s[0] == 0 and s[1] >= 1, "the oracle does not align this read: %s (%s)" % (c.key, c.aim)
        t0 = time.time()
        h = _handle(read_type, over, sv_cases.ref_of(ref_key))
        try:
            bad += _three_runs(h, batch, want, [c.key for c in cs])
        finally:
            h.close()
        t_gpu += time.time() - t0
    print("hand-made SV reads: %d reads, %.2f s with the handles" % (len(sv_cases.cases()), t_gpu))
    assert bad == []


@pytest.mark.parametrize("preset", ["default", "ont2d"])
def test_sv_fuzz_on_the_device(preset):
    reflib.build_oracle()
    R, bs = sv_cases.fuzz(preset, FUZZ_N, FUZZ_SEED)
    batch = sv_cases.concat(bs)
    want = reflib.oracle_streams(batch, reflib.lo_para(preset), 4)
    t0 = time.time()
    h = _handle(preset, (), R)
    try:
        bad = _three_runs(h, batch, want, ["%s-fuzz-%d (kind %d)" % (preset, i, i % 5) for i in range(len(bs))])
    finally:
        h.close()
    print("SV fuzz %s: %d reads, %.2f s with the handle" % (preset, len(bs), time.time() - t0))
    assert bad == []
