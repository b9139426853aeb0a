"""The two stages of the lane DP (phase_filldp, lamsa_amd/csrc/hp_phase.h; k_filldp_small<stage>) on the device: the job sets of tests/lanedp_jobs.py
(the same sets as tests/test_lanedp_stages_cpu.py, whose counters show which exits each set takes) through lamsa_hp_dp_batch kinds 12 / 13 -- the jobs
listed into the lane queues and run by the read path's own launches -- against reflib.oracle_dp word for word, in two stages and in one
(LAMSA_HP_LANE_STAGES=0): the same CIGARs, every job published, the same cells per job, and exactly the hard jobs through the hard queues.  And the reads of
c3_ont and c2_pacbio through align_batch both ways: equal streams, the oracle's.  LAMSA_HP_LANE_STAGES is read once per process, so every
(preset or scenario, stages) runs in a fresh child (tests/lanedp_child.py), one after the other.  A child that dies by a signal, aborts or runs into its
time limit ends the session: nothing more is started on the GPU."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import goldenlib
import lanedp_child
import lanedp_jobs as LJ
import reflib

pytestmark = pytest.mark.gpu

CHILD = os.path.join(reflib.ROOT, "tests", "lanedp_child.py")
# seconds a child may take.  Measured on an MI355X (profiles/lanedp_stages_ab.txt): 0.5 - 0.7 s for the twenty sets of a preset (0.08 - 0.12 s of it in the
# GPU calls), 0.4 - 0.5 s for the reads of a scenario, library load included; the limit is three times the slowest, rounded up to the next ten.
CHILD_TIMEOUT = 10


def _child(mode, what, stages, tmp_path):
    dst = str(tmp_path / ("%s_%s_%d.npz" % (mode, what, stages)))
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, CHILD, mode, what, dst], env=dict(os.environ, LAMSA_HP_LANE_STAGES=str(stages)), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.exit("the child (%s %s, stages %d) did not finish within %d s: nothing more is run on the GPU" % (mode, what, stages, CHILD_TIMEOUT), returncode=1)
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit("the child (%s %s, stages %d) died (exit status %d): nothing more is run on the GPU\n%s" % (mode, what, stages, p.returncode, p.stderr[-2000:]), returncode=1)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(dst)
    print("%s %s stages %d: child %.1f s, GPU calls %.2f s" % (mode, what, stages, time.time() - t0, float(z["seconds"][0])))
    return z


@pytest.mark.parametrize("preset", LJ.PRESETS)
def test_job_sets_on_the_device(preset, tmp_path):
    reflib.build_oracle()
    lp = reflib.lo_para(preset)
    two, one = _child("sets", preset, 1, tmp_path), _child("sets", preset, 0, tmp_path)
    bad = []
    for size in LJ.SIZES:
        for mix in LJ.MIXES:
            jobs, types, exits = LJ.job_set(preset, size, mix)
            want = reflib.oracle_dp(jobs, lp, np.where(types == 1, reflib.KIND_BI, reflib.KIND_GLOBAL), lp.band_w, 100)["cigars"]
            k = lanedp_child.set_key(size, mix)
            for name, z in (("two stages", two), ("one stage", one)):
                if z[k + "_status"].any():
                    bad.append((size, mix, name, "jobs left to the fill", np.flatnonzero(z[k + "_status"]).tolist()[:5]))
                elif lanedp_child.unflat(z[k + "_words"], z[k + "_len"]) != want:
                    bad.append((size, mix, name, "differs from the oracle"))
            if two[k + "_cells"].tolist() != one[k + "_cells"].tolist():
                bad.append((size, mix, "cells per job differ"))
            if two[k + "_hard"].tolist() != (exits > 0).astype(int).tolist() or one[k + "_hard"].any():
                bad.append((size, mix, "the hard queues did not hold exactly the hard jobs"))
    assert bad == []


@pytest.mark.parametrize("name", ["c3_ont", "c2_pacbio"])
def test_golden_reads_in_two_stages_and_in_one(name, tmp_path):
    ref, reads, args, _ = goldenlib.stage_scenario(name, str(tmp_path))
    rt, over = goldenlib.para_from_args(args)
    lp = reflib.lo_para(rt, **over)
    want = reflib.oracle_streams(reflib.Batch(ref, reads, lp), lp)
    two, one = _child("reads", name, 1, tmp_path), _child("reads", name, 0, tmp_path)
    got2, got1 = lanedp_child.unflat(two["words"], two["len"]), lanedp_child.unflat(one["words"], one["len"])
    assert not two["status"].any() and not one["status"].any()
    assert [i for i in range(len(want)) if got2[i] != got1[i]] == [], "streams of the two ways differ"
    assert [i for i in range(len(want)) if got2[i] != want[i]] == []
