"""The job sets of test_rebase_cpu.py on the MI355X: lamsa_hp_dp_batch kinds 1 (ksw_extend), 10 and 11 (a line's head and tail extension as
k_filldp_wave runs them) against the oracle, bit for bit -- score, qle, tle, CIGAR.  Every parameter set runs in a child process of its own
(tests/rebase_jobs.py as a program), one after the other.  A child that dies by a signal, aborts or runs into its time limit ends the session:
nothing more is started on the GPU."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import goldenlib
import rebase_jobs as rj
import reflib

pytestmark = pytest.mark.gpu

CHILD = os.path.join(reflib.ROOT, "tests", "rebase_jobs.py")
# seconds a child may take: three times the slowest measured on an MI355X, rounded up to the next ten (profiles/rebase_window_ab.txt)
CHILD_TIMEOUT = 10


@pytest.mark.parametrize("name", rj.PRESETS + tuple(sorted(rj.EXT_NS)))
def test_rebased_window_on_the_device(name, tmp_path):
    lp = rj.lo_para(name)
    jobs = rj.make_jobs(rj.SEEDS[name])
    wj = rj.wave_jobs(jobs)
    dst = str(tmp_path / "out.npz")
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, CHILD, name, dst], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.exit("the child of parameter set %s did not finish within %d s: nothing more is run on the GPU" % (name, CHILD_TIMEOUT), returncode=1)
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit("the child of parameter set %s died (exit status %d): nothing more is run on the GPU\n%s" % (name, p.returncode, p.stderr[-2000:]), returncode=1)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(dst)
    print("%s: child %.1f s, its dp_batch calls %.2f s" % (name, time.time() - t0, float(z["seconds"][0])))
    for k, (kind, w, h0) in enumerate(rj.runs(name, lp, jobs)):
        got = {f: z["r%d_%s" % (k, f)] for f in ("score", "qle", "tle", "status")}
        got["cigars"] = rj.unflat(z["r%d_cig" % k], z["r%d_cn" % k])
        if kind == 1:
            assert goldenlib.same_dp(reflib.oracle_dp(jobs, lp, 1, w, h0), got, 1) == [], (name, kind, w)
        else:
            want = reflib.end_extension_from_oracle(wj, lp, kind == 3, w, h0)
            bad = [i for i in range(len(wj)) if (want["score"][i], want["qle"][i], want["tle"][i], list(want["cigars"][i])) != (got["score"][i], got["qle"][i], got["tle"][i], list(got["cigars"][i]))]
            assert bad == [] and (got["status"] == 0).all(), (name, kind, w, bad[:5])
