"""The job sets of test_extband_cpu.py on the MI355X: lamsa_hp_dp_batch kinds 1 and 2 (ksw_extend, ksw_bi_extend) and the wave-job kinds
8 .. 11 (a junction, a seed gap, a head and a tail extension as k_filldp_wave runs them) against the oracle, bit for bit."""
import pytest

import extband_jobs as xj
import goldenlib
import reflib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles():
    from lamsa_amd import hp
    hs = {rt: hp.LamsaHp(hp.make_para(rt)) for rt in xj.PRESETS}
    yield hs
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("preset", xj.PRESETS)
def test_hip_extension_variants_match_oracle(handles, preset):
    lp = reflib.lo_para(preset)
    jobs = xj.make_jobs(9000 + len(preset))
    for w in xj.WS:
        for h0 in (1, 50):
            got = handles[preset].dp_batch(jobs, 1, w, h0)
            assert goldenlib.same_dp(reflib.oracle_dp(jobs, lp, 1, w, h0), got, 1) == [], (preset, w, h0)
    for w, over in ((100, 0), (200, 1), (lp.band_w, 0)):
        h0 = xj.h0_near_limit(lp, jobs, over)
        got = handles[preset].dp_batch(jobs, 1, w, h0)
        assert goldenlib.same_dp(reflib.oracle_dp(jobs, lp, 1, w, h0), got, 1) == [], (preset, w, "h0 at the limit", over)
    for h0 in (100, 7):
        got = handles[preset].dp_batch(jobs, 2, 0, h0)
        assert goldenlib.same_dp(reflib.oracle_dp(jobs, lp, 2, 0, h0), got, 2) == [], (preset, h0)


@pytest.mark.parametrize("preset", xj.PRESETS)
def test_hip_wave_job_kinds_match_oracle(handles, preset):
    lp = reflib.lo_para(preset)
    jobs = [(q, t) for q, t in xj.make_jobs(9200 + len(preset)) if t.max() < 4]
    for h0 in (100, 7):
        got = handles[preset].dp_batch(jobs, 8, 0, h0)
        assert goldenlib.same_dp(reflib.oracle_dp(jobs, lp, 2, 0, h0), got, 2) == [], (preset, h0)
    for w in (lp.band_w, 7):
        got = handles[preset].dp_batch(jobs, 9, w, 0)
        assert goldenlib.same_dp(reflib.oracle_dp(jobs, lp, 0, w, 0), got, 0) == [], (preset, w)
    for head in (True, False):
        for w, h0 in ((lp.band_w, 50), (54, 9)):
            want = reflib.end_extension_from_oracle(jobs, lp, head, w, h0)
            got = handles[preset].dp_batch(jobs, 10 if head else 11, w, h0)
            bad = [i for i in range(len(jobs)) if (want["score"][i], want["qle"][i], want["tle"][i], list(want["cigars"][i])) != (got["score"][i], got["qle"][i], got["tle"][i], list(got["cigars"][i]))]
            assert bad == [] and (got["status"] == 0).all(), (preset, head, w, h0, bad[:5])
