"""The two stages of the lane DP (phase_filldp, lamsa_amd/csrc/hp_phase.h) without a GPU: the job sets of tests/lanedp_jobs.py through the device sources
under the CPU lane emulation (tests/emu/emu_lanedp.cpp lists them into the queues and walks the queues as the drivers of emu_api.cpp do), against
reflib.oracle_dp (kind 2, ksw_bi_extend(100, 100), for a junction job and kind 0, ksw_global2(band_w), for a seed-gap job), word for word.

  * the labels of the pools are the exits the emulation takes, and every set has the exits it is named for (at least 4 jobs each where the set is
    large enough to be named for them: see MEANT);
  * two stages and one stage give the same CIGARs and charge every job the same cells;
  * the counters show that the second stage ran exactly the hard jobs and that none was left to the fill;
  * a hard queue made too small on purpose leaves its excess to the fill: those jobs are not published, the others are the oracle's, and a small ONT
    batch through the whole phased path (where the fill then runs them) still equals the oracle;
  * the hand-made reads of tests/edge_cases.py and 16 simulated 10-kbp ONT reads through the phased path equal the oracle, with hard jobs seen."""
import contextlib

import numpy as np
import pytest

import crafted
import edge_cases
import lanedp_jobs as LJ
import reflib
import track_cases

_cache = {}


def _hp_para(lp):
    from lamsa_amd.hp import HpPara
    P = HpPara()
    for n, _ in HpPara._fields_:
        setattr(P, n, getattr(lp, n))
    return P


def _set(preset, size, mix):
    """The set, its parameters and the oracle's CIGARs: made once, shared by the tests, never changed."""
    key = (preset, size, mix)
    if key not in _cache:
        reflib.build_oracle()
        lp = reflib.lo_para(preset)
        jobs, types, exits = LJ.job_set(preset, size, mix)
        want = reflib.oracle_dp(jobs, lp, np.where(types == 1, reflib.KIND_BI, reflib.KIND_GLOBAL), lp.band_w, 100)["cigars"]
        _cache[key] = (jobs, types, exits, lp, want)
    return _cache[key]


def MEANT(size, mix):
    """The exits a set is named for (it must hold at least 4 jobs of each)."""
    if size < 63:
        return ()
    return {"easy": (0,), "one-last": (0,), "hard": (1, 2, 3, 4, 5), "mixed": (0, 1, 2, 3, 4, 5) if size == 200 else (0,)}[mix]


@pytest.mark.parametrize("preset", LJ.PRESETS)
def test_pool_labels_are_the_exits_of_the_emulation(preset):
    got = LJ.emu_exits(LJ.pool(preset), _hp_para(reflib.lo_para(preset)))
    assert got.tolist() == LJ.labels(preset).tolist()
    print(preset, dict(zip(LJ.EXIT_NAMES, np.bincount(got, minlength=6).tolist())))
    assert (np.bincount(got, minlength=6) >= 20).all(), "every exit in the pool"


@pytest.mark.parametrize("preset,size,mix", LJ.set_ids(), ids=lambda v: str(v))
def test_sets_two_stages_against_one_and_the_oracle(preset, size, mix):
    jobs, types, exits, lp, want = _set(preset, size, mix)
    assert len(jobs) == size and all(1 <= len(q) <= 64 and len(t) <= 160 for q, t in jobs)
    P = _hp_para(lp)
    two = LJ.emu_stages(jobs, types, P, stages=True)
    one = LJ.emu_stages(jobs, types, P, stages=False)
    n_hard = int((exits > 0).sum())
    by_exit = np.bincount(exits[exits >= 0], minlength=6)
    st, so = two["stats"], one["stats"]
    print(preset, size, mix, "hard", n_hard, "exits", by_exit.tolist(), st)
    # the set is what its name says
    assert n_hard == {"easy": 0, "one-last": 1, "hard": size}.get(mix, n_hard) and (mix != "mixed" or (n_hard % 64 != 0 and n_hard > 0))
    for e in MEANT(size, mix):
        assert st[LJ.ST_EXIT0 + e] >= 4, (LJ.EXIT_NAMES[e], st)
    if mix == "one-last":                                # one queue, the hard job in the last lane of the first group
        assert (types == 1).all() and all(len(q) >= 49 for q, _ in jobs) and int(np.flatnonzero(exits > 0)[0]) == min(size, 64) - 1
    # results: both ways the oracle's, every job published, the same cells
    assert (two["has"] == 1).all() and (one["has"] == 1).all()
    assert two["cigars"] == want and one["cigars"] == want
    assert two["cells"].tolist() == one["cells"].tolist() and (two["cells"][[len(t) > 0 for _, t in jobs]] > 0).all()
    # counters: the exits, and the second stage ran exactly the hard jobs
    for s in (st, so):
        assert s[LJ.ST_T1] == int((types == 1).sum()) and s[LJ.ST_T2] == int((types == 2).sum())
        assert [s[LJ.ST_EXIT0 + e] for e in range(6)] == by_exit.tolist()
    assert st[LJ.ST_DEFERRED] == n_hard and st[LJ.ST_STAGE2] == n_hard and st[LJ.ST_HARD_FULL] == 0
    assert two["hard"].tolist() == (exits > 0).astype(int).tolist()
    assert so[LJ.ST_DEFERRED] == 0 and so[LJ.ST_STAGE2] == 0 and not one["hard"].any()


@pytest.mark.parametrize("preset", LJ.PRESETS)
def test_a_full_hard_queue_leaves_its_jobs_to_the_fill(preset):
    jobs, types, exits, lp, want = _set(preset, 200, "mixed")
    cap = 3                                              # per hard queue (one per query class): 70 hard jobs do not fit
    got = LJ.emu_stages(jobs, types, _hp_para(lp), stages=True, hard_cap=cap)
    st = got["stats"]
    left = int((got["has"] == 0).sum())
    print(preset, "left to the fill", left, st)
    assert st[LJ.ST_DEFERRED] == 70 and left > 0 and st[LJ.ST_HARD_FULL] == left and st[LJ.ST_STAGE2] == 70 - left and st[LJ.ST_STAGE2] <= 8 * cap
    assert (exits[got["has"] == 0] > 0).all(), "only hard jobs are left"
    assert [c for c, h in zip(got["cigars"], got["has"]) if h] == [c for c, h in zip(want, got["has"]) if h]


@contextlib.contextmanager
def _phased_with_hard_cap(cap):
    """reflib.emu_streams on the library of tests/emu/emu_lanedp.cpp (all of emu_api.cpp plus the capacity of a hard queue)."""
    E = LJ.emu()
    keep = reflib._emu
    reflib._emu = E
    E.emu_set_lj_hard_cap(int(cap))
    try:
        yield
    finally:
        E.emu_set_lj_hard_cap(0)
        reflib._emu = keep


def test_hand_made_reads_through_the_phased_path():
    reflib.build_oracle()
    cs_all = edge_cases.cases(edge_cases.SHAPES[0])
    assert len(cs_all) == 13
    hard = 0
    for (read_type, over, ref_key), cs in sorted(crafted.groups(cs_all).items()):
        batch = crafted.concat([c.batch for c in cs])
        lp = reflib.lo_para(read_type)
        want = reflib.oracle_streams(batch, lp, 4)
        stats = []
        got, st = reflib.emu_streams(batch, _hp_para(lp), stats=stats)
        assert (st == 0).all() and got == want, [c.key for c in cs]
        assert stats[LJ.ST_DEFERRED] == stats[LJ.ST_STAGE2] and stats[LJ.ST_HARD_FULL] == 0
        hard += stats[LJ.ST_STAGE2]
    print("hard jobs of the hand-made reads:", hard)


def test_simulated_ont_reads_through_the_phased_path_with_hard_jobs():
    ref, B = track_cases.sim_ont_reads(16)
    lp = reflib.lo_para("ont2d")
    reflib.build_oracle()
    want = reflib.oracle_streams(B, lp)
    stats = []
    got, st = reflib.emu_streams(B, _hp_para(lp), stats=stats)
    print({i: stats[i] for i in range(97, 108)})
    assert (st == 0).all() and got == want
    assert stats[LJ.ST_STAGE2] >= 1 and stats[LJ.ST_DEFERRED] == stats[LJ.ST_STAGE2] and stats[LJ.ST_HARD_FULL] == 0
    assert stats[LJ.ST_EXIT0] + stats[LJ.ST_DEFERRED] == stats[LJ.ST_T1], "a junction job ends in the first stage or goes to the second"
    # the same with hard queues of one entry: the fill runs what they turn away
    with _phased_with_hard_cap(1):
        stats2 = []
        got2, st2 = reflib.emu_streams(B, _hp_para(lp), stats=stats2)
    print({i: stats2[i] for i in range(97, 108)})
    assert (st2 == 0).all() and got2 == want
    assert stats2[LJ.ST_HARD_FULL] >= 1 and stats2[LJ.ST_STAGE2] + stats2[LJ.ST_HARD_FULL] == stats2[LJ.ST_DEFERRED] == stats[LJ.ST_DEFERRED]
