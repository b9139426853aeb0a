"""Branch tracking with the read's largest cluster in LDS (lamsa_amd/csrc/hp_track.h) on the CPU: the device sources under the lane emulation
against the oracle, word for word, with the LDS size of each of the three shapes of k_chain1 (2432 / 3392 / 5120 words per wave), through the
launches of hp_phase.h and through the one-kernel path.  The reads are hand-made (tests/track_cases.py): the image at its capacity and one hit
beyond, a second and third locus whose tracks run through HBM between resident ones, the tie rules of get_max_son, the negative edges of the
walk and of cut_branch, a chain of more than 64 nodes, '-' strand clusters, one node with three sons (three reads: the kept son last, in the
middle, and two tie rules in one list), a read whose first pass is all_min and one whose resident cluster holds MULTI hits, a largest cluster
that cannot be packed.  Per read and shape:

  * the oracle aligns the read (status 0, at least one line);
  * the emulated streams equal the oracle's with status 0;
  * the path counters of the phased run (hp_core.h, slots 49 - 63) show that the route the case is named after was taken on the image;
  * no phase wrote into the guard words behind its LDS (reflib.emu_streams asserts it).

And 16 simulated 10-kbp ONT reads: every one with a resident cluster, all equal to the oracle."""
import pytest

import crafted
import reflib
import track_cases

_cache = {}


def _hp_para(lp):
    from lamsa_amd.hp import HpPara
    P = HpPara()
    for n, _ in HpPara._fields_:
        setattr(P, n, getattr(lp, n))
    return P


def _case(W, key):
    """The case, its parameters and the oracle's streams: made once per shape, shared by the tests, never changed."""
    if W not in _cache:
        reflib.build_oracle()
        cs = {}
        for c in track_cases.cases(W):
            lp = reflib.lo_para(c.read_type)
            cs[c.key] = (c, lp, reflib.oracle_streams(c.batch, lp, 1))
        _cache[W] = cs
    return _cache[W][key]


@pytest.mark.parametrize("key", track_cases.CASE_KEYS)
@pytest.mark.parametrize("W", track_cases.SHAPES)
def test_tracking_on_the_image(W, key):
    c, lp, want = _case(W, key)
    assert want[0][0] == 0 and want[0][1] >= 1, "the oracle does not align this read: %s" % c.aim
    stats = []
    got, st = reflib.emu_streams(c.batch, _hp_para(lp), chain_lds_words=W, stats=stats)
    print(W, key, c.aim, "seed_out", c.seed_out, "H", c.H, {i: v for i, v in enumerate(stats) if v and i >= 48})
    assert int(st[0]) == 0 and got == want, (c.aim, "phased")
    assert crafted.check(stats, c.expect) == [], (c.aim, "(slot, op, expected, counted)")
    got, st = reflib.emu_streams(c.batch, _hp_para(lp), chain_lds_words=W, phased=False)
    assert int(st[0]) == 0 and got == want, (c.aim, "one-kernel")


@pytest.mark.parametrize("W", track_cases.SHAPES)
def test_an_image_at_capacity_ends_at_the_last_word(W):
    """With 52 seed slots the leaf bits take two words and six words per hit fill the rest of every shape exactly: the image of cap hits ends at
    word W - 1.  With the guards of the chaining phases moved onto that word, the read of cap hits damages them in one phase call more than the
    read of cap - 1 hits (whatever else of the chaining reaches that word does so for both); the streams do not change."""
    cap = track_cases.image_cap(W, 52)
    assert 2 + 6 * cap == W
    c, lp, want = _case(W, "image-cap")
    A = crafted.sim_ref("a")
    below = track_cases.capacity_read(A, cap - 1)
    hits = []
    for batch, w in ((c.batch, want), (below, reflib.oracle_streams(below, lp, 1))):
        guard = []
        got, st = reflib.emu_streams(batch, _hp_para(lp), chain_lds_words=W, lds_shrink=1, guard=guard)
        assert got == w and int(st[0]) == 0
        hits.append(guard[0])
    assert hits[0] == hits[1] + 1, hits


def test_simulated_ont_reads_all_have_a_resident_cluster():
    ref, B = track_cases.sim_ont_reads(16)
    lp = reflib.lo_para("ont2d")
    reflib.build_oracle()
    want = reflib.oracle_streams(B, lp)
    stats = []
    got, st = reflib.emu_streams(B, _hp_para(lp), stats=stats)
    print({i: v for i, v in enumerate(stats) if v and i >= 48})
    assert (st == 0).all() and got == want
    assert stats[track_cases.RESIDENT] == B.n_reads, "reads with a resident cluster"
    assert stats[track_cases.ON_IMAGE] > stats[track_cases.ON_HBM] > 0 and stats[track_cases.STEPS] > 0
