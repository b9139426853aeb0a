"""The capacity edges of the chaining kernels on the CPU: hand-made reads (tests/crafted.py) that meet a capacity exactly, one below and
one above, run through the device sources under the lane emulation with the LDS size of each of the three shapes of k_chain1 / k_chain2
(2432 / 3392 / 5120 words per wave) and that shape's real capacities -- no lowered cap.  Per read and shape:

  * the oracle aligns the read (status 0, at least one line): a read it leaves alone tests nothing;
  * the emulated streams equal the oracle's word for word with status 0, through the launches of hp_phase.h and through the one-kernel path
    (whose wave owns HP_BOTH_LDS_WORDS whatever the shape: the read is the same, the capacities are those of 2432 words);
  * the path counters of the phased run (HP_STAT / HP_STAT_ADD / HP_STAT_MAX, slots in hp_core.h) show the route and the size the case is
    named after -- crafted.cases() states them per case;
  * no phase wrote into the guard words behind its LDS (reflib.emu_streams asserts it for every test of the CPU suite)."""
import pytest

import crafted
import reflib

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
        for c in crafted.cases(W):
            lp = reflib.lo_para(c.read_type, **dict(c.over))
            cs[c.key] = (c, lp, reflib.oracle_streams(c.batch, lp, 1))
        _cache[W] = cs
    return _cache[W][key]


@pytest.mark.parametrize("key", crafted.CASE_KEYS)
@pytest.mark.parametrize("W", crafted.SHAPES)
def test_capacity_edge(W, key):
    c, lp, want = _case(W, key)
    assert want[0][0] == 0 and want[0][1] >= 1, "the oracle does not align this read: %s" % c.aim
    stats = []
    got, st = reflib.emu_streams(c.batch, _hp_para(lp), chain_lds_words=W, stats=stats)
    print(W, key, c.aim, "seed_out", c.seed_out, "H", c.H, {i: v for i, v in enumerate(stats) if v})
    assert int(st[0]) == 0 and got == want, (c.aim, "phased")
    assert crafted.check(stats, c.expect) == [], (c.aim, "(slot, op, expected, counted)")
    got, st = reflib.emu_streams(c.batch, _hp_para(lp), chain_lds_words=W, phased=False)
    assert int(st[0]) == 0 and got == want, (c.aim, "one-kernel")


@pytest.mark.parametrize("W", crafted.SHAPES)
def test_a_cluster_at_capacity_uses_its_lds_to_the_last_word(W):
    """The guard words themselves, and that the cluster reads are AT the edge.  A cluster of cap = W / 5 hits is five arrays of cap words
    (hp_cluster.h: cl_lds), so its last record ends at word 5 * cap - 1.  With the guards of the chaining phases moved inside the LDS the
    phase owns, onto that very word, the read of cap hits damages them in one phase call more than the read of cap - 1 hits, which is the same
    read but for one hit (whatever else of the chaining uses its LDS that far does so for both); the streams do not change."""
    cap = W // 5
    hits = {}
    for key in ("cluster-cap", "cluster-cap-1"):
        c, lp, want = _case(W, key)
        guard = []
        got, st = reflib.emu_streams(c.batch, _hp_para(lp), chain_lds_words=W, lds_shrink=W - 5 * cap + 1, guard=guard)
        assert got == want and int(st[0]) == 0, key
        hits[key] = guard[0]
    assert hits["cluster-cap"] == hits["cluster-cap-1"] + 1, hits
