"""SV junctions on the CPU: the hand-made reads of tests/sv_cases.py -- one junction each that junction_geo classes JC_SV -- through split_sv
(lamsa_amd/csrc/hp_fill.h) and the k-mer split mapper (hp_split.h) under the lane emulation.  Per read:

  * the oracle aligns it (status 0, at least one line);
  * the emulated streams equal the oracle's word for word with status 0, through the launches of hp_phase.h and through the one-kernel path;
  * the path counters of the phased run (slots in hp_core.h, named in sv_cases) show exactly one SV junction and the branch the case is named after;
  * the window split_sv hands to the mapper, restated in Python (sv_cases.window_of), gives the same CIGAR from the oracle, the emulation and --
    where oracle/_ref is built -- the reference itself; the k-mer the case is about matches the window positions it claims.

The fuzz batches (300 reads per preset, the five window kinds of tests/test_dp_cpu.py as whole reads) get the same comparisons per read; a read is
dropped only when the oracle does not align it or the emulation does not reach the mapper for it, and at most 5 % may be dropped.  The branches
that sv_cases' docstring lists as unreachable from any whole read keep their counters at 0 over everything run here."""
import numpy as np
import pytest

import reflib
import sv_cases

FUZZ_N, FUZZ_SEED, MAX_DROP = 300, 7, 0.05
# every branch of split_sv, the hash DP and the anchor walk that a whole read can take
BRANCH_SLOTS = [sv_cases.DEL_BI, sv_cases.DEL_MAP, sv_cases.INS_OVL, sv_cases.DUP_OFF, sv_cases.DUP_CUT, sv_cases.MIN_ROUTE, sv_cases.PROMOTED, sv_cases.MINI, sv_cases.MULTI,
                sv_cases.NO_ANCHOR, sv_cases.LONG_INS_OFF, sv_cases.LONG_INS_0] + list(range(sv_cases.L_GLOBAL, sv_cases.NONE_BI + 1))
_done, _fuzz, _three = {}, {}, {}


def _hp_para(lp):
    from lamsa_amd.hp import HpPara
    P = HpPara()
    for n, _ in HpPara._fields_:
        setattr(P, n, getattr(lp, n))
    return P


def _run(key):
    """The case, its parameters, the oracle's streams and the phased run with its counters: made once, shared, never changed."""
    if not _done:
        reflib.build_oracle()
        _done.update({c.key: None for c in sv_cases.cases()})
    if _done[key] is None:
        c = next(c for c in sv_cases.cases() if c.key == key)
        lp = reflib.lo_para(c.read_type, **dict(c.over))
        want = reflib.oracle_streams(c.batch, lp, 1)
        stats = []
        got, st = reflib.emu_streams(c.batch, _hp_para(lp), stats=stats, slab_bytes=64 << 20)
        _done[key] = (c, lp, want, got, int(st[0]), stats)
    return _done[key]


def test_case_list():
    assert [c.key for c in sv_cases.cases()] == sv_cases.CASE_KEYS


@pytest.mark.parametrize("key", sv_cases.CASE_KEYS)
def test_sv_junction(key):
    c, lp, want, got, st, stats = _run(key)
    print(key, c.aim, {i: v for i, v in enumerate(stats) if v and (i in (11, 12, 13, 28, 29, 30) or i >= 64)})
    assert want[0][0] == 0 and want[0][1] >= 1, "the oracle does not align this read: %s" % c.aim
    assert st == 0 and got == want, (c.aim, "phased")
    assert sv_cases.check(stats, c.expect) == [], (c.aim, "(slot, op, expected, counted)")
    assert [stats[s] for s in sv_cases.UNREACHABLE] == [0, 0, 0]
    got, st = reflib.emu_streams(c.batch, _hp_para(lp), phased=False, slab_bytes=64 << 20)
    assert int(st[0]) == 0 and got == want, (c.aim, "one-kernel")


@pytest.mark.parametrize("key", sv_cases.CASE_KEYS)
def test_sv_window_three_ways(key):
    """The window of split_sv restated: the oracle and the emulation agree on it, and it is what the whole read ran (the mapper was called
    exactly when the restated geometry says so, on a window of that many k-mer codes)."""
    c, lp, want, got, st, stats = _run(key)
    win = sv_cases.window_of(c.batch, lp)
    assert (win is not None) == (stats[sv_cases.MAP] == 1), "the restated geometry and the run disagree on whether the mapper is called"
    if win is None:
        return
    gap, tb, start, ref_len, off = win
    assert (off > 0) == (stats[sv_cases.DUP_OFF] == 1)
    assert stats[sv_cases.MAX_CODES] == max(ref_len - lp.hash_len + 1, 0)
    hits = sv_cases.kmer_matches(gap, tb[start:start + ref_len], lp)
    for what, slot, val in c.checks:
        assert (hits[slot] == [val]) if what == "only" else (len(hits[slot]) == val), (what, slot, val, hits[slot])
    kept = [len(h) for h in hits if len(h) <= 50]
    assert stats[sv_cases.MAX_KEPT] == max(kept + [0]) and stats[sv_cases.DROPPED] == sum(len(h) > 50 for h in hits)
    rp = reflib.ref_para(c.read_type, **dict(c.over)) if reflib.ref() is not None else None
    o, r, e = reflib.split_indel_map_three_ways(gap, tb, off, lp, rp, _hp_para(lp), ref_start=start, ref_len=ref_len)
    _three[key] = (o, r)
    assert e[2] == 0 and (e[0], e[1]) == o, "emulation vs oracle"


@pytest.mark.skipif(reflib.ref() is None, reason="compiled reference (oracle/_ref) not present")
@pytest.mark.parametrize("key", sv_cases.CASE_KEYS)
def test_sv_window_reference(key):
    """The oracle against the reference itself on the same windows: inputs the oracle's goldens never held."""
    if key not in _three:
        test_sv_window_three_ways(key)
    if key in _three:
        o, r = _three[key]
        assert r == o, "oracle vs reference"


def _fuzz_run(preset):
    if preset not in _fuzz:
        reflib.build_oracle()
        R, bs = sv_cases.fuzz(preset, FUZZ_N, FUZZ_SEED)
        lp = reflib.lo_para(preset)
        B = sv_cases.concat(bs)
        want = reflib.oracle_streams(B, lp, 4)
        _fuzz[preset] = (bs, B, lp, want)
    return _fuzz[preset]


@pytest.mark.parametrize("preset", ["default", "ont2d"])
def test_sv_fuzz(preset):
    bs, B, lp, want = _fuzz_run(preset)
    P = _hp_para(lp)
    by_oracle = [i for i, w in enumerate(want) if not (w[0] == 0 and w[1] >= 1)]
    assert len(by_oracle) <= MAX_DROP * len(bs), "the generator: the oracle alone leaves %d of %d reads unaligned" % (len(by_oracle), len(bs))
    total = np.zeros(reflib.N_STATS, np.int64)
    dropped, bad = set(by_oracle), []
    for i, b in enumerate(bs):
        if i in dropped:
            continue
        stats = []
        got, st = reflib.emu_streams(b, P, stats=stats, slab_bytes=32 << 20)
        if stats[sv_cases.MAP] == 0:
            dropped.add(i)
            continue
        total += np.array(stats, np.int64)
        if int(st[0]) != 0 or got[0] != want[i]:
            bad.append((i, "phased"))
        elif stats[sv_cases.SV] != 1 or stats[sv_cases.MAP] != 1:
            bad.append((i, "junctions", stats[sv_cases.SV], stats[sv_cases.MAP]))
    print(preset, "dropped", sorted(dropped), {i: int(v) for i, v in enumerate(total) if v and (i in (11, 12, 13, 28, 29, 30) or i >= 64)})
    assert len(dropped) <= MAX_DROP * len(bs), sorted(dropped)
    for phased in (True, False):                            # the whole batch at once, both routes
        got, st = reflib.emu_streams(B, P, phased=phased)
        bad += [(i, "batch", phased) for i in range(len(bs)) if i not in dropped and (int(st[i]) != 0 or got[i] != want[i])]
    assert bad == []
    assert [int(total[s]) for s in sv_cases.UNREACHABLE] == [0, 0, 0]
    _fuzz[preset + "/total"] = total


def test_every_branch_is_taken():
    """Every branch counter is non-zero over the hand-made reads or the fuzz, and the branches no whole read reaches stay at 0 over both."""
    total = np.zeros(reflib.N_STATS, np.int64)
    for key in sv_cases.CASE_KEYS:
        total += np.array(_run(key)[5], np.int64)
    for preset in ("default", "ont2d"):
        if preset + "/total" not in _fuzz:
            test_sv_fuzz(preset)
        total += _fuzz[preset + "/total"]
    assert [s for s in BRANCH_SLOTS if total[s] == 0] == []
    expected = {slot for c in sv_cases.cases() for (slot, op, val) in c.expect if op in (">", ">=") or (op == "==" and val > 0)}
    assert [s for s in sorted(expected) if total[s] == 0] == []
    assert [int(total[s]) for s in sv_cases.UNREACHABLE] == [0, 0, 0]
