"""Job sets of the re-based window tests (test_rebase_cpu.py, test_rebase_gpu.py): the sliding case of ksw_extend_band (lamsa_amd/csrc/hp_ksw.h)
keeps its window in plain column order and shifts it left by whole lanes when the band's right edge nears its end (a re-base).  The shapes are
the smallest at which a re-base can go wrong: queries of 130 to 900 bases, targets up to 400 bases longer, bands at both ends of what each
number of register sets (NS) slides under.

A re-base happens in the row whose end + 3 exceeds base + WN (WN = 128 NS columns, LC = 2 NS per lane) and frees s = (beg - base) / LC lanes.
With a full band (end - beg = 2w + 1) that is (WN - 2w - 3) / LC lanes: the fewest, 9, under the widest band a set count slides under
(2w + 3 + 9 LC <= WN: w = 53, 108, 218), the most under the narrowest (w = 3: 59 of 64 lanes; 54 and 109, the first bands of two and four
sets: 36).  Re-bases only happen while `end` still grows, so a job sees (qlen - WN) / (s LC) of them.

Run as a program it is the child process of test_rebase_gpu.py:    python rebase_jobs.py NAME OUT.npz"""
import os
import sys
import time

import numpy as np

import dpjobs
import extband_jobs as xj

QLENS = (130, 170, 260, 340, 400, 520, 560, 700, 900)
ERRS = (0.0, 0.12, 0.30)      # 0 %: the band stays full; 12 %: the bench's reads; 30 %: the band shrinks from the left, z-drop and empty rows after a re-base
# w -> NS it slides under (pkb_sets_q's first clause; the query must not fit the window: qlen + 3 > 128 NS)
W_SETS = {3: 1, 53: 1, 54: 2, 108: 2, 109: 4, 218: 4}
W_LIMIT = {1: 53, 2: 108, 4: 218}          # the widest band of each NS: the fewest lanes freed
W_NARROW = {1: 3, 2: 54, 4: 109}           # the narrowest: the most
# parameter sets: the three presets, and per NS the largest insertion extension penalty pkb_extend_ok lets through ((128 NS + 2) * ext < 8 000:
# 61, 31, 15 -- one more fails), on scores large enough that ksw_extend's narrowing of w leaves the band alone from 340 query bases on
_BIG = dict(match=10, mis=20, ins_ext_o=5, del_ext_o=5, del_ext_e=3, zdrop=400)
PARAMS = {
    "default": ("default", {}), "pacbio": ("pacbio", {}), "ont2d": ("ont2d", {}),
    "ext61": ("ont2d", dict(_BIG, ins_ext_e=61)), "ext31": ("ont2d", dict(_BIG, ins_ext_e=31)), "ext15": ("ont2d", dict(_BIG, ins_ext_e=15)),
}
PRESETS = ("default", "pacbio", "ont2d")
EXT_NS = {"ext61": 1, "ext31": 2, "ext15": 4}
SEEDS = {"default": 7111, "pacbio": 7102, "ont2d": 7103, "ext61": 7104, "ext31": 7105, "ext15": 7106}


def lo_para(name):
    import reflib
    rt, over = PARAMS[name]
    lp = reflib.lo_para(rt, **over)
    for k, v in over.items():
        assert getattr(lp, k) == v, (name, k)
    return lp


def w_eff(lp, qlen, w):
    """the band ksw_extend really runs (src/ksw.c:696-704)"""
    mw = max(lp.match, -lp.mis, 0)
    return min(w, max(xj._trunc_div(qlen * mw + lp.end_bonus - lp.ins_ext_o, lp.ins_ext_e), 1), max(xj._trunc_div(qlen * mw + lp.end_bonus - lp.del_ext_o, lp.del_ext_e), 1))


def slides(lp, qlen, w, h0):
    """NS when the job takes the sliding window with the band it was given, else 0"""
    c = xj.band_class(lp, qlen, w, h0)
    return c[0] if c is not None and not c[1] and w_eff(lp, qlen, w) == w and W_SETS.get(w) == c[0] else 0


def full_band_lanes(ns, w):
    return (128 * ns - 2 * w - 3) // (2 * ns)


def indel_query(rng, t, period):
    """t with a one-base deletion and a one-base insertion in turn every `period` bases: a traceback with gaps on the rows of every re-base"""
    out, k = [], 0
    for i, b in enumerate(t):
        if i and i % period == 0:
            k += 1
            if k & 1:
                continue
            out.append((b + 1) & 3)
        out.append(b)
    return np.array(out, np.uint8)


def make_jobs(seed):
    """(query, target) pairs: every length of QLENS at every error rate with a target 400 bases longer (the query ends inside a re-based window and
    the rows go on: end == qlen, base > 0) and one about as long; the same with runs of N -- in the query behind column 128 and in its last lanes,
    which re-bases load, and in the target; and per length one query with a gap every 23 bases."""
    rng = np.random.default_rng(seed)
    jobs = []
    for ql in QLENS:
        for err in ERRS:
            t0 = rng.integers(0, 4, size=2 * ql + 450, dtype=np.uint8)
            q = dpjobs.mutate(rng, t0, err / 3, err / 3, err / 3)[:ql] if err else t0[:ql].copy()
            assert len(q) == ql
            jobs.append((q.copy(), t0[:ql + 400].copy()))
            jobs.append((q.copy(), t0[:ql + int(rng.integers(-2, 3))].copy()))
            qn, tn = q.copy(), t0[:ql + 200].copy()
            for a in (min(131, ql - 40), ql - 30):
                qn[a:a + 10] = 4
            b = int(rng.integers(0, ql - 12))
            tn[b:b + 7] = 4
            jobs.append((qn, tn))
        t0 = rng.integers(0, 4, size=ql + 450, dtype=np.uint8)
        jobs.append((indel_query(rng, t0, 23)[:ql].copy(), t0[:ql + 300].copy()))
    return jobs


def runs(name, lp, jobs):
    """what both tests run over a job set: (kind, w, h0) with kind 1 = ksw_extend, 3 / 4 = a line's head / tail extension as a wave job (dp_batch kinds
    10 / 11).  The presets take every band at h0 = 50, h0 at the int16 limit and one beyond it; a penalty set takes the two bands of its NS."""
    out = []
    if name in PRESETS:
        for w in sorted(W_SETS):
            out.append((1, w, 50))
        out.append((1, 108, xj.h0_near_limit(lp, jobs)))
        out.append((1, 218, xj.h0_near_limit(lp, jobs, over=1)))          # one beyond the int16 limit: falls back to the int32 routines
        for kind in (3, 4):
            out += [(kind, 53, 50), (kind, 218, 9)]
    else:
        ns = EXT_NS[name]
        out += [(1, W_LIMIT[ns], 50), (1, W_NARROW[ns], 50), (1, W_LIMIT[ns], xj.h0_near_limit(lp, jobs)), (3, W_LIMIT[ns], 50), (4, W_LIMIT[ns], 50)]
    return out


def wave_jobs(jobs):
    return [(q, t) for q, t in jobs if t.max() < 4]          # (the packed reference has no N: wave jobs stage their target from it)


def flat(cigars):
    ln = np.array([len(c) for c in cigars], np.int64)
    return np.array([x for c in cigars for x in c], np.int64), ln


def unflat(words, ln):
    off = np.concatenate([[0], np.cumsum(ln)])
    return [words[off[i]:off[i + 1]].tolist() for i in range(len(ln))]


def child(name, dst):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from lamsa_amd import hp
    lp = lo_para(name)
    jobs = make_jobs(SEEDS[name])
    h = hp.LamsaHp(xj.hp_para(lp))
    out = {}
    t0 = time.time()
    try:
        for k, (kind, w, h0) in enumerate(runs(name, lp, jobs)):
            js = jobs if kind == 1 else wave_jobs(jobs)
            got = h.dp_batch(js, {1: 1, 3: 10, 4: 11}[kind], w, h0)
            for f in ("score", "qle", "tle", "status"):
                out["r%d_%s" % (k, f)] = np.asarray(got[f], np.int64)
            out["r%d_cig" % k], out["r%d_cn" % k] = flat(got["cigars"])
    finally:
        h.close()
    out["seconds"] = np.array([time.time() - t0])
    np.savez(dst, **out)


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
