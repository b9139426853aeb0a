"""Job sets of the band-extension tests (test_extband_cpu.py, test_extband_gpu.py): query lengths on both sides of every edge at which
ksw_extend (lamsa_amd/csrc/hp_ksw.h) changes routine, register sets or between the fixed and the sliding window, and a Python restatement
of that routing, so that a test can say which variant a job must have taken."""
import numpy as np

import dpjobs

# 62 / 63: one int32 set -> the window routine; 125 / 126: the last query a window of one set holds whole (qlen + 3 <= 128); 253 / 254 and
# 509 / 510: the same for two and four sets; 127, 255, 511: one beyond HP_PK_QMAX; 700 and 3 000: the window slides for good
QLENS = (62, 63, 125, 126, 127, 253, 254, 255, 509, 510, 511, 700, 3000)
WS = (3, 10, 53, 54, 100, 200)               # 53 / 54: the widest band one set slides under (2w + 3 + 18 <= 128) and the first that needs two
ERRS = (0.01, 0.12, 0.30)                    # 1 %: nothing stops the rows; 12 %: the bench's reads; 30 %: z-drop, rows without a maximum, a band shrinking from both sides
PRESETS = ("default", "pacbio", "ont2d")     # band_w 10 / 200 / 100


def make_jobs(seed):
    """(query, target) pairs: every length of QLENS exactly, at every error rate, with a target shorter than, about as long as and far longer
    than the query (|qlen - tlen| + 3 beyond every preset's band), and the same again with runs of N in both sequences."""
    rng = np.random.default_rng(seed)
    jobs = []
    for ql in QLENS:
        for err in ERRS:
            t0 = rng.integers(0, 4, size=2 * ql + 450, dtype=np.uint8)
            q = dpjobs.mutate(rng, t0, err / 3, err / 3, err / 3)[:ql]
            assert len(q) == ql
            for tl in (int(0.6 * ql), ql + int(rng.integers(-2, 3)), ql + 400):
                jobs.append((q.copy(), t0[:tl].copy()))
            qn, tn = q.copy(), t0[:ql + 5].copy()
            a, b = int(rng.integers(0, ql - 12)), int(rng.integers(0, ql - 12))
            qn[a:a + 10] = 4
            tn[b:b + 7] = 4
            jobs.append((qn, tn))
    return jobs


def hp_para(lp):
    from lamsa_amd.hp import HpPara
    P = HpPara()
    for n, _ in HpPara._fields_:
        setattr(P, n, getattr(lp, n))
    return P


def _trunc_div(a, b):
    return int(float(a) / float(b) + 1.0)     # (int)((double)a / b + 1.), as ksw_extend narrows w (src/ksw.c:696-704)


def band_class(lp, qlen, w, h0):
    """(NS, fixed) of the window routine a ksw_extend(qlen, w, h0) call runs, or None when it takes another routine -- hp_ksw.h: ksw_extend,
    pkb_sets_q, pkb_extend_ok."""
    if h0 <= 0 or qlen <= 62:
        return None
    mw = max(lp.match, -lp.mis, 0)              # the largest entry of the score matrix, as the narrowing of w sees it
    mx = max(lp.match, lp.mis)                  # the largest step of a score in either direction, as pkb_extend_ok bounds it
    w = min(w, max(_trunc_div(qlen * mw + lp.end_bonus - lp.ins_ext_o, lp.ins_ext_e), 1), max(_trunc_div(qlen * mw + lp.end_bonus - lp.del_ext_o, lp.del_ext_e), 1))
    ns = next((n for n in (1, 2, 4) if 2 * w + 3 + 18 * n <= 128 * n or qlen + 3 <= 128 * n), 0)
    pen = max(lp.ins_ext_o, lp.del_ext_o) + max(lp.ins_ext_e, lp.del_ext_e)
    ext = max(lp.ins_ext_e, lp.del_ext_e)
    ok = ns > 0 and 0 < mx < 256 and 0 <= pen < 4000 and min(lp.ins_ext_e, lp.del_ext_e, lp.ins_ext_o, lp.del_ext_o) >= 0 and \
        h0 + qlen * mx < 23000 and (128 * ns + 2) * ext < 8000 and qlen + 128 * ns < 32000
    return (ns, qlen + 3 <= 128 * ns) if ok else None


def h0_near_limit(lp, jobs, over=0):
    """per job: the largest h0 pkb_extend_ok lets through (h0 + qlen * mx < 23 000), plus `over`"""
    mx = max(lp.match, lp.mis)
    return np.array([22999 - len(q) * mx + over for q, _ in jobs], np.int32)


# what the read path's own band (w = band_w, as head_fix / tail_fix call the extension) can reach, by pkb_sets_q:
#   band  10: 2w + 3 + 18 = 41 <= 128, one set whatever the query -- fixed up to 125 bases, sliding beyond; two and four sets never
#   band 100: 2w + 3 + 18 n = 221 > 128, 239 <= 256: one set only while it holds the whole query (fixed), two sets fixed up to 253 bases and sliding beyond;
#             one set sliding and four sets never
#   band 200: 421 > 128, 439 > 256, 475 <= 512: one, two and four sets while they hold the whole query (fixed), four sets sliding beyond 509 bases; one and
#             two sets sliding never
OWN_BAND_CLASSES = {
    "default": {(1, True), (1, False)},
    "ont2d": {(1, True), (2, True), (2, False)},
    "pacbio": {(1, True), (2, True), (4, True), (4, False)},
}
ALL_CLASSES = {(ns, fx) for ns in (1, 2, 4) for fx in (True, False)}
