"""Seeded job sets for the two stages of the lane DP (phase_filldp, lamsa_amd/csrc/hp_phase.h): junction jobs (type 1, ksw_bi_extend(100, 100)) and
seed-gap jobs (type 2, ksw_global2(band_w)) with queries of 1 .. 64 and targets of up to 160 bases, for the three presets.

A pool per preset is made from one seed by the recipes below.  How ksw_bi_extend ends each pool job -- its EXIT, LJ_X_* of hp_lanedp.h -- is kept
here as a string of digits (LABELS): 0 finished after the left extension (an easy job: one DP pass), 1 global after left, 2 finished after the right
extension, 3 global after right, 4 sw_mid_fix with S-H, 5 sw_mid_fix with global (1 .. 5: hard jobs, the second stage runs them).  The sets are cut
from the pool by these labels alone, so the CPU and the GPU tests see the same sets without running anything; tests/test_lanedp_stages_cpu.py checks the
labels against the emulation (emu_lane_exits) and every set against the counters of the run.

Recipes (a pool holds the same number of each, in turn):
  exact      the query is a copy of the target
  err12      ~12 % substitutions and indels          err30   ~30 %
  half       the query's second half is unrelated sequence
  mid-short  an unrelated middle of a few bases in both (sw_mid_fix: global)          mid-long   a long unrelated middle in the target only (sw_mid_fix: S-H)
  t-short    a target much shorter than the query    t-long  a target much longer than the query (both leave the diagonal: the bi_near_diag fallbacks)
Sets: 1, 63, 64, 65 and 200 jobs with no hard job ("easy"), exactly one hard job in the last lane of a group ("one-last"), only hard jobs ("hard"), and a number
of hard jobs that is no multiple of 64 ("mixed").  The jobs of a "one-last" set share one queue (type 1, queries of 49 .. 64 bases), so that the set's order is
the queue's and the hard job sits in lane 63 of the first group (the last job of a set of fewer than 64)."""
import ctypes as C
import os
import subprocess

import numpy as np

import reflib

PRESETS = ("default", "ont2d", "pacbio")
SIZES = (1, 63, 64, 65, 200)
MIXES = ("easy", "one-last", "hard", "mixed")
RECIPES = ("exact", "err12", "err30", "half", "mid-short", "mid-long", "t-short", "t-long")
POOL_SEED = {"default": 20251, "ont2d": 20252, "pacbio": 20253}
POOL_N = 1600
EXIT_NAMES = ("left", "left-global", "right", "right-global", "mid-S-H", "mid-global")
# path counters of the emulation (hp_core.h)
ST_T1, ST_T2, ST_EXIT0, ST_DEFERRED, ST_STAGE2, ST_HARD_FULL = 97, 98, 99, 105, 106, 107
HP_LJ_CIG = 160 + 256 + 8


def _mutate(rng, t, e):
    out = []
    for b in t:
        r = rng.random()
        if r < e / 3:
            continue
        if r < 2 * e / 3:
            b = (int(b) + int(rng.integers(1, 4))) & 3
        out.append(b)
        if rng.random() < e / 3:
            out.append(int(rng.integers(0, 4)))
    return np.array(out[:64] if out else [int(rng.integers(0, 4))], dtype=np.uint8)


def _job(rng, recipe):
    r4 = lambda n: rng.integers(0, 4, size=int(n), dtype=np.uint8)
    ql = int(rng.integers(49, 65)) if rng.random() < 0.5 else int(rng.integers(1, 65))      # half of the pool in the longest query class
    if recipe == "exact":
        t = r4(ql); q = t.copy()
    elif recipe in ("err12", "err30"):
        t = r4(ql); q = _mutate(rng, t, 0.12 if recipe == "err12" else 0.30)
    elif recipe == "half":
        t = r4(ql); q = np.concatenate([t[:ql // 2], r4(ql - ql // 2)])
    elif recipe == "mid-short":
        a = max(1, ql // 3); m = int(rng.integers(2, 12))
        head, tail = r4(a), r4(max(1, ql - a - m))
        q = np.concatenate([head, r4(m), tail])[:64]; t = np.concatenate([head, r4(m + int(rng.integers(0, 4))), tail])
    elif recipe == "mid-long":
        a = max(1, ql // 2); head, tail = r4(a), r4(max(1, ql - a))
        q = np.concatenate([head, tail])[:64]; t = np.concatenate([head, r4(int(rng.integers(60, 90))), tail])
    elif recipe == "t-short":
        q = r4(ql); t = q[:max(0, ql // 4 - int(rng.integers(0, 3)))].copy()
    else:
        q = r4(ql); t = np.concatenate([q, r4(int(rng.integers(70, 96)))])
    return np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t[:160], np.uint8)


_pools = {}


def pool(preset):
    """The preset's pool: a list of (query, target), made once."""
    if preset not in _pools:
        rng = np.random.default_rng(POOL_SEED[preset])
        _pools[preset] = [_job(rng, RECIPES[i % len(RECIPES)]) for i in range(POOL_N)]
    return _pools[preset]


def labels(preset):
    return np.frombuffer(LABELS[preset].encode(), np.uint8) - ord("0")


def job_set(preset, size, mix):
    """(jobs, types, exits): exits[i] is the label of a type-1 job and -1 for a type-2 job (the same sequences through ksw_global2)."""
    P, lab = pool(preset), labels(preset)
    long_q = np.array([len(q) >= 49 for q, _ in P])
    easy, hard = np.flatnonzero(lab == 0), np.flatnonzero(lab > 0)
    easy_l, hard_l = np.flatnonzero((lab == 0) & long_q), np.flatnonzero((lab > 0) & long_q)
    if mix == "easy":
        idx = [(int(easy[k]), 1 if k % 3 else 2) for k in range(size)]              # every third a seed-gap job
    elif mix == "one-last":
        at = min(size, 64) - 1
        idx = [(int(easy_l[k]), 1) for k in range(size)]
        idx[at] = (int(hard_l[size % len(hard_l)]), 1)
    elif mix == "hard":
        idx = [(int(h), 1) for h in _spread(lab, hard, size)]
    else:
        n_hard = {1: 1, 63: 5, 64: 7, 65: 3, 200: 70}[size]
        hs = _spread(lab, hard, n_hard)
        idx, e = [], 0
        step = max(1, size // n_hard)
        for k in range(size):
            if k % step == step - 1 and len(hs):
                idx.append((int(hs.pop()), 1))
            else:
                idx.append((int(easy[e]), 1 if e % 4 else 2)); e += 1
    jobs = [P[i] for i, _ in idx]
    types = np.array([t for _, t in idx], np.int32)
    exits = np.array([int(lab[i]) if t == 1 else -1 for i, t in idx], np.int32)
    return jobs, types, exits


def _spread(lab, hard, n):
    """n hard pool jobs, the five hard exits in turn."""
    by = [list(np.flatnonzero(lab == e)) for e in range(1, 6)]
    out, k = [], 0
    while len(out) < n:
        b = by[k % 5]; k += 1
        if b:
            out.append(b.pop(0))
        assert k < 20 * n + 100, "the pool has too few hard jobs"
    return out


def set_ids():
    return [(p, n, m) for p in PRESETS for n in SIZES for m in MIXES]


# ---------------------------------------------------------------- the emulation's driver for explicit job sets (tests/emu/emu_lanedp.cpp)
_emu = None


def emu():
    global _emu
    if _emu is None:
        os.makedirs(reflib.EMU_DIR, exist_ok=True)
        out = os.path.join(reflib.EMU_DIR, "libhp_emu_lanedp.so")
        emu_dir = os.path.join(reflib.ROOT, "tests", "emu"); csrc = os.path.join(reflib.ROOT, "lamsa_amd", "csrc")
        src = os.path.join(emu_dir, "emu_lanedp.cpp")
        deps = [src, os.path.join(emu_dir, "emu_api.cpp"), os.path.join(emu_dir, "hp", "wave.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.run(["g++"] + reflib.EMU_FLAGS + ["-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", emu_dir, "-I", csrc,
                            "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", out, src], check=True, cwd=reflib.EMU_DIR)
        _emu = C.CDLL(out)
        _emu.emu_stat.restype = C.c_longlong
    return _emu


def _packed(jobs):
    from lamsa_amd.hp import pack_jobs
    return pack_jobs(jobs)


def emu_exits(jobs, hp_para):
    E = emu()
    seq, q_off, qlen, t_off, tlen = _packed(jobs)
    ex = np.zeros(len(jobs), np.int32)
    p = lambda a: a.ctypes.data
    E.emu_lane_exits.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    assert E.emu_lane_exits(C.byref(hp_para), len(jobs), p(seq), p(q_off), p(qlen), p(t_off), p(tlen), p(ex)) == 0
    return ex


def emu_stages(jobs, types, hp_para, stages=True, hard_cap=0):
    """The set through phase_filldp under the lane emulation: dict(has, cells, hard, cigars, stats); stats: the path counters 97 .. 107 by slot."""
    E = emu()
    n = len(jobs)
    seq, q_off, qlen, t_off, tlen = _packed(jobs)
    types = np.ascontiguousarray(types, np.int32)
    has = np.zeros(n, np.int32); cells = np.zeros(n, np.int32); hard = np.zeros(n, np.int32); cn = np.zeros(n, np.int32); cig = np.zeros(n * HP_LJ_CIG + 4, np.int32)
    p = lambda a: a.ctypes.data
    E.emu_stat_reset(); E.emu_lds_guard_reset()
    E.emu_lane_stages.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 2 + [C.c_void_p] * 5
    rc = E.emu_lane_stages(C.byref(hp_para), n, p(seq), p(q_off), p(qlen), p(t_off), p(tlen), p(types), 1 if stages else 0, int(hard_cap), p(has), p(cells), p(hard), p(cn), p(cig))
    assert rc == 0, rc
    E.emu_lds_guard_hits.restype = C.c_longlong
    assert E.emu_lds_guard_hits() == 0
    return dict(has=has, cells=cells, hard=hard, cigars=[cig[i * HP_LJ_CIG:i * HP_LJ_CIG + cn[i]].tolist() for i in range(n)], stats={i: int(E.emu_stat(i)) for i in range(97, 108)})


# the exits of the pool jobs, in pool order (checked against the emulation by tests/test_lanedp_stages_cpu.py)
LABELS = {
    "default": (
        "0105040000550400005501000005030000450400015101000145030000510400005104000055040000555100005504000055010005455400005503000051010000550300054503000055030002550300"
        "0105010000515300015504000025030000110100004504000051530000555300014103000055030000410300005554000051030000500400001504000055030000150300025101000035030005550300"
        "0051030001510300000551000041030001450300005503000045530001050300004500000005010000550100001153000052010005515100030101000355010000010400015153000045010000550300"
        "0005030000455100004503000155510000520300015553000055030000450100005503000041040001550300003201000055040000550300005501000055040001050100000501000055300000155100"
        "0141040000515300005501000055010000553100005504000005040002515400004103000055040005550100031101000055030000550100005501000045040000555300021504000251030000550300"
        "0155040005150300000501000051030001550100005001000015030004450400050504000251510001500300001103000155030005510100005503000055040000210300014551000045540000150100"
        "0045030001115300004154000145030000550300034504000051540002450300004554000055540001550100014503000031530005553300000553000555030000550100005503000055530000550400"
        "0055040001510200004553000055000000210400012553000041540000550100010504000055510000150300004503000055530000550300001153000055000000450300011501000055010000315300"
        "0051030000555300005501000051540000410300005503000052010000550300005503000135030000550000005104000155010000450400014023000055010000555300005504000145030000055300"
        "0141040000150300015501000045010001550100000103000052020000550400000503000005530000050300025503000005010000550400003103000041510000155300005504000255010001455100"
    ),
    "ont2d": (
        "0101010000010300000201000012040001150100000203000002010000110300001103000011010000110400000204000001510001010100001204000002030000120100010103000102510000010100"
        "0011030000020300000503000011010000020100000151000012030001110100010251000112030000010300000201000002500000020100011201000031030000110300005104000002010000115300"
        "0001040000120300011201000001000000515300000203000002030000010300000203000152030001125100005101000011030001050100000104000011230000050100000502000111040000000400"
        "0011030001020400000153000102030000120100010200000012010001010100001101000012030001115100000101000112030000120100021201000101040000110100001101000001030000010000"
        "0001040000025300001204000001040000115300000201000015010001110400001103000012040000010300001101000012030000010200011103000102510000120100001104000002030000125400"
        "0111010000010300011101000002040000115100011201000101010001110300000254000001030001122100001100000001030000120100000203000012530000010300000101000011030000010200"
        "0002040000120400013201000001030000010300001201000011010000020300011101000001010000010100000101000012010001010100001204000111010000120100001203000111010001020300"
        "0011030000120100000101000001040001010400001151000005010000120100000201000012030000110300000103000001010000010400000501000011030000120300001101000030010001110100"
        "0012010000020100000201000002040000025300010203000012010000025100001203000012030000120300001201000001030001021400000101000112030000010300011204000011030000010300"
        "0002030000020300000201000002030000020300001204000112300001050100000103000105010001110300000203000011010000020400001103000012210000000100000201000011010000010300"
    ),
    "pacbio": (
        "0002010001120300001154000002040001120300000101000111030000120100001221000002010000020100000203000102010000120300000201000031010001050100001203000112040001020300"
        "0012540000010400001201000012040005050300001203000002030001020400000253000002530001020400011203000111010000120100000251000012040000015300000101000015010000110400"
        "0012030000120100005213000002030000120100001204000101030001110400000203000012030000120400000203000112030001020100012101000012010000020300001204000002030000120100"
        "0011030001020400001501000011030000120300001204000112010000010100000102000012010000015400010204000111010000020100010201000012040001020100011501000111010000010300"
        "0101010000120100001503000121030000020100001201000012030001020300001201000012030000120100011203000012030000020400000101000001040000020400011204000002030001020300"
        "0101010000120300011201000115010000050300000204000101030000020300001503000002030000120100001153000011130000010100001201000012030001110300011123000052010000020300"
        "0002010001115100001203000012030000150000001201000012030001010300001201000002040001120100001201000011000000120300000204000012510000120100011203000105010000020300"
        "0002040000010400001203000152010000120400001103000012040000015300010253000052030000020300010103000011130001120100010001000111030001020100010103000112040000120100"
        "0001030001010100011201000112000000110100005103000002030000150300000203000012030000020400011201000001040000050300001201000012010000020100001203000005030000120100"
        "0102330001020100010251000002040000020400001203000012040001120300000201000102030000320300000201000012010001020100001203000002030000520300005251000012010000120300"
    ),
}
