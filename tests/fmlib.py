"""Shared by tests/test_fm_cpu.py and tests/test_fm_gpu.py: the synthetic repeat genome, the query sets with their class counters, and
the CPU builds that link tests/emu/emu_fm.cpp (lamsa_hp_fm_load / lamsa_hp_fm_search on the lane emulation)."""
import ctypes as C
import os
import subprocess

import numpy as np

import reflib
from lamsa_amd import hp

ROOT = reflib.ROOT
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "lamsa_amd", "csrc")
HOST = os.path.join(ROOT, "lamsa_amd", "host")
KS = (1, 12, 19, 33)


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def _hdrs():
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(EMU, "hp", "wave.h"), os.path.join(ROOT, "include", "lamsa_hp.h"),
                                                                                    os.path.join(HOST, "lamsa_host.h"), os.path.join(HOST, "rescue.h")]


def emu_fm_lib():
    """tests/_build/libhp_emu_fm.so: emu_fm.cpp alone (hp_fm.h under the lane emulation)."""
    os.makedirs(reflib.EMU_DIR, exist_ok=True)
    out = os.path.join(reflib.EMU_DIR, "libhp_emu_fm.so")
    src = os.path.join(EMU, "emu_fm.cpp")
    if _stale(out, [src] + _hdrs()):
        subprocess.run(["g++"] + reflib.EMU_FLAGS + ["-g", "-std=c++17", "-fPIC", "-shared", "-I", EMU, "-I", CSRC, "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                                     "-o", out, src], check=True, cwd=reflib.EMU_DIR)
    L = C.CDLL(out)
    L.lamsa_hp_fm_load.argtypes = [C.c_void_p, C.POINTER(hp.HpFmIndex)]
    L.lamsa_hp_fm_search.argtypes = [C.c_void_p, C.POINTER(hp.HpFmQueries), C.POINTER(hp.HpFmOut)]
    L.emu_fm_last_slices.restype = C.c_longlong
    return L


def emu_cli_fm():
    """tests/_build/lamsa_emu_fm: the host program on the emulated C-ABI (as reflib.emu_cli) with emu_fm.cpp supplying the two FM calls."""
    os.makedirs(reflib.EMU_DIR, exist_ok=True)
    out = os.path.join(reflib.EMU_DIR, "lamsa_emu_fm")
    srcs = [os.path.join(HOST, f) for f in ("main.cpp", "lamsa_host.cpp", "rescue.cpp", "index.cpp")] + [os.path.join(EMU, f) for f in ("emu_api.cpp", "emu_capi.cpp", "emu_fm.cpp")]
    if _stale(out, srcs + _hdrs()):
        subprocess.run(["g++"] + reflib.EMU_FLAGS + ["-g", "-std=c++17", "-ffp-contract=off", "-I", EMU, "-I", CSRC, "-o", out] + srcs + ["-lz", "-lpthread"], check=True, cwd=reflib.EMU_DIR)
    return out


def plan_check_bin():
    """tests/_build/fm_plan_check: tests/host/fm_plan_check.cpp (its own main) + the planner + emu_fm.cpp, with ASan and UBSan."""
    os.makedirs(reflib.EMU_DIR, exist_ok=True)
    out = os.path.join(reflib.EMU_DIR, "fm_plan_check")
    srcs = [os.path.join(ROOT, "tests", "host", "fm_plan_check.cpp"), os.path.join(HOST, "rescue.cpp"), os.path.join(HOST, "lamsa_host.cpp"),
            os.path.join(EMU, "emu_api.cpp"), os.path.join(EMU, "emu_capi.cpp"), os.path.join(EMU, "emu_fm.cpp")]
    if _stale(out, srcs + _hdrs()):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I", EMU, "-I", CSRC, "-I", HOST, "-o", out] + srcs + ["-lz", "-lpthread"], check=True, cwd=reflib.EMU_DIR)
    return out


# ------------------------------------------------------------------ the synthetic repeat genome
UNIT64_COPIES, TANDEM_COPIES, POLY_A = 150, 700, 300


def write_repeat_genome(path, seed=20):
    """At most 100 kbp in two contigs: random sequence, a 64-bp unit scattered UNIT64_COPIES times, a 24-bp unit TANDEM_COPIES times in
    tandem, a poly-A run of POLY_A and a stretch of N.  The first base is G, so the doubled text ends in C and its smallest suffix is the
    start of the A run (row 1), its largest the start of the T run of the reverse strand (the last row)."""
    rng = np.random.RandomState(seed)
    B = np.array(list("ACGT"))

    def rnd(n):
        return "".join(B[rng.randint(0, 4, n)])
    unit64, unit24 = rnd(64), "ACGGTCATTGCAGTACCTGATCGA"
    c1 = "G" + rnd(199)
    for i in range(100):
        c1 += unit64 + rnd(int(rng.randint(150, 450)))
    c1 += "N" * 50 + rnd(1500)
    c2 = rnd(3000)
    for i in range(UNIT64_COPIES - 100):
        c2 += unit64 + rnd(int(rng.randint(150, 300)))
    c2 += "C" + unit24 * TANDEM_COPIES + "G" + rnd(700) + "C" + "A" * POLY_A + "G" + rnd(2500)
    assert len(c1) + len(c2) <= 100000
    with open(path, "w") as f:
        for name, s in (("rep1", c1), ("rep2", c2)):
            f.write(">%s\n" % name)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    return unit64, unit24


def index_genome(cli, fasta):
    """`lamsa index --no-gem` (host code: the product binary and the emulated one are the same here)."""
    p = subprocess.run([cli, "index", "--no-gem", fasta], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    for ext in (".pac", ".ann", ".bwt", ".sa"):
        assert os.path.exists(fasta + ext), ext


# ------------------------------------------------------------------ query sets
def make_queries(chk, k, seed, sa_intv=32, repeat_genome=True):
    """Windows of k - 1, k, k + 1 and 300 bases: cut from the text on both strands, at the k-mers of chosen rows (row 1, the last row, the
    rows round `primary`, rows at the ends of a 128-row block and sampled rows), with errors, with N, and random ones.  Returns (seq, win_off)."""
    rng = np.random.RandomState(seed)
    t, n = chk.text, chk.n
    wins = []

    def cut(p, ln):
        p = max(0, min(int(p), n - ln))
        wins.append(t[p:p + ln].copy())
    for ln in (k - 1, k, k + 1, 300):
        for p in rng.randint(0, n - 300, 6):
            cut(p, ln)
    rows = [1, 2, n, n - 1, chk.primary - 1, chk.primary, chk.primary + 1]
    for m in (1, 2, chk.primary // 128, chk.primary // 128 + 1, n // 128 - 1):
        rows += [128 * m - 1, 128 * m, 128 * m + 1, 128 * m + 127, 128 * m + 128]
    rows += [sa_intv * int(x) for x in rng.randint(1, n // sa_intv, 6)]
    for r in rows:
        if 1 <= r <= n and chk.row_value(r) + k <= n:
            cut(chk.row_value(r), k)
    if repeat_genome:
        s = "".join("ACGT"[c] for c in t[:n // 2])
        for pat in ("ACGGTCATTGCAGTACCTGATCGA" * 4, "A" * 40):
            a = s.find(pat); b = s.rfind(pat) + len(pat)
            for p in (a - 150, a - k // 2, a + 30, b - 150, b - 290, b - k - 1, b - k, b - k + 1):     # into, inside and out of the tandem / the A run
                cut(p, 300); cut(p, k + 1); cut(n - 1 - p - 300, 300)
        for j in range(3):                                                                            # a 64-bp unit copy: find one through its count
            p = int(rng.randint(0, n - 300))
            cut(p, 300)
    for i in range(8):                                      # errors, N, and sequence that is not there
        w = t[int(rng.randint(0, n - 300)):][:300].copy()
        for x in rng.randint(0, 300, 12):
            w[x] = (w[x] + 1 + rng.randint(0, 3)) & 3
        if i & 1:
            w[rng.randint(0, 300, 3)] = 4
        wins.append(w)
    wins.append(rng.randint(0, 4, 300).astype(np.uint8))
    wins.append(np.full(k + 1, 4, np.uint8))
    wins.append(np.zeros(0, np.uint8))
    win_off = np.concatenate([[0], np.cumsum([len(w) for w in wins])]).astype(np.int64)
    return np.concatenate(wins + [np.zeros(16, np.uint8)]).astype(np.uint8), win_off


def kmers_of(seq, win_off, k):
    parts = [np.lib.stride_tricks.sliding_window_view(seq[win_off[w]:win_off[w + 1]], k) for w in range(len(win_off) - 1) if win_off[w + 1] - win_off[w] >= k]
    return np.concatenate(parts) if parts else np.zeros((0, k), np.uint8)


def pick_max_occ(cnt):
    """A max_occ, besides 100 and 500, that some k-mer of the set meets exactly and another exceeds by one: the largest such count."""
    have = set(int(c) for c in cnt)
    best = [c for c in have if c >= 2 and c + 1 in have and c not in (100, 500)]
    return max(best) if best else None


def classes(seq, win_off, k, cnt, max_occ):
    """Counters of the classes stage 4 tells apart, over the k-mers of a query set (cnt: the checker's occurrence counts)."""
    km = kmers_of(seq, win_off, k)
    has4 = (km > 3).any(axis=1)
    return dict(absent=int(((cnt == 0) & ~has4).sum()), once=int((cnt == 1).sum()), at_max=int((cnt == max_occ).sum()), over_max=int((cnt == max_occ + 1).sum()),
                mid=int(((cnt >= 101) & (cnt <= 500)).sum()), many=int((cnt > 500).sum()), code4=int(has4.sum()),
                a_run=int(((km[:, -min(k, 8):] == 0).all(axis=1) & ~has4).sum()))


def rows_queried(lo, hi, cnt, max_occ):
    """[(lo, hi)] of the k-mers whose rows are located."""
    take = (cnt >= 1) & (cnt <= max_occ)
    return lo[take].astype(np.int64), hi[take].astype(np.int64)


def covers(lo, hi, row):
    return bool(((lo <= row) & (row <= hi)).any())


def covers_where(lo, hi, pred, limit=200000):
    """Is there a located row r with pred(r)?  (walks the intervals; they are short)"""
    seen = 0
    for a, b in zip(lo.tolist(), hi.tolist()):
        for r in range(a, b + 1):
            if pred(r):
                return True
            seen += 1
            if seen > limit:
                return False
    return False


def fm_search_lib(L, handle, seq, win_off, k, max_occ):
    """lamsa_hp_fm_search of a ctypes library -> (rc, arrays or None)."""
    seq = np.ascontiguousarray(seq, np.uint8); win_off = np.ascontiguousarray(win_off, np.int64)
    n_win = len(win_off) - 1
    Q = hp.HpFmQueries(n_win, seq.ctypes.data, len(seq), win_off.ctypes.data, int(k), int(max_occ))
    O = hp.HpFmOut()
    rc = L.lamsa_hp_fm_search(handle, C.byref(Q), C.byref(O))
    return rc, (hp.fm_result(O, n_win) if rc == 0 else None)


def assert_same(got, want, what):
    kmer_off, lo, hi, pos_off, pos = got
    assert np.array_equal(kmer_off, want[0]), what
    assert np.array_equal(lo, want[1]) and np.array_equal(hi, want[2]), (what, np.nonzero((lo != want[1]) | (hi != want[2]))[0][:5])
    assert np.array_equal(pos_off, want[3]), what
    assert np.array_equal(pos, want[4]), (what, np.nonzero(pos != want[4])[0][:5])
