"""Shared by tests/test_seed_cpu.py and tests/test_seed_gpu.py: the CPU builds that link tests/emu/emu_seed.cpp (lamsa_hp_fm_seed on the
lane emulation, with emu_fm.cpp's index), the hand-placed reads on the repeat genome of tests/fmlib.py, and the parameter sets."""
import ctypes as C
import os
import subprocess

import numpy as np

import fmcheck
import fmlib
import goldenlib
import reflib
import seedcheck
from lamsa_amd import hp

ROOT = reflib.ROOT
EMU, CSRC, HOST = fmlib.EMU, fmlib.CSRC, fmlib.HOST
# (seed_len, seed_step, max_hits); the last one runs on three short reads only
PARAMS = ((50, 100, 200), (50, 25, 150), (50, 25, 149), (20, 10, 200), (63, 63, 200))
PARAMS_SHORT = (1, 1, 16383)


def emu_seed_lib():
    """tests/_build/libhp_emu_seed.so: emu_seed.cpp (which includes emu_fm.cpp): the three FM calls on the lane emulation."""
    os.makedirs(reflib.EMU_DIR, exist_ok=True)
    out = os.path.join(reflib.EMU_DIR, "libhp_emu_seed.so")
    srcs = [os.path.join(EMU, "emu_seed.cpp")]
    if fmlib._stale(out, srcs + [os.path.join(EMU, "emu_fm.cpp")] + fmlib._hdrs()):
        subprocess.run(["g++"] + reflib.EMU_FLAGS + ["-g", "-std=c++17", "-fPIC", "-shared", "-I", EMU, "-I", CSRC, "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                                     "-o", out] + srcs, check=True, cwd=reflib.EMU_DIR)
    L = C.CDLL(out)
    L.lamsa_hp_fm_load.argtypes = [C.c_void_p, C.POINTER(hp.HpFmIndex)]
    L.lamsa_hp_fm_seed.argtypes = [C.c_void_p, C.POINTER(hp.HpSeedQueries), C.POINTER(hp.HpBatch)]
    L.emu_seed_last_slices.restype = C.c_longlong
    return L


def emu_cli_seed():
    """tests/_build/lamsa_emu_seed: the host program on the emulated C-ABI with emu_seed.cpp supplying the three FM calls (--seed-fm, --rescue-gpu)."""
    os.makedirs(reflib.EMU_DIR, exist_ok=True)
    out = os.path.join(reflib.EMU_DIR, "lamsa_emu_seed")
    srcs = [os.path.join(HOST, f) for f in ("main.cpp", "lamsa_host.cpp", "rescue.cpp", "index.cpp")] + [os.path.join(EMU, f) for f in ("emu_api.cpp", "emu_capi.cpp", "emu_seed.cpp")]
    if fmlib._stale(out, srcs + [os.path.join(EMU, "emu_fm.cpp")] + fmlib._hdrs()):
        subprocess.run(["g++"] + reflib.EMU_FLAGS + ["-g", "-std=c++17", "-ffp-contract=off", "-I", EMU, "-I", CSRC, "-o", out] + srcs + ["-lz", "-lpthread"], check=True, cwd=reflib.EMU_DIR)
    return out


def seed_check_bin():
    """tests/_build/seed_check: tests/host/seed_check.cpp (its own main) + the host's index readers + emu_seed.cpp, with ASan and UBSan."""
    os.makedirs(reflib.EMU_DIR, exist_ok=True)
    out = os.path.join(reflib.EMU_DIR, "seed_check")
    srcs = [os.path.join(ROOT, "tests", "host", "seed_check.cpp"), os.path.join(HOST, "rescue.cpp"), os.path.join(HOST, "lamsa_host.cpp"),
            os.path.join(EMU, "emu_api.cpp"), os.path.join(EMU, "emu_capi.cpp"), os.path.join(EMU, "emu_seed.cpp")]
    if fmlib._stale(out, srcs + [os.path.join(EMU, "emu_fm.cpp")] + fmlib._hdrs()):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I", EMU, "-I", CSRC, "-I", HOST, "-o", out] + srcs + ["-lz", "-lpthread"], check=True, cwd=reflib.EMU_DIR)
    return out


def fm_seed_lib(L, handle, read_off, read_seq, seed_len, seed_step, max_hits, seq_offset, seq_len, n_reads=None):
    """lamsa_hp_fm_seed of a ctypes library -> (rc, dict of arrays or None)."""
    read_off = np.ascontiguousarray(read_off, np.int64); read_seq = np.ascontiguousarray(read_seq, np.uint8)
    seq_offset = np.ascontiguousarray(seq_offset, np.int64); seq_len = np.ascontiguousarray(seq_len, np.int32)
    Q = hp.HpSeedQueries(len(read_off) - 1 if n_reads is None else n_reads, read_off.ctypes.data, read_seq.ctypes.data, int(seed_len), int(seed_step), int(max_hits),
                         len(seq_len), seq_offset.ctypes.data, seq_len.ctypes.data)
    b = hp.HpBatch()
    rc = L.lamsa_hp_fm_seed(handle, C.byref(Q), C.byref(b))
    if rc != 0:
        return rc, None
    d = hp.seed_batch_arrays(b)
    d["read_seq"] = read_seq
    return rc, d


def hp_para_of(lp):
    """The oracle's parameters (reflib.lo_para) as the struct of the C-ABI, without the HIP library."""
    P = hp.HpPara()
    for n, _ in hp.HpPara._fields_:
        setattr(P, n, getattr(lp, n))
    return P


def contig_arrays(contigs):
    return np.array([c[1] for c in contigs], np.int64), np.array([c[2] for c in contigs], np.int32)


INVERTED = (5000, 200)                                       # bases of contig 1 whose reverse complement ends contig 2


def write_seed_genome(path):
    """fmlib.write_repeat_genome's two contigs, the second one followed by the reverse complement of INVERTED of the first: that genome
    has no sequence on both strands, and a slot with hits on both strands is one of the classes the tests want."""
    fmlib.write_repeat_genome(path)
    seqs, name = {}, None
    for line in open(path):
        if line.startswith(">"):
            name = line[1:].strip(); seqs[name] = []
        else:
            seqs[name].append(line.strip())
    c1, c2 = "".join(seqs["rep1"]), "".join(seqs["rep2"])
    inv = c1[INVERTED[0]:INVERTED[0] + INVERTED[1]]
    assert "N" not in inv
    c2 += inv[::-1].translate(str.maketrans("ACGT", "TGCA"))
    assert len(c1) + len(c2) <= 100000
    with open(path, "w") as f:
        for nm, s in (("rep1", c1), ("rep2", c2)):
            f.write(">%s\n" % nm)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")


# ------------------------------------------------------------------ the hand-placed reads
def make_reads(chk, contigs, seed=5):
    """About a hundred reads of 0 .. 1 200 bases on the genome of write_seed_genome, cut from the doubled text -- so from both
    strands -- at the places where a rule of the definition decides: inside the 64-bp unit (150 rows: exactly max_hits, or one more), the
    24-bp tandem and the A run (over max), across the boundary of the two contigs on both strands, across the middle of the doubled
    text, at the first and the last base of a contig, through the N stretch; reads of length 0, seed_len - 1, seed_len for every seed
    length, lengths with (L - seed_len) % seed_step zero and non-zero, an all-N read, a random read that hits nothing, a read that is a
    forward stretch followed by the reverse complement of another, two through the stretch that lies on both strands, and a few with
    1 % substitutions.  Returns (names, reads)."""
    rng = np.random.RandomState(seed)
    t, n = chk.text, chk.n
    l_pac = n // 2
    off2 = contigs[1][1]
    s = "".join("ACGT"[x] for x in t[:l_pac])
    reads = []

    def cut(p, ln):
        p = max(0, min(int(p), n - ln))
        reads.append(t[p:p + ln].copy())
    u = 200                                                  # the first copy of the 64-bp unit
    for ln in (64, 114, 164, 400):
        cut(u, ln); cut(u - (ln - 64) // 2, ln); cut(n - u - 64, ln)
    tandem = s.find("ACGGTCATTGCAGTACCTGATCGA" * 4); polya = s.find("A" * 40)
    for p in (tandem - 100, tandem + 24 * 350, tandem + 24 * 700 - 150, polya - 120, polya + 100, polya + 300 - 90):
        cut(p, 300); cut(n - p - 300, 300)
    for ln in (126, 150, 200, 263, 1200):                    # across the contig boundary, '+' and '-', and across the middle of the text
        cut(off2 - ln // 2, ln); cut(off2 - ln + 20, ln); cut(n - off2 - ln // 2, ln); cut(n - off2 - 20, ln)
        cut(l_pac - ln // 2, ln); cut(l_pac - ln + 30, ln)
    for ln in (126, 150, 200, 630):                          # first and last bases of both contigs, both strands
        cut(0, ln); cut(off2 - ln, ln); cut(off2, ln); cut(l_pac - ln, ln)
        cut(n - ln, ln); cut(n - off2, ln); cut(n - off2 - ln, ln); cut(l_pac, ln)
    nst = s.find(s[contigs[0][2] - 1500 - 50:contigs[0][2] - 1500])      # (the N stretch of contig 1: 50 substituted bases before its last 1 500)
    cut(contigs[0][2] - 1500 - 150, 400)
    for ln in (0, 19, 20, 49, 50, 62, 63, 75, 101, 175):      # length 0, seed_len - 1, seed_len; (L - seed_len) % seed_step zero and not
        cut(int(rng.randint(0, n - 200)), ln)
    reads.append(np.full(180, 4, np.uint8))                   # all N
    reads.append(rng.randint(0, 4, 400).astype(np.uint8))     # hits nothing
    w = t[5000:5400].copy(); w[[30, 130, 260]] = 4; reads.append(w)      # N inside some seeds
    a = t[7000:7150].copy(); b = t[n - 9000 - 150:n - 9000].copy(); reads.append(np.concatenate([a, b]))       # '+' then '-'
    cut(INVERTED[0] + 10, 176); cut(INVERTED[0] - 100, 400)   # through the stretch that lies on both strands (write_seed_genome)
    for i in range(6):                                        # 1 % substitutions
        w = t[int(rng.randint(0, n - 1200)):][:1200 if i < 2 else 500].copy()
        for x in rng.randint(0, len(w), max(1, len(w) // 100)):
            w[x] = (w[x] + 1 + rng.randint(0, 3)) & 3
        reads.append(w)
    names = ["q%d" % i for i in range(len(reads))]
    assert nst >= 0
    return names, reads


def short_reads(chk):
    """Three short reads for (1, 1, 16383)."""
    t = chk.text
    return ["s0", "s1", "s2"], [t[100:103].copy(), np.array([0, 4, 3, 2, 1], np.uint8), np.zeros(0, np.uint8)]


# ------------------------------------------------------------------ the golden scenarios for `lamsa aln --seed-fm`
def stage(name, d, golden):
    """The scenario without its GEM map and without a .gem index; the checker's map for the scenario's seeding options written beside."""
    ref, reads, args, _ = goldenlib.stage_scenario(name, d)
    os.remove(reads + ".seed.gem.map")
    rt, over = goldenlib.para_from_args(args)
    P = reflib.lo_para(rt, **over)
    prm = (int(P.seed_len), int(P.seed_step), int(P.per_aln_m))
    rd = seedcheck.read_fasta(reads)
    want = seedcheck.expected(golden["chk"], golden["contigs"], [r for _, r in rd], *prm)
    mp = os.path.join(d, "checker.map")
    seedcheck.write_map(mp, [n for n, _ in rd], want, golden["contigs"], prm[0], prm[1])
    with open(reads + ".seed.info", "w") as f:
        for r, (n, s) in enumerate(rd):
            f.write("%s %d %d %d\n" % (n, int(want.seed_all[r]), int(want.last_len[r]), len(s)))
    os.makedirs(os.path.join(d, "nogem"), exist_ok=True)
    return ref, reads, args, mp, want
