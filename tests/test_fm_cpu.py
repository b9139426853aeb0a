"""The device FM index without a GPU: the independent checker (tests/fmcheck.py) against the index files, lamsa_amd/csrc/hp_fm.h under the
lane emulation (tests/emu/emu_fm.cpp) against the checker, the stage-4 planner from both seed sources (tests/host/fm_plan_check.cpp, built
with ASan and UBSan), and `lamsa aln --rescue-gpu` of the emulated host program.  tests/test_fm_gpu.py runs the same query sets on the
MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fmcheck
import fmlib
import goldenlib as G
import reflib
from lamsa_amd import hp

GOLD_REF = os.path.join(G.GOLD, "ref", "ref.fa")


@pytest.fixture(scope="module")
def golden():
    return GOLD_REF, fmcheck.FmCheck(GOLD_REF)


@pytest.fixture(scope="module")
def repeat(tmp_path_factory):
    d = tmp_path_factory.mktemp("repeat")
    fa = str(d / "rep.fa")
    fmlib.write_repeat_genome(fa)
    fmlib.index_genome(reflib.emu_cli(), fa)
    return fa, fmcheck.FmCheck(fa)


@pytest.fixture(scope="module")
def emu_fm():
    return fmlib.emu_fm_lib()


def _load(L, key, prefix):
    ix, keep = hp.read_fm_index(prefix)
    assert L.lamsa_hp_fm_load(C.c_void_p(key), C.byref(ix)) == 0
    return ix


def test_checker_against_the_index_files(golden, repeat):
    """(a) The checker's rows are the index's: `primary` is the row of suffix 0 and the j-th value of .sa is the value of row sa_intv * j,
    for every sample of the fixture and of the repeat genome."""
    for prefix, chk in (golden, repeat):
        hdr = np.fromfile(prefix + ".bwt", np.uint64, 5)
        sh = np.fromfile(prefix + ".sa", np.uint64, 7)
        sa = np.fromfile(prefix + ".sa", np.uint64, offset=56)
        intv = int(sh[5])
        assert int(hdr[4]) == chk.n and int(hdr[0]) == chk.primary
        assert len(sa) == chk.n // intv
        assert np.array_equal(sa.astype(np.int64), chk.sa[intv - 1::intv][:len(sa)])
        counts = np.bincount(chk.text, minlength=4)
        assert np.array_equal(np.cumsum(counts), hdr[1:5].astype(np.int64))


@pytest.mark.parametrize("k", fmlib.KS)
@pytest.mark.parametrize("genome", ["golden", "repeat"])
def test_emulated_search_against_the_checker(genome, k, golden, repeat, emu_fm):
    """(b) hp_fm.h under the lane emulation: lo, hi, pos_off and pos word for word the checker's, with max_occ 100, 500 and one that a
    k-mer of the set meets exactly and another exceeds by one; on the repeat genome the set holds every class of k-mer and row.
    A 1-mer occurs tens of thousands of times in either genome, so for k = 1 only the classes above 500, with code 4 and ending in A exist."""
    prefix, chk = golden if genome == "golden" else repeat
    key = 0x1000 + (genome == "repeat")
    ix = _load(emu_fm, key, prefix)
    seq, win_off = fmlib.make_queries(chk, k, seed=7 * k + 1, sa_intv=int(ix.sa_intv), repeat_genome=genome == "repeat")
    cnt = chk.search(seq, win_off, k, 0)[5]
    m_star = fmlib.pick_max_occ(cnt)
    for max_occ in (100, 500, m_star, 0):
        if max_occ is None:
            continue
        want = chk.search(seq, win_off, k, max_occ)
        rc, got = fmlib.fm_search_lib(emu_fm, C.c_void_p(key), seq, win_off, k, max_occ)
        assert rc == 0
        fmlib.assert_same(got, want, (genome, k, max_occ))
    if genome != "repeat":
        return
    want = chk.search(seq, win_off, k, 500)
    cl = fmlib.classes(seq, win_off, k, cnt, m_star if m_star is not None else -9)
    print(k, m_star, cl)
    assert cl["many"] > 0 and cl["code4"] > 0 and cl["a_run"] > 0, cl
    if k > 1:
        assert m_star is not None and all(v > 0 for v in cl.values()), (m_star, cl)
        lo, hi = fmlib.rows_queried(want[1], want[2], cnt, 500)
        for row in (1, chk.n, chk.primary - 1, chk.primary, chk.primary + 1):
            assert fmlib.covers(lo, hi, row), row
        stored = lambda r: r - (r >= chk.primary)
        assert fmlib.covers_where(lo, hi, lambda r: r % int(ix.sa_intv) == 0)
        assert fmlib.covers_where(lo, hi, lambda r: r != chk.primary and stored(r) % 128 == 0)
        assert fmlib.covers_where(lo, hi, lambda r: r != chk.primary and stored(r) % 128 == 127)


def test_emulated_search_slices_and_edges(repeat, emu_fm, monkeypatch):
    """The locate pass in slices of 1000 positions (LAMSA_HP_FM_SLICE) gives the same words; zero windows, a set whose k-mers are no
    multiple of 64, and the same call twice in a row."""
    prefix, chk = repeat
    key = C.c_void_p(0x2000)
    _load(emu_fm, 0x2000, prefix)
    seq, win_off = fmlib.make_queries(chk, 19, seed=3)
    want = chk.search(seq, win_off, 19, 500)
    monkeypatch.setenv("LAMSA_HP_FM_SLICE", "1000")
    for rep in range(2):
        rc, got = fmlib.fm_search_lib(emu_fm, key, seq, win_off, 19, 500)
        assert rc == 0 and emu_fm.emu_fm_last_slices() == (len(want[4]) + 999) // 1000 > 3
        fmlib.assert_same(got, want, "slices")
    monkeypatch.delenv("LAMSA_HP_FM_SLICE")
    rc, got = fmlib.fm_search_lib(emu_fm, key, seq, win_off[:1], 19, 500)
    assert rc == 0 and len(got[1]) == 0 and got[3].tolist() == [0]
    sub = win_off[:12]
    want = chk.search(seq, sub, 19, 500)
    assert len(want[1]) % 64 != 0
    rc, got = fmlib.fm_search_lib(emu_fm, key, seq, sub, 19, 500)
    assert rc == 0
    fmlib.assert_same(got, want, "odd")


def _plan_cases(prefix):
    """Regions placed inside each repeat class and next to an anchor (fm_plan_check.cpp's format)."""
    _, contigs = fmcheck.read_ann(prefix)
    text = fmcheck.doubled_text(prefix)
    s = "".join("ACGT"[c] for c in text[:len(text) // 2])
    off2 = contigs[1][1]
    tandem = s.find("ACGGTCATTGCAGTACCTGATCGA" * 4) - off2
    polya = s.find("A" * 40) - off2
    cases = []
    for ln in (120, 250, 300):
        cases.append((1, 5000, 1, 5200, ln))                      # the true continuation: unique hits next to both anchors
        cases.append((2, 400, 2, 600, ln))
        cases.append((2, tandem - 200, 2, tandem, ln))             # the tandem behind its own left flank: > 500 and, near its end, fewer rows
        cases.append((2, tandem - 200 + 24 * 690, 2, tandem + 24 * 690, ln))
        cases.append((1, 9000, 2, tandem + 2400, ln))              # the tandem with both anchors on the other contig
        cases.append((2, polya - 230, 2, polya - 30, ln))          # into the A run: 101 .. 500 rows, next to the anchors
        cases.append((1, 12000, 2, polya + 10, ln))                # the A run, anchors elsewhere
        cases.append((1, 700, 1, 30000, ln))                       # unique sequence from elsewhere on the contig, within SV_len_thd or not
        cases.append((2, 1000, 1, 200 + 0, ln))
    u = s.find(s[200:264])                                         # the 64-bp unit: its first copy begins at offset 200 of contig 1
    assert u == 200
    for ln in (64, 150):
        cases.append((1, 0, 1, 200, ln))                           # a unit copy (150 rows) next to the anchor, and far from it
        cases.append((2, 20000, 1, 200, ln))
    return cases


def test_planner_from_both_seed_sources(repeat, tmp_path):
    """(c) rescue_plan (host FmIndex, a row located when asked for) and rescue_windows / lamsa_hp_fm_search / rescue_plan_found on the
    repeat genome, in a program of its own under ASan and UBSan: identical plans and job lists."""
    prefix, chk = repeat
    exe = fmlib.plan_check_bin()
    cases = _plan_cases(prefix)
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for c in cases:
            f.write("%d %d %d %d %d\n" % c)
    p = subprocess.run([exe, prefix, path], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-3000:])
    regions, lines, jobs, kmers, located = [int(x) for x in p.stdout.split()[1:6]]
    assert regions == len(cases) and lines >= len(cases) // 2 and jobs >= lines and located > 10000, p.stdout


@pytest.mark.parametrize("name", ["c7_rescue", "c8_rescue_ont"])
def test_cli_rescue_gpu_on_the_emulation(name, tmp_path):
    """(d) The emulated host program with emu_fm.cpp supplying the two calls: --rescue-gpu gives golden_full.sam (chunks of 5 reads on 3
    threads; c7_rescue also in one chunk, and with -R 0, where there is nothing to do); built without emu_fm.cpp it prints its note,
    searches on the host and gives the same."""
    ref, reads, args, want_r0 = G.stage_scenario(name, str(tmp_path))
    want = G.strip_pg(G.golden_full(name))
    cli = fmlib.emu_cli_fm()
    for extra in ([["--batch", "5", "-t", "3"], []] if name == "c7_rescue" else [["--batch", "5", "-t", "3"]]):
        p = subprocess.run([cli, "aln", "-N", "--rescue-gpu"] + extra + args + [ref, reads], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        assert "lamsa_hp_fm_load" not in p.stderr
        assert G.strip_pg(p.stdout) == want
    if name == "c7_rescue":
        p = subprocess.run([cli, "aln", "-N", "--rescue-gpu", "-R", "0"] + args + [ref, reads], capture_output=True, text=True)
        assert p.returncode == 0 and G.strip_pg(p.stdout) == G.strip_pg(want_r0), p.stderr[-2000:]
    q = subprocess.run([reflib.emu_cli(), "aln", "-N", "--rescue-gpu"] + args + [ref, reads], capture_output=True, text=True)
    assert q.returncode == 0, q.stderr[-2000:]
    assert "no lamsa_hp_fm_load / lamsa_hp_fm_search" in q.stderr
    assert G.strip_pg(q.stdout) == want
