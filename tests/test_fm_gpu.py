"""The device FM index on the MI355X: lamsa_hp_fm_load / lamsa_hp_fm_search (k_fm_search, k_fm_locate, the scan between them) against
the independent checker of tests/fmcheck.py on the query sets of tests/test_fm_cpu.py, the error returns, and `lamsa aln --rescue-gpu`
of the product binary on the golden scenarios."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fmcheck
import fmlib
import goldenlib as G
from lamsa_amd import hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lamsa_amd", "bin", "lamsa")
GOLD_REF = os.path.join(G.GOLD, "ref", "ref.fa")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    d = tmp_path_factory.mktemp("repeat")
    fa = str(d / "rep.fa")
    fmlib.write_repeat_genome(fa)
    fmlib.index_genome(BIN, fa)
    return {"golden": (GOLD_REF, fmcheck.FmCheck(GOLD_REF)), "repeat": (fa, fmcheck.FmCheck(fa))}


@pytest.fixture(scope="module")
def handles(genomes):
    """One handle per genome, created without a reference as the stage-4 handle is."""
    hs = {}
    for name, (prefix, _) in genomes.items():
        hs[name] = hp.LamsaHp(hp.make_para(), device=0)
        hs[name].fm_load(prefix)
    yield hs
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("k", fmlib.KS)
@pytest.mark.parametrize("genome", ["golden", "repeat"])
def test_search_against_the_checker(genome, k, genomes, handles):
    """lo, hi, pos_off and pos word for word the checker's, with max_occ 100, 500, one that a k-mer of the set meets exactly and another
    exceeds by one, and 0 (intervals only); on the repeat genome the set holds every class of k-mer and row (k = 1: only the classes a
    1-mer can be in, see tests/test_fm_cpu.py)."""
    prefix, chk = genomes[genome]
    h = handles[genome]
    seq, win_off = fmlib.make_queries(chk, k, seed=7 * k + 1, repeat_genome=genome == "repeat")
    cnt = chk.search(seq, win_off, k, 0)[5]
    m_star = fmlib.pick_max_occ(cnt)
    for max_occ in (100, 500, m_star, 0):
        if max_occ is None:
            continue
        fmlib.assert_same(h.fm_search(seq, win_off, k, max_occ), chk.search(seq, win_off, k, max_occ), (genome, k, max_occ))
    if genome != "repeat":
        return
    cl = fmlib.classes(seq, win_off, k, cnt, m_star if m_star is not None else -9)
    print(k, m_star, cl)
    assert cl["many"] > 0 and cl["code4"] > 0 and cl["a_run"] > 0, cl
    if k > 1:
        want = chk.search(seq, win_off, k, 500)
        assert m_star is not None and all(v > 0 for v in cl.values()), (m_star, cl)
        lo, hi = fmlib.rows_queried(want[1], want[2], cnt, 500)
        for row in (1, chk.n, chk.primary - 1, chk.primary, chk.primary + 1):
            assert fmlib.covers(lo, hi, row), row
        stored = lambda r: r - (r >= chk.primary)
        assert fmlib.covers_where(lo, hi, lambda r: r % 32 == 0)
        assert fmlib.covers_where(lo, hi, lambda r: r != chk.primary and stored(r) % 128 == 0)
        assert fmlib.covers_where(lo, hi, lambda r: r != chk.primary and stored(r) % 128 == 127)


def test_odd_sizes_no_windows_twice_and_slices(genomes, handles, monkeypatch):
    """A set whose k-mers are no multiple of 64; zero windows; the same call twice in a row on one handle; the locate pass in slices of
    1000 positions (LAMSA_HP_FM_SLICE): the same words every time."""
    prefix, chk = genomes["repeat"]
    h = handles["repeat"]
    seq, win_off = fmlib.make_queries(chk, 19, seed=3)
    sub = win_off[:12]
    want = chk.search(seq, sub, 19, 500)
    assert len(want[1]) % 64 != 0
    fmlib.assert_same(h.fm_search(seq, sub, 19, 500), want, "odd")
    got = h.fm_search(seq, win_off[:1], 19, 500)
    assert len(got[1]) == 0 and got[3].tolist() == [0] and got[0].tolist() == [0]
    got = h.fm_search(np.zeros(0, np.uint8), np.zeros(1, np.int64), 19, 500)
    assert len(got[1]) == 0
    want = chk.search(seq, win_off, 19, 500)
    for rep in range(2):
        fmlib.assert_same(h.fm_search(seq, win_off, 19, 500), want, "twice")
    monkeypatch.setenv("LAMSA_HP_FM_SLICE", "1000")
    assert len(want[4]) > 3000
    fmlib.assert_same(h.fm_search(seq, win_off, 19, 500), want, "slices")


def test_error_returns(genomes):
    """LAMSA_HP_EINVAL for a search before a load, k outside 1..255, a negative max_occ, offsets that decrease or leave seq_bytes and an
    index whose sizes contradict each other; LAMSA_HP_ENOMEM for an index no device holds; the handle works afterwards."""
    prefix, chk = genomes["repeat"]
    L = hp.load_library()
    h = hp.LamsaHp(hp.make_para(), device=0)
    seq, win_off = fmlib.make_queries(chk, 19, seed=5)
    EINVAL, ENOMEM = -2, -3
    assert fmlib.fm_search_lib(L, h._h, seq, win_off, 19, 500)[0] == EINVAL            # nothing loaded
    ix, keep = hp.read_fm_index(prefix)

    def changed(**kw):
        c = hp.HpFmIndex()
        C.memmove(C.byref(c), C.byref(ix), C.sizeof(ix))
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    for bad in (changed(n_sa=ix.n_sa - 1), changed(bwt_words=ix.bwt_words // 2), changed(seq_len=ix.seq_len + 64), changed(sa_intv=24), changed(primary=0), changed(bwt=None)):
        assert L.lamsa_hp_fm_load(h._h, C.byref(bad)) == EINVAL
        assert fmlib.fm_search_lib(L, h._h, seq, win_off, 19, 500)[0] == EINVAL        # a failed load leaves no index
    big = hp.HpFmIndex()
    big.seq_len = 1 << 46; big.primary = 1; big.sa_intv = 32
    for c in range(1, 5):
        big.L2[c] = big.seq_len
    big.bwt_words = ((big.seq_len + 15) >> 4) + ((big.seq_len + 127) >> 7) * 8; big.n_sa = (big.seq_len + 32) // 32
    big.bwt = ix.bwt; big.sa = ix.sa                                                   # never read: the allocation is refused first
    assert L.lamsa_hp_fm_load(h._h, C.byref(big)) == ENOMEM
    h.fm_load(prefix)
    want = chk.search(seq, win_off, 19, 500)
    for k, max_occ in ((0, 500), (256, 500), (-1, 500), (19, -1)):
        assert fmlib.fm_search_lib(L, h._h, seq, win_off, k, max_occ)[0] == EINVAL
    down = win_off.copy(); down[3] = down[2] - 1
    assert fmlib.fm_search_lib(L, h._h, seq, down, 19, 500)[0] == EINVAL
    assert fmlib.fm_search_lib(L, h._h, seq[:int(win_off[-1]) - 1], win_off, 19, 500)[0] == EINVAL
    neg = win_off.copy(); neg[0] = -1
    assert fmlib.fm_search_lib(L, h._h, seq, neg, 19, 500)[0] == EINVAL
    fmlib.assert_same(h.fm_search(seq, win_off, 19, 500), want, "after the errors")
    h.fm_load(GOLD_REF)                                                                # a second load replaces the index
    gchk = genomes["golden"][1]
    gs, gw = fmlib.make_queries(gchk, 19, seed=9, repeat_genome=False)
    fmlib.assert_same(h.fm_search(gs, gw, 19, 500), gchk.search(gs, gw, 19, 500), "replaced")
    h.close()


_plain = {}


def _run_bin(name, d, extra):
    ref, reads, args, _ = G.stage_scenario(name, d)
    p = subprocess.run([BIN, "aln", "-N", "-t", "4"] + extra + args + [ref, reads], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "searches on the host" not in p.stderr
    return G.strip_pg(p.stdout)


@pytest.mark.parametrize("extra", [[], ["--batch", "4"], ["--devices", "0,0"]], ids=["plain", "batch4", "two_handles"])
@pytest.mark.parametrize("name", G.SCENARIOS)
def test_product_binary_rescue_gpu(name, extra, tmp_path):
    """`lamsa aln --rescue-gpu` prints what the run without the option prints (one such run per scenario, shared; on the rescue scenarios
    it is golden_full.sam), also in batches of 4 reads and on two handles of device 0."""
    if name not in _plain:
        _plain[name] = _run_bin(name, str(tmp_path), [])
        if name in G.RESCUE_SCENARIOS:
            assert _plain[name] == G.strip_pg(G.golden_full(name))
    assert _run_bin(name, str(tmp_path), ["--rescue-gpu"] + extra) == _plain[name]
