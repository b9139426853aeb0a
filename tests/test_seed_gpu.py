"""Seeding in the device FM index on the MI355X: lamsa_hp_fm_seed (k_seed_search, k_seed_locate, k_seed_hits, k_seed_slot, k_seed_emit
and the scans between them) against the independent checker of tests/seedcheck.py on the reads of tests/test_seed_cpu.py, the batch
through the read path, the error returns, and `lamsa aln --seed-fm` of the product binary against its own run with -N on the GEM map
text the checker wrote."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fmcheck
import fmlib
import goldenlib as G
import reflib
import seedcheck
import seedlib
from lamsa_amd import hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lamsa_amd", "bin", "lamsa")
GOLD_REF = os.path.join(G.GOLD, "ref", "ref.fa")
EINVAL = -2
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def repeat(tmp_path_factory):
    d = tmp_path_factory.mktemp("seedrep")
    fa = str(d / "rep.fa")
    seedlib.write_seed_genome(fa)
    fmlib.index_genome(BIN, fa)
    chk = fmcheck.FmCheck(fa)
    contigs = fmcheck.read_ann(fa)[1]
    names, reads = seedlib.make_reads(chk, contigs)
    h = hp.LamsaHp(hp.make_para(), device=0)              # created without a reference, as the host program's seeding handle is
    h.fm_load(fa)
    yield dict(prefix=fa, chk=chk, contigs=contigs, names=names, reads=reads, want={}, h=h)
    h.close()


@pytest.fixture(scope="module")
def golden():
    chk = fmcheck.FmCheck(GOLD_REF)
    contigs = fmcheck.read_ann(GOLD_REF)[1]
    h = hp.LamsaHp(hp.make_para(), device=0)
    h.fm_load(GOLD_REF)
    yield dict(prefix=GOLD_REF, chk=chk, contigs=contigs, h=h)
    h.close()


def _want(g, prm):
    if prm not in g["want"]:
        reads = seedlib.short_reads(g["chk"])[1] if prm == seedlib.PARAMS_SHORT else g["reads"]
        g["want"][prm] = seedcheck.expected(g["chk"], g["contigs"], reads, *prm, prefix=g["prefix"])
    return g["want"][prm]


def _seed(g, prm, want):
    so, sl = seedlib.contig_arrays(g["contigs"])
    return g["h"].fm_seed(want.read_off, want.read_seq, *prm, so, sl)


@pytest.mark.parametrize("prm", seedlib.PARAMS + (seedlib.PARAMS_SHORT,), ids=lambda p: "%d_%d_%d" % p)
def test_seeding_against_the_checker(prm, repeat):
    """The batch arrays of lamsa_hp_fm_seed word for word the checker's, on the repeat genome with the hand-placed reads, which hold
    every class of seed and row (tests/test_seed_cpu.py asserts that on the same reads)."""
    want = _want(repeat, prm)
    seedcheck.assert_batch(_seed(repeat, prm, want), want, prm)
    if prm == (50, 25, 149):
        assert all(v > 0 for k, v in want.classes.items() if k != "e_at_max"), want.classes
    if prm == (50, 25, 150):
        assert want.classes["e_at_max"] > 0


@pytest.mark.parametrize("prm", [(50, 100, 200), (50, 25, 200)], ids=lambda p: "%d_%d_%d" % p)
def test_seeding_on_the_golden_reference(prm, golden):
    """The reads of c1_perfect and c5_sv (200 reads, 0.9 Mbp) on the 400-kbp golden reference."""
    reads = []
    for name in ("c1_perfect", "c5_sv"):
        reads += [r for _, r in seedcheck.read_fasta(os.path.join(G.GOLD, name, "reads.fa.gz"))]
    want = seedcheck.expected(golden["chk"], golden["contigs"], reads, *prm)
    assert want.n_hits > 1000
    so, sl = seedlib.contig_arrays(golden["contigs"])
    seedcheck.assert_batch(golden["h"].fm_seed(want.read_off, want.read_seq, *prm, so, sl), want, prm)


def test_odd_sizes_no_reads_twice_and_slices(repeat, monkeypatch):
    """A seed count that is no multiple of 64; zero reads; the same call twice in a row on one handle; the locate pass in slices of 1000
    rows (LAMSA_HP_FM_SLICE) on a set that locates more than 3 000, and in slices of 7, where seeds straddle slices: the same words."""
    prm = (50, 25, 150)
    want = _want(repeat, prm)
    assert len(want._map["sid"]) % 64 != 0 and want.n_rows_located > 3000
    so, sl = seedlib.contig_arrays(repeat["contigs"])
    got = repeat["h"].fm_seed(np.zeros(1, np.int64), np.zeros(16, np.uint8), *prm, so, sl)
    assert got["n_reads"] == 0 and got["n_cig"] == 0 and got["seed_off"].tolist() == [0] and got["hit_off"].tolist() == [0]
    for rep in range(2):
        seedcheck.assert_batch(_seed(repeat, prm, want), want, ("twice", rep))
    for slice_rows in ("1000", "7"):
        monkeypatch.setenv("LAMSA_HP_FM_SLICE", slice_rows)
        seedcheck.assert_batch(_seed(repeat, prm, want), want, ("slices", slice_rows))


def test_seeded_batch_through_the_read_path(repeat):
    """align_batch of the returned batch equals reflib.oracle_streams of the checker's batch, status 0 everywhere; and two seeded chunks in
    flight through submit_batch / collect_batch give the same streams."""
    prm = (50, 100, 200)
    want = _want(repeat, prm)
    got = _seed(repeat, prm, want)
    lp = reflib.lo_para("default")
    assert (lp.seed_len, lp.seed_step, lp.per_aln_m) == prm
    ref = reflib.oracle_streams(want, lp)
    B = seedcheck.as_batch(got, want)
    h = hp.LamsaHp(hp.make_para(), ref=(want.pac, want.l_pac, want.seq_off, want.seq_len), device=0)
    dev, st = h.align_batch(B)
    assert (st == 0).all() and dev == ref
    # two chunks: the reads split in two, each seeded by a call of its own, both submitted before the first is collected
    n = want.n_reads; half = n // 2
    so, sl = seedlib.contig_arrays(repeat["contigs"])
    chunks = []
    for a, b in ((0, half), (half, n)):
        ro = (want.read_off[a:b + 1] - want.read_off[a]).astype(np.int64)
        rs = np.concatenate([want.read_seq[want.read_off[a]:want.read_off[b]], np.zeros(16, np.uint8)])
        g = repeat["h"].fm_seed(ro, rs, *prm, so, sl)
        chunks.append(seedcheck.as_batch(g, want)); chunks[-1].read_seq = rs
    h.submit_batch(chunks[0]); h.submit_batch(chunks[1])
    d0, s0 = h.collect_batch(); d1, s1 = h.collect_batch()
    h.close()
    assert (s0 == 0).all() and (s1 == 0).all() and d0 + d1 == ref


def test_error_returns(repeat):
    """LAMSA_HP_EINVAL: no index loaded; seed_len outside 1..63, seed_step < 1, max_hits outside 1..16383; offsets that do not start at 0
    or that decrease; a read longer than 2^24; a base code above 4; a contig table that is empty, not contiguous, or of another genome.
    The handle works afterwards."""
    L = hp.load_library()
    want = _want(repeat, (50, 25, 150))
    so, sl = seedlib.contig_arrays(repeat["contigs"])
    ro, rs = want.read_off, want.read_seq
    h = hp.LamsaHp(hp.make_para(), device=0)

    def call(read_off=ro, read_seq=rs, prm=(50, 25, 150), seq_off=so, seq_len=sl, n_reads=None):
        return seedlib.fm_seed_lib(L, h._h, read_off, read_seq, *prm, seq_off, seq_len, n_reads=n_reads)[0]
    assert call() == EINVAL                                    # nothing loaded
    h.fm_load(repeat["prefix"])
    for prm in ((0, 25, 150), (64, 25, 150), (50, 0, 150), (50, -3, 150), (50, 25, 0), (50, 25, 16384)):
        assert call(prm=prm) == EINVAL, prm
    bad = ro.copy(); bad[0] = 1
    assert call(read_off=bad) == EINVAL
    bad = ro.copy(); bad[5] = bad[4] - 1
    assert call(read_off=bad) == EINVAL
    assert call(read_off=np.array([0, (1 << 24) + 1], np.int64), read_seq=np.zeros(8, np.uint8)) == EINVAL      # refused before a base is read
    bad = rs.copy(); bad[100] = 5
    assert call(read_seq=bad) == EINVAL
    assert call(seq_off=so[:0], seq_len=sl[:0]) == EINVAL
    assert call(seq_off=so, seq_len=np.array([sl[0] - 1, sl[1]], np.int32)) == EINVAL
    assert call(seq_off=np.array([1, so[1]], np.int64)) == EINVAL
    assert call(seq_off=so[:1], seq_len=sl[:1]) == EINVAL                                                       # ends before the index's text does
    assert call(n_reads=-1) == EINVAL
    rc, got = seedlib.fm_seed_lib(L, h._h, ro, rs, 50, 25, 150, so, sl)
    assert rc == 0
    seedcheck.assert_batch(got, want, "after the errors")
    h.close()


# ------------------------------------------------------------------ the product binary
def _run(cmd, timeout=120):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (cmd, p.stderr[-2000:])
    return p


@pytest.mark.parametrize("name", ["c1_perfect", "c5_sv", "c6_edge"])
def test_product_binary_seed_fm(name, golden, tmp_path):
    """`lamsa aln --seed-fm` prints what the same binary prints with -N on the GEM map text the checker wrote: plain, in batches of 4
    reads, and on two handles of device 0.  The scenario is staged without a .gem index and without a map, --gem-dir is an empty
    directory: no gem-mapper is started and no seed file written."""
    d = str(tmp_path)
    ref, reads, args, mp, want = seedlib.stage(name, d, golden)
    gem = ["--gem-dir", os.path.join(d, "nogem")]
    base = G.strip_pg(_run([BIN, "aln", "--seed-result", mp, "-t", "4"] + args + [ref, reads]).stdout)
    assert sum(1 for l in base.split("\n") if l and not l.startswith("@") and l.split("\t")[2] != "*") > 0      # (c6_edge's noisy reads: few exact 50-mers, 22 mapped records)
    for extra in ([], ["--batch", "4"], ["--devices", "0,0"]):
        p = _run([BIN, "aln", "--seed-fm", "-t", "4"] + extra + gem + args + [ref, reads])
        assert G.strip_pg(p.stdout) == base, extra
        assert "gem-mapper" not in p.stderr and not os.path.exists(reads + ".seed") and not os.path.exists(reads + ".seed.gem.map")


def test_product_binary_seed_fm_with_rescue_gpu_and_paf(golden, tmp_path):
    """c7_rescue: --seed-fm with --rescue-gpu (stage 4 searches in the seeding handle's index) equals the -N run on the checker's map;
    and --paf once."""
    d = str(tmp_path)
    ref, reads, args, mp, want = seedlib.stage("c7_rescue", d, golden)
    gem = ["--gem-dir", os.path.join(d, "nogem")]
    base = G.strip_pg(_run([BIN, "aln", "--seed-result", mp, "-t", "4"] + args + [ref, reads]).stdout)
    p = _run([BIN, "aln", "--seed-fm", "--rescue-gpu", "-t", "4"] + gem + args + [ref, reads])
    assert G.strip_pg(p.stdout) == base and "searches on the host" not in p.stderr
    paf = _run([BIN, "aln", "--seed-result", mp, "--paf", "-t", "4"] + args + [ref, reads]).stdout
    assert paf and _run([BIN, "aln", "--seed-fm", "--paf", "-t", "4"] + gem + args + [ref, reads]).stdout == paf
