"""Seeding in the FM index without a GPU: lamsa_amd/csrc/hp_seed.h under the lane emulation (tests/emu/emu_seed.cpp) against the
independent checker (tests/seedcheck.py over tests/fmcheck.py), the batch through the oracle and the emulated read path, the error
returns, the sanitizer program (tests/host/seed_check.cpp), and `lamsa aln --seed-fm` of the emulated host program against the same
binary -- and, where it was built, the reference's -- run with -N on the GEM map text the checker wrote.  tests/test_seed_gpu.py runs the
same reads on the MI355X."""
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

GOLD_REF = os.path.join(G.GOLD, "ref", "ref.fa")
REF_BIN = os.path.join(reflib.ROOT, "oracle", "_ref", "lamsa")
EINVAL = -2


@pytest.fixture(scope="module")
def repeat(tmp_path_factory):
    d = tmp_path_factory.mktemp("seedrep")
    fa = str(d / "rep.fa")
    seedlib.write_seed_genome(fa)
    fmlib.index_genome(reflib.emu_cli(), fa)
    chk = fmcheck.FmCheck(fa)
    contigs = fmcheck.read_ann(fa)[1]
    names, reads = seedlib.make_reads(chk, contigs)
    return dict(prefix=fa, chk=chk, contigs=contigs, names=names, reads=reads, want={})


def _want(g, prm):
    """The checker's batch for a parameter set, computed once and shared."""
    if prm not in g["want"]:
        reads = seedlib.short_reads(g["chk"])[1] if prm == seedlib.PARAMS_SHORT else g["reads"]
        g["want"][prm] = seedcheck.expected(g["chk"], g["contigs"], reads, *prm, prefix=g["prefix"])
    return g["want"][prm]


@pytest.fixture(scope="module")
def golden():
    return dict(prefix=GOLD_REF, chk=fmcheck.FmCheck(GOLD_REF), contigs=fmcheck.read_ann(GOLD_REF)[1])


@pytest.fixture(scope="module")
def emu(repeat):
    L = seedlib.emu_seed_lib()
    ix, keep = hp.read_fm_index(repeat["prefix"])
    assert L.lamsa_hp_fm_load(C.c_void_p(0x5000), C.byref(ix)) == 0
    return L, C.c_void_p(0x5000)


def _seed(emu, g, prm, want):
    so, sl = seedlib.contig_arrays(g["contigs"])
    return seedlib.fm_seed_lib(emu[0], emu[1], want.read_off, want.read_seq, *prm, so, sl)


def test_reads_meet_every_class(repeat):
    """The hand-placed reads hold every class of seed and row the definition tells apart: each is counted by the checker and none is
    empty -- over the parameter sets, and (except 'exactly max_hits rows', which is the 64-bp unit at max_hits = 150) in (50, 25, 149)
    alone.  The lengths: 0, seed_len - 1 and seed_len for 20, 50 and 63, (L - seed_len) % seed_step zero and not, an all-N read."""
    tot = {}
    for prm in seedlib.PARAMS:
        cl = _want(repeat, prm).classes
        print(prm, cl)
        for k, v in cl.items():
            tot[k] = tot.get(k, 0) + v
    assert all(v > 0 for v in tot.values()), tot
    assert _want(repeat, (50, 25, 150)).classes["e_at_max"] > 0
    c149 = _want(repeat, (50, 25, 149)).classes
    assert c149["e_at_max"] == 0 and c149["f_over_max"] > _want(repeat, (50, 25, 150)).classes["f_over_max"]
    assert all(v > 0 for k, v in c149.items() if k != "e_at_max"), c149
    lens = set(len(r) for r in repeat["reads"])
    assert {0, 19, 20, 49, 50, 62, 63} <= lens and any((r == 4).all() and len(r) for r in repeat["reads"])
    assert any((l - 50) % 25 == 0 and l > 50 for l in lens) and any((l - 50) % 25 != 0 and l > 50 for l in lens)
    w = _want(repeat, (50, 100, 200))
    assert ((w.seed_off[1:] - w.seed_off[:-1] == 0) & (w.seed_all > 0)).any()       # a read with seeds and no hit at all


@pytest.mark.parametrize("prm", seedlib.PARAMS + (seedlib.PARAMS_SHORT,), ids=lambda p: "%d_%d_%d" % p)
def test_emulated_seeding_against_the_checker(prm, repeat, emu):
    """The batch arrays of the emulated call word for word the checker's."""
    want = _want(repeat, prm)
    rc, got = _seed(emu, repeat, prm, want)
    assert rc == 0
    seedcheck.assert_batch(got, want, prm)


def test_slices_odd_sizes_no_reads_and_twice(repeat, emu, monkeypatch):
    """The locate pass in slices of 1000 rows (LAMSA_HP_FM_SLICE) and of 7, where most seeds with several rows straddle slices: the same
    words; a seed count that is no multiple of 64; zero reads; the same call twice in a row."""
    prm = (50, 25, 150)
    want = _want(repeat, prm)
    assert want.n_rows_located > 3000 and len(want._map["sid"]) % 64 != 0
    for slice_rows in (1000, 7):
        monkeypatch.setenv("LAMSA_HP_FM_SLICE", str(slice_rows))
        for rep in range(2):
            rc, got = _seed(emu, repeat, prm, want)
            assert rc == 0 and emu[0].emu_seed_last_slices() == (want.n_rows_located + slice_rows - 1) // slice_rows
            seedcheck.assert_batch(got, want, ("slices", slice_rows, rep))
    monkeypatch.delenv("LAMSA_HP_FM_SLICE")
    so, sl = seedlib.contig_arrays(repeat["contigs"])
    rc, got = seedlib.fm_seed_lib(emu[0], emu[1], np.zeros(1, np.int64), np.zeros(16, np.uint8), *prm, so, sl)
    assert rc == 0 and got["n_reads"] == 0 and got["n_cig"] == 0 and got["seed_off"].tolist() == [0] and got["hit_off"].tolist() == [0]
    rc, got = _seed(emu, repeat, prm, want)
    assert rc == 0
    seedcheck.assert_batch(got, want, "after zero reads")


def test_seeded_batch_through_the_oracle_and_the_emulated_read_path(repeat, emu):
    """reflib.oracle_streams on the checker's batch equals reflib.emu_streams on the emulated call's batch: the batch is one the read path
    takes, in its compact form, and aligns as the oracle aligns the checker's."""
    prm = (50, 100, 200)
    want = _want(repeat, prm)
    rc, got = _seed(emu, repeat, prm, want)
    assert rc == 0
    P = reflib.lo_para("default")
    assert (P.seed_len, P.seed_step, P.per_aln_m) == prm
    ref = reflib.oracle_streams(want, P)
    dev, st = reflib.emu_streams(seedcheck.as_batch(got, want), seedlib.hp_para_of(P))
    assert (st == 0).all() and dev == ref
    assert sum(1 for s in ref if s[1] > 0) > len(ref) // 2                      # most reads have lines


def test_error_returns(repeat, emu):
    """LAMSA_HP_EINVAL: no index loaded; seed_len outside 1..63, seed_step < 1, max_hits outside 1..16383; offsets that do not start at 0
    or that decrease; a read longer than 2^24; a base code above 4; a contig table that is empty, not contiguous, or of another genome.
    A working call after them."""
    L, key = emu
    want = _want(repeat, (50, 25, 150))
    so, sl = seedlib.contig_arrays(repeat["contigs"])
    ro, rs = want.read_off, want.read_seq

    def call(read_off=ro, read_seq=rs, prm=(50, 25, 150), seq_off=so, seq_len=sl, handle=key, n_reads=None):
        return seedlib.fm_seed_lib(L, handle, read_off, read_seq, *prm, seq_off, seq_len, n_reads=n_reads)[0]
    assert call(handle=C.c_void_p(0x5abc)) == EINVAL
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
    rc, got = _seed(emu, repeat, (50, 25, 150), want)
    assert rc == 0
    seedcheck.assert_batch(got, want, "after the errors")


def _write_fasta(path, names, reads):
    with open(path, "w") as f:
        for nm, r in zip(names, reads):
            f.write(">%s\n%s\n" % (nm, "".join("ACGTN"[x] for x in r)))


def test_sanitizer_program(repeat, tmp_path):
    """tests/host/seed_check.cpp, built with ASan and UBSan, on the hand-placed reads: every parameter set, slices of 7 and 1000 rows, each
    hit compared with the host's own FmIndex, the reads handed over without a byte to spare.  It ends clean."""
    exe = seedlib.seed_check_bin()
    fa = str(tmp_path / "reads.fa")
    _write_fasta(fa, repeat["names"], repeat["reads"])
    p = subprocess.run([exe, repeat["prefix"], fa], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-3000:])
    calls, seeds, slots, hits = [int(x) for x in p.stdout.split()[1:5]]
    assert calls == 11 and seeds > 10000 and slots > 5000 and hits > 30000, p.stdout


# ------------------------------------------------------------------ the host program
def _run(cmd):
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, (cmd, p.stderr[-2000:])
    return p


@pytest.mark.parametrize("name", ["c1_perfect", "c5_sv", "c6_edge"])
def test_cli_seed_fm_equals_the_run_on_the_checkers_map(name, golden, tmp_path):
    """The emulated host program with --seed-fm -R 0 prints what the same binary prints with -N on the GEM map text the checker wrote --
    also in chunks of 5 reads on 3 threads and as two shards -- and, where the compiled reference exists, what the reference's
    `lamsa aln -N -R 0` prints on that map, which pins the mode to the reference itself.  No mapper is started: there is no .gem index,
    no map file, and --gem-dir is an empty directory.  --save-hits then --hits gives the same SAM."""
    d = str(tmp_path)
    ref, reads, args, mp, want = seedlib.stage(name, d, golden)
    assert want.n_hits > 0
    cli = seedlib.emu_cli_seed()
    gem = ["--gem-dir", os.path.join(d, "nogem")]
    base = G.strip_pg(_run([cli, "aln", "--seed-result", mp, "-R", "0"] + args + [ref, reads]).stdout)
    assert sum(1 for l in base.split("\n") if l and not l.startswith("@") and l.split("\t")[2] != "*") > 0
    p = _run([cli, "aln", "--seed-fm", "-R", "0"] + gem + args + [ref, reads])
    assert G.strip_pg(p.stdout) == base
    assert "gem-mapper" not in p.stderr and not os.path.exists(reads + ".seed") and not os.path.exists(reads + ".seed.gem.map")
    p = _run([cli, "aln", "--seed-fm", "-R", "0", "--batch", "5", "-t", "3"] + gem + args + [ref, reads])
    assert G.strip_pg(p.stdout) == base
    parts = [_run([cli, "aln", "--seed-fm", "-R", "0", "--shard", "%d/2" % i] + gem + args + [ref, reads]).stdout for i in range(2)]
    assert G.strip_pg("".join(parts)) == base
    hits = os.path.join(d, "hits.bin")
    p = _run([cli, "aln", "--seed-fm", "-R", "0", "--batch", "7", "--save-hits", hits] + gem + args + [ref, reads])
    assert G.strip_pg(p.stdout) == base
    assert G.strip_pg(_run([cli, "aln", "--hits", hits, "-R", "0"] + args + [ref, reads]).stdout) == base
    _run([cli, "aln", "--seed-fm", "--parse-only"] + gem + args + [ref, reads])
    if os.path.exists(REF_BIN):
        import shutil
        shutil.copy(mp, reads + ".seed.gem.map")
        out = os.path.join(d, "ref.sam")
        q = subprocess.run([REF_BIN, "aln"] + args + ["-N", "-I", "-R", "0", "-o", out, ref, reads], capture_output=True, text=True, timeout=600)
        assert q.returncode == 0, q.stderr[-2000:]
        assert G.strip_pg(open(out).read()) == base


def test_cli_seed_fm_with_stage_4(golden, tmp_path):
    """c7_rescue with stage 4 on: --seed-fm equals the -N run on the checker's map, on the host search and with --rescue-gpu (where stage 4
    searches in the seeding handle, one call at a time)."""
    d = str(tmp_path)
    ref, reads, args, mp, want = seedlib.stage("c7_rescue", d, golden)
    cli = seedlib.emu_cli_seed()
    base = G.strip_pg(_run([cli, "aln", "--seed-result", mp] + args + [ref, reads]).stdout)
    for extra in ([], ["--rescue-gpu"], ["--rescue-gpu", "--batch", "5", "-t", "3"]):
        assert G.strip_pg(_run([cli, "aln", "--seed-fm"] + extra + args + [ref, reads]).stdout) == base, extra


def test_cli_refusals(golden, tmp_path):
    """--seed-fm with -N, --seed-result, --hits, --seed-first or -l above 63, without <ref>.bwt / <ref>.sa, or on a library without
    lamsa_hp_fm_seed: exit status 2 and a message, nothing written."""
    d = str(tmp_path)
    ref, reads, args, mp, want = seedlib.stage("c1_perfect", d, golden)
    cli = seedlib.emu_cli_seed()
    for extra in (["-N"], ["--seed-result", mp], ["--hits", mp], ["--seed-first"], ["-l", "64"]):
        p = subprocess.run([cli, "aln", "--seed-fm"] + extra + args + [ref, reads], capture_output=True, text=True)
        assert p.returncode == 2 and "--seed-fm" in p.stderr and p.stdout == "", (extra, p.returncode, p.stderr[-500:])
    p = subprocess.run([reflib.emu_cli(), "aln", "--seed-fm"] + args + [ref, reads], capture_output=True, text=True)
    assert p.returncode == 2 and "lamsa_hp_fm_seed" in p.stderr and p.stdout == ""
    os.remove(ref + ".sa")
    p = subprocess.run([cli, "aln", "--seed-fm"] + args + [ref, reads], capture_output=True, text=True)
    assert p.returncode == 2 and ".sa" in p.stderr and p.stdout == ""
