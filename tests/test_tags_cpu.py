"""--MD / --SA on the emulated host program (tests/emu): the tags pass the independent checker (tests/tagcheck.py), and with
them removed the output is the reference's byte for byte.  The emulated C-ABI has no lamsa_hp_set_result_tags, so here the
host derives the mismatch lists itself; tests/test_tags_gpu.py checks the device's lists."""
import os
import subprocess

import pytest

import goldenlib as G
import reflib
import tagcheck as T


@pytest.fixture(scope="module")
def cli():
    return reflib.emu_cli()


@pytest.fixture(scope="module")
def ref():
    return T.load_ref(os.path.join(G.GOLD, "ref", "ref.fa"))


def _run(cli, tmp_path, name, extra):
    r, reads, a, gold = G.stage_scenario(name, str(tmp_path))
    p = subprocess.run([cli, "aln", "-N"] + extra + a + [r, reads], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, gold


@pytest.mark.parametrize("name", G.SCENARIOS)
def test_tags_with_R0(cli, ref, name, tmp_path):
    out, gold = _run(cli, tmp_path, name, ["-R", "0", "--MD", "--SA"])
    assert G.strip_pg(T.strip_tags(out)) == G.strip_pg(gold)
    assert "\tMD:Z:" in out
    assert T.check_sam(out, *ref) == []


@pytest.mark.parametrize("name", G.SCENARIOS)
def test_tags_default_run(cli, ref, name, tmp_path):
    out, gold = _run(cli, tmp_path, name, ["--MD", "--SA", "--batch", "5"])
    want = G.golden_full(name) if name in G.RESCUE_SCENARIOS else gold
    assert G.strip_pg(T.strip_tags(out)) == G.strip_pg(want)
    assert T.check_sam(out, *ref) == []


def test_split_reads_carry_sa(cli, ref, tmp_path):
    """The SV scenarios have split reads: their records are linked, supplementary ones list the primary first; -S writes the same lists."""
    for extra in ([], ["-S"]):
        out, _ = _run(cli, tmp_path, "c9_rearr", ["-R", "0", "--SA"] + extra)
        recs = [l.split("\t") for l in out.split("\n") if l and not l.startswith("@")]
        sa = [f for f in recs if any(t.startswith("SA:Z:") for t in f[11:])]
        assert sa, "no SA tags"
        assert all(not any(t.startswith("MD:Z:") for t in f[11:]) for f in recs)
        if not extra:
            supp = [f for f in sa if int(f[1]) & 0x800]
            assert supp
            for f in supp:
                prim = next(g for g in recs if g[0] == f[0] and not int(g[1]) & 0x900)
                first = [t for t in f[11:] if t.startswith("SA:Z:")][0][5:].split(";")[0].split(",")
                assert first[:2] == [prim[2], prim[3]]
        else:
            assert not any(int(f[1]) & 0x800 for f in recs)
        assert T.check_sam(out, *ref) == []


def test_tags_with_devices_shards_and_hit_stream(cli, ref, tmp_path):
    """--devices, --shard, --save-hits / --hits give the same tagged output."""
    r, reads, a, gold = G.stage_scenario("c7_rescue", str(tmp_path))
    base = subprocess.run([cli, "aln", "-N", "--MD", "--SA"] + a + [r, reads], capture_output=True, text=True)
    assert base.returncode == 0 and T.check_sam(base.stdout, *ref) == []
    hits = str(tmp_path / "h.bin")
    p = subprocess.run([cli, "aln", "-N", "--batch", "2", "--devices", "0,0,0", "--MD", "--SA", "--save-hits", hits] + a + [r, reads], capture_output=True, text=True)
    assert p.returncode == 0 and G.strip_pg(p.stdout) == G.strip_pg(base.stdout)
    p = subprocess.run([cli, "aln", "--hits", hits, "--MD", "--SA"] + a + [r, reads], capture_output=True, text=True)
    assert p.returncode == 0 and G.strip_pg(p.stdout) == G.strip_pg(base.stdout)
    parts = [subprocess.run([cli, "aln", "-N", "--shard", "%d/2" % i, "--MD", "--SA"] + a + [r, reads], capture_output=True, text=True) for i in range(2)]
    assert all(q.returncode == 0 for q in parts)
    assert G.strip_pg(parts[0].stdout + parts[1].stdout) == G.strip_pg(base.stdout)


def _md_nm(cigar, seq, ref_seq):
    pac = bytearray((len(ref_seq) + 3) // 4 + 1)
    for k, c in enumerate(ref_seq):
        pac[k >> 2] |= "ACGT".index(c) << ((~k & 3) << 1)
    import numpy as np
    return T.md_nm(np.frombuffer(bytes(pac), np.uint8), 0, T.parse_cigar(cigar), seq)


def test_checker_on_hand_made_records():
    ref = "ACGTACGTAC" + "GGCCAATT" + "ACGTACGTAC"
    assert _md_nm("10M", "ACGTACGTAC", ref) == ("10", 0)
    assert _md_nm("10M", "TCGTACGTAG", ref) == ("0A8C0", 2)                       # mismatches at both ends
    assert _md_nm("4M2D4M", "ACGTGTAC", ref) == ("4^AC4", 2)
    assert _md_nm("4M2D4M", "ACGTCTAC", ref) == ("4^AC0G3", 3)                    # a deletion next to a mismatch
    assert _md_nm("3M2I3M", "ACGTTTAC", ref) == ("6", 2)                         # inserted bases: NM only
    assert _md_nm("4M", "ANGT", ref) == ("1C2", 1)                                # a read N is a mismatch
    assert _md_nm("3H4M5H", "ACGA", ref) == ("3T0", 1)                            # hard clips: SEQ holds the aligned bases only
    assert _md_nm("2S4M", "GGACGG", ref) == ("3T0", 1)
    sam = "\n".join(["@SQ\tSN:c\tLN:28",
                     "r\t0\tc\t1\t9\t4M6S\t*\t0\t0\tACGTTTTTTT\t*\tNM:i:0\tAS:i:4\tMD:Z:4\tSA:Z:c,11,-,4S6M,9,1;",
                     "r\t2064\tc\t11\t9\t4H6M\t*\t0\t0\tGGCCAT\t*\tNM:i:1\tAS:i:1\tMD:Z:5A0\tSA:Z:c,1,+,4M6S,9,0;",      # reverse strand, hard-clipped
                     "u\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*"]) + "\n"
    import numpy as np
    pac = bytearray(8)
    for k, c in enumerate(ref):
        pac[k >> 2] |= "ACGT".index(c) << ((~k & 3) << 1)
    pac = np.frombuffer(bytes(pac), np.uint8)
    assert T.check_sam(sam, pac, {"c": 0}) == []
    assert T.check_sam(sam.replace("MD:Z:5A0", "MD:Z:5A"), pac, {"c": 0})
    assert T.check_sam(sam.replace("SA:Z:c,1,+,4M6S,9,0;", "SA:Z:c,1,+,4M6H,9,0;"), pac, {"c": 0})
    assert T.check_sam(sam.replace("\tMD:Z:4\tSA:Z:c,11,-,4S6M,9,1;", "\tMD:Z:4"), pac, {"c": 0})
    assert T.check_sam(sam.replace("ACGT\t*\n", "ACGT\t*\tMD:Z:4\n"), pac, {"c": 0})


def test_stream_event_split():
    """The stream layout with mismatch lists (include/lamsa_hp.h) and its recomputation by the checker."""
    import numpy as np
    ref = "ACGTACGTACGGCCAATT"
    pac = bytearray(8)
    for k, c in enumerate(ref):
        pac[k >> 2] |= "ACGT".index(c) << ((~k & 3) << 1)
    pac = np.frombuffer(bytes(pac), np.uint8)
    read = [0, 1, 3, 3, 4, 1, 2, 3]                                    # ACTTNCGT against ACGTACGT at POS 1
    plain = [0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1, 5, 2, 1, 8 << 4]
    ev = T.stream_events(plain, read, pac, [0])
    assert ev == [[2 << 2 | 2, 4 << 2 | 0]]
    tagged = plain + [2] + ev[0]
    assert T.split_events(tagged) == (plain, ev)
