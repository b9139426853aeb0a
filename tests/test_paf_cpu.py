"""LAMSA_HP_TAG_SUMMARY / --paf / --paf-cg without a GPU: the checker itself (tests/pafcheck.py) on hand-made SAM, one record through the
device's out_line under the CPU lane emulation, the whole emulated per-read path with the flag (phased, and one-kernel at scale 8)
against the checker's summaries of the flag-off stream, and the emulated host program, whose C-ABI has no lamsa_hp_set_result_tags:
there the host makes the summaries from the CIGARs (rec_summary).  tests/test_paf_gpu.py checks the words the HIP kernels make.

No golden scenario has a record with an I next to a D (the DP routines emit none, and the junctions between fragments are M-bounded), so
that counter is fed by hand-made cases here -- the checker's, and a record with such a pair through out_line -- and asserted on those."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import goldenlib as G
import pafcheck as P
import reflib

TAG_MISMATCHES, TAG_EQX, TAG_LEFT_ALIGN, TAG_SUMMARY = 1, 2, 8, 32
EINVAL = -2


def words_of(text):
    return [int(n) << 4 | "MIDNSHP=X".index(o) for n, o in P._CIG.findall(text)]


# ---------------------------------------------------------------- 1. the checker on hand-made SAM
HAND_SAM = "\n".join([
    "@SQ\tSN:c1\tLN:1000", "@SQ\tSN:c2\tLN:500", "@PG\tID:x",
    # '+' with soft clips on both ends, an I next to a D, and two XA alternatives (one '-', one with an =/X CIGAR)
    "r1\t0\tc1\t101\t37\t5S20M2I3D10M3S\t*\t0\t0\t" + "A" * 40 + "\t*\tNM:i:7\tAS:i:11\tXA:Z:c2,-11,3S30M7S,4;c1,+301,4S10=1X25=,1;\tMD:Z:20^ACG3T6\tcs:Z::20+aa-acg:3*ta:6",
    # '-' with a hard clip in front: the clips swap
    "r1\t2064\tc2\t11\t9\t30H6M4S\t*\t0\t0\tACGTAC\t*\tNM:i:0\tAS:i:6",
    # an =/X CIGAR; de = 1 / 3000 = 0.000333.. -> 0.0003, and 5 / 10000 -> 0.0005
    "r2\t16\tc1\t1\t60\t1000=1X1999=\t*\t0\t0\t*\t*\tNM:i:1\tAS:i:2990",
    "r3\t0\tc1\t1\t60\t10000M\t*\t0\t0\t*\t*\tNM:i:5\tAS:i:9000",
    # 0.00045 is not a binary fraction: 9 / 20000 prints as 0.0004 or 0.0005 by the double's value, which '%.4f' decides alike everywhere
    "r4\t0\tc1\t1\t60\t20000M\t*\t0\t0\t*\t*\tNM:i:9\tAS:i:1",
    # rounding up at the fourth digit: 7 / 10001 = 0.00069993 -> 0.0007
    "r5\t0\tc1\t1\t60\t10001M\t*\t0\t0\t*\t*\tNM:i:7\tAS:i:1",
    "u\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*"]) + "\n"


def test_checker_on_hand_made_sam():
    cl = P.contig_lengths(HAND_SAM)
    assert cl == {"c1": 1000, "c2": 500}
    st = P.new_stats()
    got = P.sam_to_paf(HAND_SAM, cl, False, st).split("\n")
    assert got[0] == "r1\t40\t5\t37\t+\tc1\t1000\t100\t133\t28\t35\t37\ttp:A:P\tNM:i:7\tAS:i:11\tde:f:0.1250"        # n_mm 2; (2 + 2) / (30 + 2)
    assert got[1] == "r1\t40\t7\t37\t-\tc2\t500\t10\t40\t26\t30\t0\ttp:A:S\tNM:i:4\tde:f:0.1333"
    assert got[2] == "r1\t40\t4\t40\t+\tc1\t1000\t300\t336\t35\t36\t0\ttp:A:S\tNM:i:1\tde:f:0.0278"
    assert got[3] == "r1\t40\t4\t10\t-\tc2\t500\t10\t16\t6\t6\t9\ttp:A:P\tNM:i:0\tAS:i:6\tde:f:0.0000"
    assert got[4].split("\t")[1:5] == ["3000", "0", "3000", "-"] and got[4].endswith("de:f:0.0003")
    assert got[5].endswith("de:f:0.0005")
    assert got[6].endswith("de:f:%.4f" % (9 / 20000))
    assert got[7].endswith("de:f:0.0007")
    assert got[8:] == [""]                                             # nothing for the unmapped read, no header
    assert st == {"minus": 3, "both_clips": 3, "multi_rec": 0, "long_cigar": 0, "adjacent_id": 1, "xa": 2}
    cg = P.sam_to_paf(HAND_SAM, cl, True).split("\n")
    assert cg[0] == got[0] + "\tcg:Z:20M2I3D10M\tMD:Z:20^ACG3T6\tcs:Z::20+aa-acg:3*ta:6"
    assert cg[1] == got[1] + "\tcg:Z:30M" and cg[2] == got[2] + "\tcg:Z:10=1X25=" and cg[3] == got[3] + "\tcg:Z:6M"
    # the stream side of the checker: one line of two records, the second '-' with an I next to a D
    class Para:
        match, mis, ins_gapo, ins_gape, del_gapo, del_gape = 1, 3, 2, 1, 3, 2
    c1, c2 = words_of("5S20M2I3D10M3S"), words_of("32S6M2S")
    plain = [0, 1, 0, 5, 0, 0, 2] + [101, 0, 1, 1, 28 - 6 - 2 - 2 - 3 - 6, 7, len(c1)] + c1 + [11, 0, 2, 0, 6, 0, len(c2)] + c2
    st = P.new_stats()
    want = P.stream_summaries(plain, 40, Para, st)
    assert want == [0, 1, 0, 5, 0, 0, 2] + [101, 0, 1, 1, 9, 7, 6, 6, 37, 33, 30, 2, 3, 1, 1] + [11, 0, 2, 0, 6, 0, 3, 3, 8, 6, 6, 0, 0, 0, 0]
    assert st == {"minus": 1, "both_clips": 2, "multi_rec": 1, "long_cigar": 0, "adjacent_id": 1, "xa": 0}
    assert P.stream_summaries([4, 0, 0], 40) == [4, 0, 0]
    with pytest.raises(AssertionError):                               # NM below the gap bases: the first identity
        P.stream_summaries(plain[:12] + [4] + plain[13:], 40)
    with pytest.raises(AssertionError):                               # a score that is not the formula's: the second
        P.stream_summaries(plain[:11] + [10] + plain[12:], 40, Para)


# ---------------------------------------------------------------- 2. the device code under the lane emulation
_lib = None


def emu_summary():
    """tests/emu/emu_summary.cpp (which includes emu_eqx.cpp and with it emu_api.cpp) compiled the way reflib.emu() compiles emu_api.cpp."""
    global _lib
    if _lib is None:
        os.makedirs(reflib.EMU_DIR, exist_ok=True)
        out = os.path.join(reflib.EMU_DIR, "libhp_emu_summary.so")
        root = reflib.ROOT
        srcs = [os.path.join(root, "tests", "emu", "emu_summary.cpp")]
        deps = srcs + [os.path.join(root, "tests", "emu", f) for f in ("emu_eqx.cpp", "emu_api.cpp", os.path.join("hp", "wave.h"))] + \
            [os.path.join(root, "include", "lamsa_hp.h")] + \
            [os.path.join(root, "lamsa_amd", "csrc", f) for f in os.listdir(os.path.join(root, "lamsa_amd", "csrc")) if f.endswith(".h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.run(["g++"] + reflib.EMU_FLAGS + ["-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                            "-I", os.path.join(root, "tests", "emu"), "-I", os.path.join(root, "lamsa_amd", "csrc"),
                            "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", out] + srcs, check=True, cwd=reflib.EMU_DIR)
        _lib = C.CDLL(out)
    return _lib


SENTINEL = 0x5eed5eed
ST_OVERFLOW = 1


def test_out_line_writes_fifteen_words():
    """One record through out_line with the flag: 4 line words and the 15 of the record, nothing behind them, and no word at all when a
    single one is missing (ST_OVERFLOW)."""
    E = emu_summary()
    E.emu_summary_record.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    cig = np.array(words_of("5S20M2I3D10M3S") * 30, np.int32)           # 180 elements: none of them may reach the output
    hdr = np.array([-5, 3, 2, 0, 77, 9], np.int32)                      # (an offset above 2^32, its low word negative as an int32)
    summ = np.array([4, 37, 33, 30, 2, 3, 1, 1], np.int32)
    for cap, ok in ((19, True), (18, False), (64, True)):
        buf = np.full(cap + 2, SENTINEL, np.int32)
        n = C.c_int32(0)
        st = E.emu_summary_record(hdr.ctypes.data, cig.ctypes.data, len(cig), summ.ctypes.data, buf[1:].ctypes.data, cap, C.byref(n))
        assert buf[0] == SENTINEL and (buf[1 + max(n.value, 4):] == SENTINEL).all(), cap
        if ok:
            assert st == 0 and n.value == 19
            assert buf[1:20].tolist() == [0, 0, 0, 1] + hdr.tolist() + [len(cig)] + summ.tolist()
        else:
            assert st & ST_OVERFLOW and n.value == 4


def _hp_para(lp):
    from lamsa_amd.hp import HpPara
    Q = HpPara()
    for n, _ in HpPara._fields_:
        setattr(Q, n, getattr(lp, n))
    return Q


def _emu_streams_tags(batch, hp_para, tags, scale=1, phased=True, slab_bytes=256 << 20):
    from lamsa_amd.hp import HpRef, HpBatch
    E = emu_summary()
    E.emu_lds_guard_reset()
    n = batch.n_reads
    hb = reflib.hp_batch_struct(batch, HpBatch)
    hr = HpRef(batch.pac.ctypes.data, int(batch.l_pac), len(batch.seq_len), batch.seq_off.ctypes.data, batch.seq_len.ctypes.data)
    cap = 4096 + 64 * n + 24 * int(batch.read_off[-1]) * scale
    stream = np.full(cap, SENTINEL, np.int32); nw = C.c_int64(-1)
    off = np.zeros(max(n, 1), np.int64); ln = np.zeros(max(n, 1), np.int32); st = np.zeros(max(n, 1), np.int32)
    E.emu_align_batch_checked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = E.emu_align_batch_checked(C.byref(hp_para), C.byref(hr), C.byref(hb), scale, 1 if phased else 0, tags, slab_bytes, stream.ctypes.data, cap, C.byref(nw), off.ctypes.data, ln.ctypes.data, st.ctypes.data)
    if rc != 0:
        assert nw.value == -1 and (stream == SENTINEL).all()            # refused: nothing ran
        return rc, None
    E.emu_lds_guard_hits.restype = C.c_longlong
    assert E.emu_lds_guard_hits() == 0
    assert (stream[nw.value:] == SENTINEL).all()
    return reflib.split_streams(stream, off[:n], ln[:n]), st[:n].copy()


EMU_STATS = P.new_stats()


@pytest.mark.parametrize("name", G.SCENARIOS)
def test_whole_path_under_the_emulation(name, tmp_path):
    ref, reads, args, _ = G.stage_scenario(name, str(tmp_path))
    rt, over = G.para_from_args(args)
    lp = reflib.lo_para(rt, **over)
    B = reflib.Batch(ref, reads, lp)
    Q = _hp_para(lp)
    L = [int(B.read_off[r + 1] - B.read_off[r]) for r in range(B.n_reads)]
    plain, st0 = _emu_streams_tags(B, Q, 0)
    assert plain == reflib.oracle_streams(B, lp)
    want = [P.stream_summaries(plain[r], L[r], Q, EMU_STATS) for r in range(B.n_reads)]
    assert want != plain
    for scale, phased in ((1, True), (8, False)):
        got, st = _emu_streams_tags(B, Q, TAG_SUMMARY, scale, phased)
        assert (st == st0).all(), (scale, phased)
        assert [r for r in range(B.n_reads) if got[r] != want[r]] == [], (scale, phased)
        both, st = _emu_streams_tags(B, Q, TAG_SUMMARY | TAG_LEFT_ALIGN, scale, phased)
        assert (st == st0).all() and both == got, (scale, phased)
    if name == "c1_perfect":
        for flags in (TAG_SUMMARY | TAG_MISMATCHES, TAG_SUMMARY | TAG_EQX, TAG_SUMMARY | TAG_EQX | TAG_MISMATCHES, 4, 16, 64, TAG_SUMMARY | 4, 128):
            assert _emu_streams_tags(B, Q, flags)[0] == EINVAL, flags
        E = emu_summary()
        assert [f for f in range(256) if E.emu_result_tags_valid(f)] == [0, 1, 2, 3, 8, 9, 10, 11, 32, 40]


def test_the_emulated_streams_exercise_the_cases():
    """(after the scenarios above, which feed the counters)"""
    st = EMU_STATS
    assert st["minus"] > 0 and st["both_clips"] > 0 and st["multi_rec"] > 0 and st["long_cigar"] > 0, st
    hand = P.new_stats()
    P.summary_words(words_of("5S20M2I3D10M3S"), 0, 40, hand)
    assert hand["adjacent_id"] == 1                                    # (no golden record has one: see the module docstring)


# ---------------------------------------------------------------- 3. the emulated host program (host fallback: rec_summary)
@pytest.fixture(scope="module")
def cli():
    return reflib.emu_cli()


def _run(cli, tmp_path, name, extra, rc=0):
    r, reads, a, gold = G.stage_scenario(name, str(tmp_path))
    p = subprocess.run([cli, "aln", "-N"] + extra + a + [r, reads], capture_output=True, text=True)
    assert p.returncode == rc, p.stderr[-2000:]
    return p.stdout, gold


CLI_STATS = P.new_stats()


@pytest.mark.parametrize("name", G.SCENARIOS)
def test_cli_paf_equals_the_golden_sam(cli, name, tmp_path):
    gold = G.stage_scenario(name, str(tmp_path))[3]
    cl = P.contig_lengths(gold)
    modes = [(["-R", "0"], gold)] + ([([], G.golden_full(name))] if name in G.RESCUE_SCENARIOS else [])
    for mode, sam in modes:
        out, _ = _run(cli, tmp_path, name, mode + ["--paf"])
        assert out == P.sam_to_paf(sam, cl, False, CLI_STATS), mode
        out, _ = _run(cli, tmp_path, name, mode + ["--paf-cg"])
        assert out == P.sam_to_paf(sam, cl, True), mode
    if name not in G.RESCUE_SCENARIOS:                                 # stage 4 finds nothing there: the default run prints the same
        out, _ = _run(cli, tmp_path, name, ["--paf"])
        assert out == P.sam_to_paf(gold, cl, False)


@pytest.mark.parametrize("name", ["c2_pacbio", "c5_sv", "c7_rescue", "c8_rescue_ont"])
def test_cli_paf_cg_with_the_tag_options(cli, name, tmp_path):
    """--paf-cg honours --eqx, --cs, --MD and --left-align as the SAM writer does: checked against the same binary's SAM."""
    opts = ["--eqx", "--cs", "--MD", "--left-align"]
    for mode in (["-R", "0"], []):
        sam, _ = _run(cli, tmp_path, name, mode + opts)
        out, _ = _run(cli, tmp_path, name, mode + opts + ["--paf-cg"])
        want = P.sam_to_paf(sam, P.contig_lengths(sam), True)
        assert out == want and "cg:Z:" in out and "=" in out and "\tMD:Z:" in out and "\tcs:Z:" in out
        # --left-align, -S and -C change no byte of --paf
        plain, _ = _run(cli, tmp_path, name, mode + ["--paf"])
        assert _run(cli, tmp_path, name, mode + ["--paf", "--left-align", "-S", "-C"])[0] == plain


def test_cli_counters():
    """(after the CLI tests above)"""
    st = CLI_STATS
    assert st["minus"] > 0 and st["both_clips"] > 0 and st["long_cigar"] > 0 and st["xa"] > 0, st
    hand = P.new_stats()
    P.sam_to_paf(HAND_SAM, P.contig_lengths(HAND_SAM), False, hand)
    assert hand["adjacent_id"] == 1


def test_cli_batches_shards_hits_and_output_file(cli, tmp_path):
    r, reads, a, gold = G.stage_scenario("c7_rescue", str(tmp_path))
    for opt in ("--paf", "--paf-cg"):
        base = subprocess.run([cli, "aln", "-N", opt] + a + [r, reads], capture_output=True, text=True)
        assert base.returncode == 0 and base.stdout == P.sam_to_paf(G.golden_full("c7_rescue"), P.contig_lengths(gold), opt == "--paf-cg")
        p = subprocess.run([cli, "aln", "-N", "--batch", "4", opt] + a + [r, reads], capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout == base.stdout
        parts = [subprocess.run([cli, "aln", "-N", "--shard", "%d/2" % i, opt] + a + [r, reads], capture_output=True, text=True) for i in range(2)]
        assert all(q.returncode == 0 for q in parts) and parts[0].stdout and parts[1].stdout
        assert parts[0].stdout + parts[1].stdout == base.stdout
        hits = str(tmp_path / "h.bin")
        p = subprocess.run([cli, "aln", "-N", "--devices", "0,0", "--batch", "3", "--save-hits", hits, opt] + a + [r, reads], capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout == base.stdout
        outf = str(tmp_path / "o.paf")
        p = subprocess.run([cli, "aln", "--hits", hits, "-o", outf, "-t", "3", opt] + a + [r, reads], capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout == "" and open(outf).read() == base.stdout


def test_cli_refused_option_sets(cli, tmp_path):
    r, reads, a, _ = G.stage_scenario("c1_perfect", str(tmp_path))
    for extra in (["--paf", "--SA"], ["--paf-cg", "--SA"], ["--paf", "--MD"], ["--paf", "--cs"], ["--paf", "--eqx"], ["--paf", "--paf-cg"]):
        p = subprocess.run([cli, "aln", "-N"] + extra + a + [r, reads], capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and "[lamsa_aln]" in p.stderr and "Mapping reads" not in p.stderr, extra
    # and without the two options every byte is what it was
    out, gold = _run(cli, tmp_path, "c1_perfect", ["-R", "0"])
    assert G.strip_pg(out) == G.strip_pg(gold)
