"""LAMSA_HP_TAG_LEFT_ALIGN / --left-align without a GPU: the checker itself (tests/lalcheck.py) on hand-made records, the device routine
(lamsa_amd/csrc/hp_lalign.h) under the CPU lane emulation on the same inputs and on random ones, the whole emulated per-read path
with the flag, and the emulated host program, whose C-ABI has no lamsa_hp_set_result_tags: there the host shifts the gaps itself
(rec_left_align).  tests/test_lalign_gpu.py checks the words the HIP kernels make."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import eqxcheck as X
import goldenlib as G
import lalcheck as LA
import reflib
import tagcheck as T

TAG_MISMATCHES, TAG_EQX, TAG_LEFT_ALIGN = 1, 2, 8


def _pac_of_codes(ref):
    pac = np.zeros(len(ref) // 4 + 2, np.uint8)
    for k, c in enumerate(ref):
        pac[k >> 2] |= int(c) << ((~k & 3) << 1)
    return pac


def _pac(ref_seq):
    return _pac_of_codes(["ACGT".index(c) for c in ref_seq])


def _codes(seq):
    return T.NT4[np.frombuffer(seq.encode(), np.uint8)]


def _la(cigar, seq, ref, k0=0, stats=None):
    return X.text_of(LA.left_align(X.words_of(cigar), _codes(seq), _pac(ref), k0, stats))


# the hand-made records: (name, CIGAR, read, reference, .pac coordinate of POS, the left-aligned CIGAR)
REP = "GATTACA" + "CAG" * 6 + "TTGC"


def _cascade():
    words = ["200M"] + ["1D", "1M"] * 149 + ["1D", "50M"]
    want = ["1M"] + ["1D", "1M"] * 149 + ["1D", "249M"]
    return "".join(words), "A" * 399, "A" * (399 + 150), "".join(want)


HAND = [
    # a deletion at the right end of a 200-base homopolymer, an M of 150 before it: the M keeps one base
    ("homopolymer", "150M1D8M", "A" * 150 + "CGTTGCAC", "C" * 7 + "A" * 200 + "CGTTGCAC", 7 + 49, "1M1D157M"),
    # a deletion of one period of a tandem repeat moves in steps of one base through the whole repeat
    ("tandem D", "22M3D4M", "GATTACA" + "CAG" * 5 + "TTGC", REP, 0, "7M3D19M"),
    ("tandem I", "25M3I4M", "GATTACA" + "CAG" * 7 + "TTGC", REP, 0, "7M3I22M"),
    # inserted read bases that are N: N equals N
    ("N insert", "4M2I4M", "ACNNNNACGT", "ACGTACGT", 0, "2M2I6M"),
    ("M of one", "1M1D5M", "AAAAAA", "AAAAAAA", 0, "1M1D5M"),
    ("after a clip", "3S2I5M", "AAAAAAAAAA", "AAAAA", 0, "3S2I5M"),
    ("after a clip, M between", "3S1M2I5M", "AAAAAAAAAAA", "AAAAAA", 0, "3S1M2I5M"),
    ("last aligned element", "5M2I3S", "AAAAAAAAAA", "AAAAA", 0, "5M2I3S"),
    ("last element", "5M2D", "AAAAA", "AAAAAAA", 0, "5M2D"),
    ("first element", "2D5M", "AAAAA", "AAAAAAA", 0, "2D5M"),
    # two adjacent gaps: both stay, and the gap after them stops in front of them
    ("adjacent gaps", "6M2I3D3M1D6M", "A" * 17, "A" * 19, 0, "6M2I3D1M1D8M"),
    ("mismatching bases", "4M1D4M", "ACGTCGTA", "ACGTACGTA", 0, "4M1D4M"),
]
_c = _cascade()
HAND.append(("cascade of 150", _c[0], _c[1], _c[2], 0, _c[3]))


# ---------------------------------------------------------------- 1. the checker on hand-made records
def test_checker_on_hand_made_records():
    for name, cigar, seq, ref, k0, want in HAND:
        st = LA.new_stats()
        got = _la(cigar, seq, ref, k0, st)
        assert got == want, name
        assert _la(got, seq, ref, k0) == got, name + ": not idempotent"
        assert LA.check_consequences(X.words_of(cigar), X.words_of(got)) == [], name
        pac = _pac(ref)
        md0, nm0 = T.md_nm(pac, k0, T.parse_cigar(cigar), seq)
        md1, nm1 = T.md_nm(pac, k0, T.parse_cigar(got), seq)
        assert nm0 == nm1, name
        # MD: the same mismatched bases in the same order, the same deleted bases or a rotation of them (a deletion that moved one base
        # left drops its last base and takes the one in front of it, which is the same base)
        assert re.sub(r"\^[A-Z]+|\d+", "", md0) == re.sub(r"\^[A-Z]+|\d+", "", md1), name
        assert [len(d) for d in re.findall(r"\^[A-Z]+", md0)] == [len(d) for d in re.findall(r"\^[A-Z]+", md1)], name
        if name == "homopolymer":
            assert st == {"gaps": 1, "moved": 1, "room": 1, "cascade": 0, "cascade_block": 0}
        if name == "cascade of 150":
            assert st["gaps"] == 150 and st["moved"] == 150 and st["room"] == 150 and st["cascade"] == 149 and st["cascade_block"] == 4      # 301 elements: the gaps at 65, 129, 193, 257
    # a mismatch inside the stretch a deletion moves across keeps its base and gets ref_off + k
    seq = "GATTACA" + "CAG" + "CTG" + "CAG" * 3 + "TTGC"
    pac = _pac(REP)
    plain = [0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1, 0, 0, 3] + X.words_of("22M3D4M")
    assert T.stream_events(plain, _codes(seq), pac, [0]) == [[11 << 2 | 0]]
    moved = LA.stream_left_aligned(plain, _codes(seq), pac, [0])
    assert moved == plain[:14] + X.words_of("7M3D19M")
    assert T.stream_events(moved, _codes(seq), pac, [0]) == [[14 << 2 | 0]]
    assert T.md_nm(pac, 0, T.parse_cigar("22M3D4M"), seq) == ("11A10^CAG4", 4) and T.md_nm(pac, 0, T.parse_cigar("7M3D19M"), seq) == ("7^CAG4A14", 4)
    # a '-' record aligns the reverse complement; the SAM text: field 6, XA:Z and SA:Z
    rc = "".join("TGCA"["ACGT".index(c)] for c in reversed("GATTACA" + "CAG" * 5 + "TTGC"))
    reads = {"r": "GATTACA" + "CAG" * 5 + "TTGC", "m": rc}
    sam = "\n".join(["@SQ\tSN:c\tLN:29",
                     "r\t0\tc\t1\t9\t22M3D4M\t*\t0\t0\t%s\t*\tNM:i:3\tAS:i:2\tXA:Z:c,+1,22M3D4M,3;\tSA:Z:c,1,+,22M3D4M,9,3;" % reads["r"],
                     "m\t16\tc\t1\t9\t22M3D4M\t*\t0\t0\t%s\t*\tNM:i:3\tAS:i:2" % reads["r"],
                     "u\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*"]) + "\n"
    want = sam.replace("22M3D4M", "7M3D19M")
    assert LA.replace_cigars(sam, pac, {"c": 0}, reads) == (want, 4)
    assert LA.check_sam(sam, want, pac, {"c": 0}, reads) == []
    assert LA.check_sam(sam, sam, pac, {"c": 0}, reads)
    assert LA.check_sam(sam, want.replace("XA:Z:c,+1,7M3D19M", "XA:Z:c,+1,22M3D4M"), pac, {"c": 0}, reads)
    assert LA.check_sam(sam, want.replace("SA:Z:c,1,+,7M3D19M", "SA:Z:c,1,+,8M3D18M"), pac, {"c": 0}, reads)


# ---------------------------------------------------------------- 2. the device routine under the lane emulation
_lib = None


def emu_lalign():
    """tests/emu/emu_lalign.cpp (which includes emu_eqx.cpp and with it emu_api.cpp) compiled the way reflib.emu() compiles emu_api.cpp."""
    global _lib
    if _lib is None:
        os.makedirs(reflib.EMU_DIR, exist_ok=True)
        out = os.path.join(reflib.EMU_DIR, "libhp_emu_lalign.so")
        root = reflib.ROOT
        srcs = [os.path.join(root, "tests", "emu", "emu_lalign.cpp")]
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


def _device(words, read, ref):
    """The record's CIGAR after lalign_cigar; a guard word on either side of the CIGAR must survive."""
    E = emu_lalign()
    buf = np.full(len(words) + 2, SENTINEL, np.int32)
    buf[1:-1] = words
    r = np.ascontiguousarray(read, np.uint8); t = np.ascontiguousarray(ref, np.uint8)
    E.emu_lalign_record.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    moved = E.emu_lalign_record(buf[1:].ctypes.data, len(words), r.ctypes.data, len(r), t.ctypes.data, len(t))
    assert buf[0] == SENTINEL and buf[-1] == SENTINEL, "words written outside the CIGAR"
    return buf[1:-1].tolist(), moved


def test_device_routine_on_hand_made_records():
    for name, cigar, seq, ref, k0, want in HAND:
        words = X.words_of(cigar)
        rl = sum(w >> 4 for w in words if w & 0xf in (0, 2))
        st = LA.new_stats()
        assert LA.left_align(words, _codes(seq), _pac(ref), k0, st) == X.words_of(want)
        got, moved = _device(words, _codes(seq), _codes(ref)[k0:k0 + rl])
        assert X.text_of(got) == want, name
        assert moved == st["moved"], name


def _random_record(rng, n_el):
    """n_el elements over M / I / D with short lengths (many gaps one or two bases apart), clips at the ends now and then, neighbouring
    gaps and neighbouring Ms now and then, against a read and a reference over two letters (long repeats everywhere); rarely a read N,
    rarely an empty M (the routine's walk by the definition)."""
    ops = []
    for i in range(n_el):
        u = rng.random()
        if ops and ops[-1] != 0 and u < 0.85:
            ops.append(0)
        elif ops and ops[-1] == 0 and u < 0.9:
            ops.append(int(rng.integers(1, 3)))
        else:
            ops.append(int(rng.integers(0, 3)))
    if n_el >= 2 and rng.random() < 0.5:
        ops[0] = 4
    if n_el >= 3 and rng.random() < 0.5:
        ops[-1] = 4
    empty_m = rng.random() < 0.1
    lens = []
    for o in ops:
        if o == 0:
            lens.append(0 if empty_m and rng.random() < 0.1 else int(rng.integers(1, 8)) if rng.random() < 0.9 else int(rng.integers(8, 300)))
        else:
            lens.append(int(rng.integers(1, 4)))
    words = [n << 4 | o for o, n in zip(ops, lens)]
    ql = sum(n for o, n in zip(ops, lens) if o in (0, 1, 4)); tl = sum(n for o, n in zip(ops, lens) if o in (0, 2))
    read = rng.integers(0, 2, ql).astype(np.uint8) * 2                  # A / G
    ref = rng.integers(0, 2, tl).astype(np.uint8) * 2
    if rng.random() < 0.5:                                             # stretches of one letter: everything slides
        read[:] = 0; ref[:] = 0
    if ql and rng.random() < 0.2:
        read[rng.integers(0, ql, max(1, ql // 10))] = 4
    return words, read, ref


@pytest.mark.parametrize("n_el", [1, 2, 3, 5, 62, 63, 64, 65, 66, 127, 128, 129, 130, 192, 193, 400])
def test_device_routine_fuzz(n_el):
    rng = np.random.default_rng(4000 + n_el)
    total = LA.new_stats()
    for _ in range(40):
        words, read, ref = _random_record(rng, n_el)
        st = LA.new_stats()
        want = LA.left_align(words, read, _pac_of_codes(ref), 0, st)
        got, moved = _device(words, read, ref)
        assert got == want, (n_el, words)
        assert LA.check_consequences(words, got) == [] or any(w & 0xf == 0 and w >> 4 == 0 for w in words)
        assert LA.left_align(got, read, _pac_of_codes(ref), 0) == got
        if not any(w & 0xf == 0 and w >> 4 == 0 for w in words):
            assert moved == st["moved"]
        for k in total:
            total[k] += st[k]
    for _ in range(10):                                                # 1 .. 400 elements, whatever the parameter
        words, read, ref = _random_record(rng, int(rng.integers(1, 401)))
        assert _device(words, read, ref)[0] == LA.left_align(words, read, _pac_of_codes(ref), 0)
    if n_el >= 5:
        assert total["moved"] > 0 and total["room"] > 0
    if n_el >= 62:
        assert total["cascade"] > 0
    if n_el >= 127:
        assert total["cascade_block"] > 0


# ---------------------------------------------------------------- 3. the whole path under the emulation, the flag set
def _hp_para(lp):
    from lamsa_amd.hp import HpPara
    P = HpPara()
    for n, _ in HpPara._fields_:
        setattr(P, n, getattr(lp, n))
    return P


def _emu_streams_tags(batch, hp_para, tags, scale=1, phased=True, slab_bytes=256 << 20):
    from lamsa_amd.hp import HpRef, HpBatch
    E = emu_lalign()
    E.emu_lds_guard_reset()
    n = batch.n_reads
    hb = reflib.hp_batch_struct(batch, HpBatch)
    hr = HpRef(batch.pac.ctypes.data, int(batch.l_pac), len(batch.seq_len), batch.seq_off.ctypes.data, batch.seq_len.ctypes.data)
    cap = 4096 + 64 * n + 24 * int(batch.read_off[-1]) * scale
    stream = np.zeros(cap, np.int32); nw = C.c_int64(0)
    off = np.zeros(max(n, 1), np.int64); ln = np.zeros(max(n, 1), np.int32); st = np.zeros(max(n, 1), np.int32)
    E.emu_align_batch_tags.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    E.emu_align_batch_tags(C.byref(hp_para), C.byref(hr), C.byref(hb), scale, 1 if phased else 0, tags, slab_bytes, stream.ctypes.data, cap, C.byref(nw), off.ctypes.data, ln.ctypes.data, st.ctypes.data)
    E.emu_lds_guard_hits.restype = C.c_longlong
    assert E.emu_lds_guard_hits() == 0
    return reflib.split_streams(stream, off[:n], ln[:n]), st[:n].copy()


@pytest.mark.parametrize("name", ["c2_pacbio", "c3_ont", "c5_sv"])
def test_whole_path_under_the_emulation(name, tmp_path):
    ref, reads, args, _ = G.stage_scenario(name, str(tmp_path))
    rt, over = G.para_from_args(args)
    lp = reflib.lo_para(rt, **over)
    B = reflib.Batch(ref, reads, lp)
    P = _hp_para(lp)
    want0 = reflib.oracle_streams(B, lp)
    rd = [B.read_seq[B.read_off[r]:B.read_off[r + 1]] for r in range(B.n_reads)]
    st_ = LA.new_stats()
    want = [LA.stream_left_aligned(want0[r], rd[r], B.pac, B.seq_off, st_) for r in range(B.n_reads)]
    assert st_["moved"] > 0 and want != want0
    want_ev = [T.stream_events(want[r], rd[r], B.pac, B.seq_off) for r in range(B.n_reads)]
    want_eq = [X.stream_to_eqx(want[r], rd[r], B.pac, B.seq_off) for r in range(B.n_reads)]
    for phased in (True, False):
        plain, st0 = _emu_streams_tags(B, P, 0, 1, phased)
        assert plain == want0 and (st0 == 0).all(), phased
        la, st = _emu_streams_tags(B, P, TAG_LEFT_ALIGN, 1, phased)
        assert (st == st0).all()
        assert [r for r in range(B.n_reads) if la[r] != want[r]] == [], phased
        mm, st = _emu_streams_tags(B, P, TAG_LEFT_ALIGN | TAG_MISMATCHES, 1, phased)
        assert (st == st0).all()
        both, st = _emu_streams_tags(B, P, TAG_LEFT_ALIGN | TAG_EQX | TAG_MISMATCHES, 1, phased)
        assert (st == st0).all()
        for r in range(B.n_reads):
            s, ev = T.split_events(mm[r])
            assert s == want[r] and ev == want_ev[r], (phased, r)
            s, ev = T.split_events(both[r])
            assert s == want_eq[r] and ev == want_ev[r], (phased, r)


# ---------------------------------------------------------------- 4. the emulated host program (host fallback: rec_left_align)
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
    return p.stdout, gold, X.load_reads(reads)


TAGS = ["--MD", "--cs", "--eqx", "--SA"]


def check_pair(plain, out, rf, reads, tags):
    """out = the run with --left-align, plain = the same run without it."""
    assert LA.check_sam(plain, out, rf[0], rf[1], reads) == []
    if tags:
        assert T.check_sam(X.collapse(out), *rf) == []
        assert X.check_sam(out, rf[0], rf[1], reads) == []


@pytest.mark.parametrize("name", G.SCENARIOS)
def test_cli_with_R0(cli, ref, name, tmp_path):
    plain, gold, reads = _run(cli, tmp_path, name, ["-R", "0"])
    assert G.strip_pg(plain) == G.strip_pg(gold)
    out, _, _ = _run(cli, tmp_path, name, ["-R", "0", "--left-align"])
    check_pair(plain, out, ref, reads, False)
    out_t, _, _ = _run(cli, tmp_path, name, ["-R", "0", "--left-align"] + TAGS)
    check_pair(plain, T.strip_tags(out_t), ref, reads, False)                      # (SA:Z is checked against the records' own fields by tagcheck)
    assert T.check_sam(X.collapse(out_t), *ref) == [] and X.check_sam(out_t, ref[0], ref[1], reads) == []
    assert G.strip_pg(X.collapse(T.strip_tags(out_t))) == G.strip_pg(out)         # the tags add nothing else


@pytest.mark.parametrize("name", G.SCENARIOS)
def test_cli_default_run(cli, ref, name, tmp_path):
    """Stage 4 on: the rescue scenarios have records made on the host, which are shifted there."""
    plain, gold, reads = _run(cli, tmp_path, name, [])
    assert G.strip_pg(plain) == G.strip_pg(G.golden_full(name) if name in G.RESCUE_SCENARIOS else gold)
    out, _, _ = _run(cli, tmp_path, name, ["--left-align"])
    check_pair(plain, out, ref, reads, False)
    out_t, _, _ = _run(cli, tmp_path, name, ["--left-align"] + TAGS)
    check_pair(plain, T.strip_tags(out_t), ref, reads, False)
    assert T.check_sam(X.collapse(out_t), *ref) == [] and X.check_sam(out_t, ref[0], ref[1], reads) == []


def test_cli_moves_gaps_on_the_goldens(cli, ref, tmp_path):
    """The option does something: on the noisy scenarios gaps move, some stop only for want of room."""
    for name in ("c2_pacbio", "c3_ont", "c7_rescue"):
        plain, _, reads = _run(cli, tmp_path, name, [])
        out, _, _ = _run(cli, tmp_path, name, ["--left-align"])
        st = LA.new_stats()
        assert LA.check_sam(plain, out, ref[0], ref[1], reads, st) == []
        assert out != plain and st["moved"] > 0 and st["gaps"] > st["moved"], (name, st)
        again = LA.new_stats()
        assert LA.check_sam(out, out, ref[0], ref[1], reads, again) == [] and again["moved"] == 0      # idempotent


def test_cli_batches_and_shards(cli, ref, tmp_path):
    opts = ["--left-align"] + TAGS
    r, reads, a, gold = G.stage_scenario("c7_rescue", str(tmp_path))
    base = subprocess.run([cli, "aln", "-N"] + opts + a + [r, reads], capture_output=True, text=True)
    assert base.returncode == 0
    p = subprocess.run([cli, "aln", "-N", "--batch", "4"] + opts + a + [r, reads], capture_output=True, text=True)
    assert p.returncode == 0 and G.strip_pg(p.stdout) == G.strip_pg(base.stdout)
    parts = [subprocess.run([cli, "aln", "-N", "--shard", "%d/2" % i] + opts + a + [r, reads], capture_output=True, text=True) for i in range(2)]
    assert all(q.returncode == 0 for q in parts)
    assert G.strip_pg(parts[0].stdout + parts[1].stdout) == G.strip_pg(base.stdout)
    hits = str(tmp_path / "h.bin")
    p = subprocess.run([cli, "aln", "-N", "--devices", "0,0", "--batch", "3", "--save-hits", hits] + opts + a + [r, reads], capture_output=True, text=True)
    assert p.returncode == 0 and G.strip_pg(p.stdout) == G.strip_pg(base.stdout)
    p = subprocess.run([cli, "aln", "--hits", hits] + opts + a + [r, reads], capture_output=True, text=True)
    assert p.returncode == 0 and G.strip_pg(p.stdout) == G.strip_pg(base.stdout)
    plain = subprocess.run([cli, "aln", "-N", "-S"] + TAGS + a + [r, reads], capture_output=True, text=True)         # -S: every record soft-clipped
    p = subprocess.run([cli, "aln", "-N", "-S"] + opts + a + [r, reads], capture_output=True, text=True)
    assert p.returncode == 0 and plain.returncode == 0
    check_pair(plain.stdout, p.stdout, ref, X.load_reads(reads), True)
