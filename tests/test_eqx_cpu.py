"""LAMSA_HP_TAG_EQX / --eqx / --cs without a GPU: the checker itself (tests/eqxcheck.py) on hand-made records, the device routine
(lamsa_amd/csrc/hp_eqx.h) under the CPU lane emulation on explicit inputs and through the whole per-read path, and the emulated
host program, whose C-ABI has no lamsa_hp_set_result_tags: there the host converts the CIGARs itself.  tests/test_eqx_gpu.py checks
the words the HIP kernels make."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import eqxcheck as X
import goldenlib as G
import reflib
import tagcheck as T

ST_OVERFLOW = 1
TAG_MISMATCHES, TAG_EQX = 1, 2


def _pac(ref_seq):
    pac = bytearray((len(ref_seq) + 3) // 4 + 1)
    for k, c in enumerate(ref_seq):
        pac[k >> 2] |= "ACGT".index(c) << ((~k & 3) << 1)
    return np.frombuffer(bytes(pac), np.uint8)


def _codes(seq):
    return T.NT4[np.frombuffer(seq.encode(), np.uint8)]


# ---------------------------------------------------------------- 1. the checker on hand-made records
def test_checker_on_hand_made_records():
    ref = "ACGTACGTAC" + "GGCCAATT" + "ACGTACGTAC"
    pac = _pac(ref)

    def eqx(cigar, seq, k0=0):
        return X.text_of(X.to_eqx(X.words_of(cigar), _codes(seq), pac, k0))

    def cs(cigar, seq, k0=0):
        return X.cs_of(X.words_of(cigar), _codes(seq), pac, k0)

    assert eqx("10M", "ACGTACGTAC") == "10="
    assert eqx("10M", "TCGTACGTAG") == "1X8=1X"                                  # mismatches at both ends of an M
    assert cs("10M", "TCGTACGTAG") == "*at:8*cg"
    assert eqx("4M", "TGCA") == "4X"                                             # a whole M mismatching
    assert cs("4M", "TGCA") == "*at*cg*gc*ta"
    assert eqx("3M2I3M", "ACTGGAAC") == "2=1X2I1X2="                             # X | I | X stays three elements
    assert cs("3M2I3M", "ACTGGAAC") == ":2*gt+gg*ta:2"
    assert eqx("4M", "ANGT") == "1=1X2="                                         # a read N differs
    assert cs("4M", "ANGT") == ":1*cn:2"
    assert eqx("4M2D4M", "ACGTGTAC") == "4=2D4="
    assert cs("4M2D4M", "ACGTGTAC") == ":4-ac:4"
    assert cs("4M2D4M", "ACGTCTAC") == ":4-ac*gc:3"
    assert eqx("2S4M", "GGACGG") == "2S3=1X" and cs("2S4M", "GGACGG") == ":3*tg"     # clips contribute nothing
    assert eqx("3H4M5H", "TTTACGATTTTT") == "3H3=1X5H" and cs("3H4M5H", "TTTACGATTTTT") == ":3*ta"       # hard clips: the whole read is given
    assert cs(eqx("3M2I3M", "ACTGGAAC"), "ACTGGAAC") == cs("3M2I3M", "ACTGGAAC")  # cs is the same from either form
    # SAM text: a '+' record with an XA entry, and a '-' strand, hard-clipped record of the same read (its reverse complement is
    # AAAAAATCGT: the last six bases against GGCCAA at POS 11); collapse() and the text checker
    sam = "\n".join(["@SQ\tSN:c\tLN:28",
                     "r\t0\tc\t1\t9\t3=1X6S\t*\t0\t0\tACGATTTTTT\t*\tNM:i:1\tAS:i:2\tXA:Z:c,+5,3=1X6S,1;\tMD:Z:3T0\tcs:Z::3*ta\tSA:Z:c,11,-,4S3X1=2X,9,5;",
                     "r\t2064\tc\t11\t9\t4H3X1=2X\t*\t0\t0\tAATCGT\t*\tNM:i:5\tAS:i:1\tMD:Z:0G0G0C1A0A0\tcs:Z:*ga*ga*ct:1*ag*at\tSA:Z:c,1,+,3=1X6S,9,1;",
                     "u\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*"]) + "\n"
    flat = X.collapse(sam)
    assert "cs:Z" not in flat and "=" not in flat and "X" not in flat.replace("XA:Z", "")
    assert "\t4M6S\t" in flat and "XA:Z:c,+5,4M6S,1;" in flat and "SA:Z:c,11,-,4S6M,9,5;" in flat and "\t4H6M\t" in flat and "SA:Z:c,1,+,4M6S,9,1;" in flat
    assert T.check_sam(flat, pac, {"c": 0}) == []
    reads = {"r": "ACGATTTTTT", "u": "ACGT"}
    assert X.check_sam(sam, pac, {"c": 0}, reads) == []
    assert X.check_sam(sam.replace("cs:Z::3*ta", "cs:Z::3*tc"), pac, {"c": 0}, reads)
    assert X.check_sam(sam.replace("\t3=1X6S\t", "\t4=6S\t"), pac, {"c": 0}, reads)
    assert X.check_sam(sam.replace("\t4H3X1=2X\t", "\t4H2X1X1=2X\t"), pac, {"c": 0}, reads)          # neighbours must alternate
    assert X.check_sam(sam.replace("XA:Z:c,+5,3=1X6S", "XA:Z:c,+5,4M6S"), pac, {"c": 0}, reads)
    assert X.check_sam(sam.replace("SA:Z:c,11,-,4S3X1=2X", "SA:Z:c,11,-,4S6M"), pac, {"c": 0}, reads)
    assert X.check_sam(sam.replace("\tMD:Z:3T0\tcs:Z::3*ta", "\tcs:Z::3*ta\tMD:Z:3T0"), pac, {"c": 0}, reads)       # tag order
    assert X.check_sam(flat, pac, {"c": 0}, reads, eqx=False, cs=False) == []


def test_stream_to_eqx():
    pac = _pac("ACGTACGTACGGCCAATT")
    read = [0, 1, 3, 3, 4, 1, 2, 3]                                    # ACTTNCGT against ACGTACGT at POS 1
    plain = [0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1, 5, 2, 1, 8 << 4]
    assert X.stream_to_eqx(plain, read, pac, [0]) == plain[:13] + [5, 2 << 4 | 7, 1 << 4 | 8, 1 << 4 | 7, 1 << 4 | 8, 3 << 4 | 7]


# ---------------------------------------------------------------- 2. the device routine under the lane emulation
_lib = None


def emu_eqx():
    """tests/emu/emu_eqx.cpp (which includes emu_api.cpp) compiled the way reflib.emu() compiles emu_api.cpp."""
    global _lib
    if _lib is None:
        os.makedirs(reflib.EMU_DIR, exist_ok=True)
        out = os.path.join(reflib.EMU_DIR, "libhp_emu_eqx.so")
        root = reflib.ROOT
        srcs = [os.path.join(root, "tests", "emu", "emu_eqx.cpp")]
        deps = srcs + [os.path.join(root, "tests", "emu", "emu_api.cpp"), os.path.join(root, "tests", "emu", "hp", "wave.h")] + \
            [os.path.join(root, "lamsa_amd", "csrc", f) for f in os.listdir(os.path.join(root, "lamsa_amd", "csrc")) if f.endswith(".h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.run(["g++"] + reflib.EMU_FLAGS + ["-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                            "-I", os.path.join(root, "tests", "emu"), "-I", os.path.join(root, "lamsa_amd", "csrc"),
                            "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", out] + srcs, check=True, cwd=reflib.EMU_DIR)
        _lib = C.CDLL(out)
    return _lib


SENTINEL = 0x5eed5eed
HDR = 11                                                               # line header (4), record header (6), cigar_n


def _device_eqx(words, mm, cap=None):
    """(status, cigar words or None) of one record through out_line + eqx_words; cap: output capacity in words (default: ample)."""
    E = emu_eqx()
    w = np.ascontiguousarray(words, np.int32); m = np.ascontiguousarray(list(mm) + [0], np.int32)
    big = HDR + len(words) + 2 * len(mm) + 8
    cap = big if cap is None else cap
    out = np.full(big + 8, SENTINEL, np.int32)
    n = C.c_int32(0)
    st = E.emu_eqx_record(w.ctypes.data_as(C.c_void_p), len(words), m.ctypes.data_as(C.c_void_p), len(mm), out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    assert (out[cap:] == SENTINEL).all(), "words written behind the capacity"
    if st != 0:
        return st, None
    assert n.value == HDR + out[HDR - 1]
    return st, out[HDR:n.value].tolist()


def _random_record(rng, ops, lens, n_mm, runs=True):
    """A CIGAR of the given ops / lengths against a random reference, and a read with n_mm mismatches placed in its M elements
    (runs: neighbours likely).  Returns (words, read codes, pac, mismatch list)."""
    words = [int(n) << 4 | int(o) for o, n in zip(ops, lens)]
    rl = sum(n for o, n in zip(ops, lens) if o in (0, 2)); ql = sum(n for o, n in zip(ops, lens) if o in (0, 1, 4))
    ref = rng.integers(0, 4, rl + 4).astype(np.uint8)
    read = rng.integers(0, 4, ql).astype(np.uint8)
    qi = ri = 0
    mpos = []                                                          # (read index, ref index) of every aligned base
    for o, n in zip(ops, lens):
        if o == 0:
            read[qi:qi + n] = ref[ri:ri + n]
            mpos += [(qi + j, ri + j) for j in range(n)]
            qi += n; ri += n
        elif o in (1, 4):
            qi += n
        elif o == 2:
            ri += n
    n_mm = min(n_mm, len(mpos))
    if n_mm:
        if runs:                                                       # seeds grown into runs
            pick = set()
            while len(pick) < n_mm:
                k = int(rng.integers(0, len(mpos)))
                for j in range(int(rng.integers(1, 5))):
                    if len(pick) < n_mm and k + j < len(mpos):
                        pick.add(k + j)
        else:
            pick = set(rng.choice(len(mpos), n_mm, replace=False).tolist())
        for k in pick:
            q, r = mpos[k]
            read[q] = (ref[r] + 1 + int(rng.integers(0, 3))) % 4 if rng.integers(0, 8) else 4       # sometimes a read N
    pac = np.zeros(len(ref) // 4 + 2, np.uint8)
    for k, c in enumerate(ref):
        pac[k >> 2] |= int(c) << ((~k & 3) << 1)
    plain = [0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1, 0, 0, len(words)] + words
    mm = T.stream_events(plain, read, pac, [0])[0]
    return words, read, pac, mm


def _check(words, read, pac, mm, what):
    want = X.to_eqx(words, read, pac, 0)
    st, got = _device_eqx(words, mm)
    assert st == 0 and got == want, what
    # the stated consequences of the definition
    assert sum(w >> 4 for w in got if w & 0xf == 8) == len(mm)
    assert len(got) <= len(words) + 2 * len(mm)
    # a capacity that fits exactly, and one word short: flagged, nothing behind it touched (checked in _device_eqx)
    st, again = _device_eqx(words, mm, cap=HDR + len(want))
    assert st == 0 and again == want, what
    st, _ = _device_eqx(words, mm, cap=HDR + len(want) - 1)
    assert st & ST_OVERFLOW, what


def _mixed_ops(rng, n):
    """n elements: M separated by I / D, a soft clip at either end when there is room."""
    ops = []
    for i in range(n):
        if i % 2 == 0:
            ops.append(0)
        else:
            ops.append(int(rng.integers(1, 3)))
    if n >= 3:
        ops[0] = 4; ops[-1] = 4 if ops[-2] == 0 else ops[-1]
    return ops


@pytest.mark.parametrize("n_el", [1, 63, 64, 65, 128, 129, 400])
def test_device_routine_fuzz(n_el):
    rng = np.random.default_rng(1000 + n_el)
    for n_mm in (0, 1, 63, 64, 65, 128, 129, 1000):
        for runs in (True, False):
            ops = _mixed_ops(rng, n_el)
            lens = [int(rng.integers(1, 40)) if o == 0 else int(rng.integers(1, 4)) for o in ops]
            if n_el == 1:
                ops, lens = [0], [1200]
            _check(*_random_record(rng, ops, lens, n_mm, runs), what=(n_el, n_mm, runs))


def _place(words, read_len_ops, mism_ref_offsets):
    """A record with mismatches at exactly the given reference offsets (all inside M elements)."""
    ops = [w & 0xf for w in words]; lens = [w >> 4 for w in words]
    rng = np.random.default_rng(7)
    words, read, pac, _ = _random_record(rng, ops, lens, 0)
    ref_total = sum(n for o, n in zip(ops, lens) if o in (0, 2))
    ref = T.ref_codes(pac, 0, ref_total)
    qi = ri = 0
    want = set(mism_ref_offsets)
    for o, n in zip(ops, lens):
        if o == 0:
            for j in range(n):
                if ri + j in want:
                    read[qi + j] = (int(ref[ri + j]) + 1) % 4
            qi += n; ri += n
        elif o in (1, 4):
            qi += n
        elif o == 2:
            ri += n
    plain = [0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1, 0, 0, len(words)] + words
    mm = T.stream_events(plain, read, pac, [0])[0]
    assert [e >> 2 for e in mm] == sorted(want)
    return words, read, pac, mm


def test_device_routine_edges():
    M, I, D, S = 0, 1, 2, 4
    w = lambda n, o: n << 4 | o
    # one M of 5 000 bases carrying 250 mismatches (passes of 64, no lane walks them)
    rng = np.random.default_rng(5)
    _check(*_random_record(rng, [0], [5000], 250, False), what="5k M, scattered")
    _check(*_random_record(rng, [0], [5000], 250, True), what="5k M, runs")
    # runs of neighbouring mismatches that straddle a multiple of 64 in the list
    offs = list(range(0, 120, 2)) + list(range(200, 212)) + list(range(300, 500, 3))        # entries 60 .. 71 are one run: it spans entry 64
    _check(*_place([w(600, M)], None, offs), what="run across list entry 64")
    offs = list(range(10, 10 + 200))                                                         # one run of 200: open over three passes
    _check(*_place([w(5, S), w(300, M), w(5, S)], None, offs), what="one run of 200")
    offs = list(range(0, 126, 2)) + [126, 127, 128, 129] + list(range(140, 300, 2))          # entries 63 .. 66 are one run
    _check(*_place([w(400, M)], None, offs), what="run from entry 63")
    # elements that straddle a multiple of 64 in the CIGAR, mismatches on both sides
    words = []
    for i in range(70):
        words += [w(6, M), w(1, I if i % 3 else D)]
    words += [w(6, M)]
    ref_starts, ri = [], 0
    for x in words:
        if x & 0xf == M:
            ref_starts.append(ri)
        if x & 0xf in (M, D):
            ri += x >> 4
    offs = [ref_starts[31] + 5, ref_starts[32], ref_starts[32] + 5, ref_starts[33] + 2]      # elements 62, 64, 66 (the block changes at element 64)
    _check(*_place(words, None, offs), what="elements across 64")
    offs = sorted(set(s for s in ref_starts) | set(s + 5 for s in ref_starts))               # first and last base of every M
    _check(*_place(words, None, offs), what="first / last base of every M")
    # one-base Ms, mismatching or not
    words = []
    for i in range(150):
        words += [w(1, M), w(1, I)]
    words += [w(1, M)]
    _check(*_place(words, None, list(range(0, 151, 2))), what="one-base Ms")
    _check(*_place(words, None, list(range(0, 151))), what="one-base Ms, all mismatching")
    # X | I | X: pieces never merge across elements
    words, read, pac, mm = _place([w(3, M), w(2, I), w(3, M)], None, [2, 3])
    st, got = _device_eqx(words, mm)
    assert st == 0 and got == [w(2, 7), w(1, 8), w(2, I), w(1, 8), w(2, 7)]
    _check(words, read, pac, mm, what="X | I | X")
    # a whole M mismatching, next to a deletion
    _check(*_place([w(4, M), w(3, D), w(4, M)], None, [0, 1, 2, 3, 7, 10]), what="whole M")


# ---------------------------------------------------------------- 3. the whole path under the emulation, flags set
def _hp_para(lp):
    from lamsa_amd.hp import HpPara
    P = HpPara()
    for n, _ in HpPara._fields_:
        setattr(P, n, getattr(lp, n))
    return P


def _emu_streams_tags(batch, hp_para, tags, scale=1, phased=True, slab_bytes=256 << 20):
    from lamsa_amd.hp import HpRef, HpBatch
    E = emu_eqx()
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


@pytest.mark.parametrize("name", ["c3_ont", "c5_sv", "c6_edge", "c9_rearr"])
def test_whole_path_under_the_emulation(name, tmp_path):
    ref, reads, args, _ = G.stage_scenario(name, str(tmp_path))
    rt, over = G.para_from_args(args)
    lp = reflib.lo_para(rt, **over)
    B = reflib.Batch(ref, reads, lp)
    P = _hp_para(lp)
    want = reflib.oracle_streams(B, lp)
    n_x = 0
    for phased, scale in ((True, 1), (False, 1), (False, 8)):
        plain, st0 = _emu_streams_tags(B, P, 0, scale, phased)
        assert plain == want and (st0 == 0).all(), (phased, scale)
        eq, st = _emu_streams_tags(B, P, TAG_EQX, scale, phased)
        assert (st == st0).all()
        both, st = _emu_streams_tags(B, P, TAG_EQX | TAG_MISMATCHES, scale, phased)
        assert (st == st0).all()
        for r in range(B.n_reads):
            read = B.read_seq[B.read_off[r]:B.read_off[r + 1]]
            assert eq[r] == X.stream_to_eqx(plain[r], read, B.pac, B.seq_off), (phased, scale, r)
            s, ev = T.split_events(both[r])
            assert s == eq[r], (phased, scale, r)
            assert ev == T.stream_events(plain[r], read, B.pac, B.seq_off), (phased, scale, r)
            n_x += sum(len(e) for e in ev)
    assert n_x > 0


# ---------------------------------------------------------------- 4. the emulated host program (host fallback: no lamsa_hp_set_result_tags)
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


def check_output(out, want, ref, reads, eqx=True, cs=True):
    """The assertions on a SAM text made with --eqx / --cs (and --MD --SA): back in M form and without the tags it is `want`, the
    reference's output; MD and SA pass tagcheck; every CIGAR and cs is the checker's."""
    flat = X.collapse(out)
    assert G.strip_pg(T.strip_tags(flat)) == G.strip_pg(want)
    assert T.check_sam(flat, *ref) == []
    assert X.check_sam(out, ref[0], ref[1], reads, eqx=eqx, cs=cs) == []


@pytest.mark.parametrize("name", G.SCENARIOS)
def test_cli_with_R0(cli, ref, name, tmp_path):
    out, gold, reads = _run(cli, tmp_path, name, ["-R", "0", "--eqx", "--cs", "--MD", "--SA"])
    check_output(out, gold, ref, reads)
    assert "\tcs:Z:" in out and "\tMD:Z:" in out


@pytest.mark.parametrize("name", G.SCENARIOS)
def test_cli_default_run(cli, ref, name, tmp_path):
    """Stage 4 on: the rescue scenarios have records made on the host, which go through the same conversion."""
    out, gold, reads = _run(cli, tmp_path, name, ["--eqx", "--cs", "--MD", "--SA"])
    check_output(out, G.golden_full(name) if name in G.RESCUE_SCENARIOS else gold, ref, reads)


def test_cli_batches_devices_shards_and_hit_stream(cli, ref, tmp_path):
    tags = ["--eqx", "--cs", "--MD", "--SA"]
    r, reads, a, gold = G.stage_scenario("c7_rescue", str(tmp_path))
    base = subprocess.run([cli, "aln", "-N"] + tags + a + [r, reads], capture_output=True, text=True)
    assert base.returncode == 0
    check_output(base.stdout, G.golden_full("c7_rescue"), ref, X.load_reads(reads))
    p = subprocess.run([cli, "aln", "-N", "--batch", "5"] + tags + a + [r, reads], capture_output=True, text=True)
    assert p.returncode == 0 and G.strip_pg(p.stdout) == G.strip_pg(base.stdout)
    hits = str(tmp_path / "h.bin")
    p = subprocess.run([cli, "aln", "-N", "--devices", "0,0,0", "--batch", "2", "--save-hits", hits] + tags + a + [r, reads], capture_output=True, text=True)
    assert p.returncode == 0 and G.strip_pg(p.stdout) == G.strip_pg(base.stdout)
    p = subprocess.run([cli, "aln", "--hits", hits] + tags + a + [r, reads], capture_output=True, text=True)
    assert p.returncode == 0 and G.strip_pg(p.stdout) == G.strip_pg(base.stdout)
    parts = [subprocess.run([cli, "aln", "-N", "--shard", "%d/2" % i] + tags + a + [r, reads], capture_output=True, text=True) for i in range(2)]
    assert all(q.returncode == 0 for q in parts)
    assert G.strip_pg(parts[0].stdout + parts[1].stdout) == G.strip_pg(base.stdout)
    p = subprocess.run([cli, "aln", "-N", "-S"] + tags + a + [r, reads], capture_output=True, text=True)      # -S: every record soft-clipped
    assert p.returncode == 0 and X.check_sam(p.stdout, ref[0], ref[1], X.load_reads(reads)) == [] and T.check_sam(X.collapse(p.stdout), *ref) == []


@pytest.mark.parametrize("name", ["c7_rescue", "c9_rearr"])
def test_cli_each_option_alone(cli, ref, name, tmp_path):
    """--eqx alone changes the CIGARs and nothing else; --cs alone adds the tag and nothing else."""
    plain, gold, reads = _run(cli, tmp_path, name, [])
    out, _, _ = _run(cli, tmp_path, name, ["--eqx"])
    assert "cs:Z" not in out and "MD:Z" not in out and out != plain
    assert G.strip_pg(X.collapse(out)) == G.strip_pg(plain)
    assert X.check_sam(out, ref[0], ref[1], reads, eqx=True, cs=False) == []
    out, _, _ = _run(cli, tmp_path, name, ["--cs"])
    assert G.strip_pg(X.collapse(out)) == G.strip_pg(plain) and "\tcs:Z:" in out
    assert X.check_sam(out, ref[0], ref[1], reads, eqx=False, cs=True) == []
