"""The record-stream helpers of lamsa_amd/csrc/hp_out.h without a GPU (tests/emu/emu_out.cpp): the capacity table against the values the
functions had before they moved into one file (tests/golden/out_caps.json, recorded from that commit), the lane copy at the block edges
next to guard words, and a covered interval through out_reg and back."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import reflib

_lib = None


def emu_out():
    """tests/emu/emu_out.cpp (which includes emu_api.cpp) compiled the way reflib.emu() compiles emu_api.cpp."""
    global _lib
    if _lib is None:
        os.makedirs(reflib.EMU_DIR, exist_ok=True)
        out = os.path.join(reflib.EMU_DIR, "libhp_emu_out.so")
        root = reflib.ROOT
        srcs = [os.path.join(root, "tests", "emu", "emu_out.cpp")]
        deps = srcs + [os.path.join(root, "tests", "emu", f) for f in ("emu_api.cpp", os.path.join("hp", "wave.h"))] + \
            [os.path.join(root, "include", "lamsa_hp.h")] + \
            [os.path.join(root, "lamsa_amd", "csrc", f) for f in os.listdir(os.path.join(root, "lamsa_amd", "csrc")) if f.endswith(".h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.run(["g++"] + reflib.EMU_FLAGS + ["-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                            "-I", os.path.join(root, "tests", "emu"), "-I", os.path.join(root, "lamsa_amd", "csrc"),
                            "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", out] + srcs, check=True, cwd=reflib.EMU_DIR)
        _lib = C.CDLL(out)
    return _lib


# ---------------------------------------------------------------- 1. the capacity table
LENGTHS, SCALES = (1, 2, 49, 50, 51, 4000, 10000, 100000), (1, 8)
TAG_SETS = [t for t in range(64) if not t & ~(1 | 2 | 8 | 32) and not (t & 32 and t & 3)]       # what result_tags_valid accepts


def test_capacity_table_is_the_recorded_one():
    E = emu_out()
    fx = json.load(open(os.path.join(reflib.ROOT, "tests", "golden", "out_caps.json")))
    want = {tuple(r[:3]): r[3:] for r in fx["rows"]}
    assert sorted(want) == sorted((L, s, t) for L in LENGTHS for s in SCALES for t in TAG_SETS)
    for (L, scale, tags), vals in want.items():
        v = (C.c_int64 * 32)()
        k = E.emu_out_caps(L, scale, tags, fx["n_reads"], fx["band_w"], 2 * L + 3, v)
        assert k == len(fx["names"])
        got = [int(v[i]) for i in range(k)]
        assert got == vals, "L %d scale %d tags %d: %s" % (L, scale, tags, [(n, a, b) for n, a, b in zip(fx["names"], got, vals) if a != b])


# ---------------------------------------------------------------- 2. the lane copy
GUARD = 0x5eed5eed


@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129])
def test_out_copy_at_block_edges(n, width):
    E = emu_out()
    rng = np.random.default_rng(100 * width + n)
    if width == 4:
        src = rng.integers(-2**31, 2**31, n + 8, dtype=np.int64).astype(np.int32)
    else:
        src = rng.integers(-2**15, 2**15, n + 8, dtype=np.int64).astype(np.int16)             # negative elements too: the copy sign-extends
    buf = np.full(64 + n + 64, GUARD, dtype=np.int64).astype(np.int32)
    E.emu_out_copy(width, src.ctypes.data_as(C.c_void_p), n, buf[64:].ctypes.data_as(C.POINTER(C.c_int32)))
    assert (buf[:64] == np.int32(GUARD)).all() and (buf[64 + n:] == np.int32(GUARD)).all()
    assert buf[64:64 + n].tolist() == [int(x) for x in src[:n]]


# ---------------------------------------------------------------- 3. a covered interval
def test_out_reg_layout_and_read_back():
    E = emu_out()
    # beg, end; '-' end at chr 3, position 5 000 000 123 (above 2^32); '+' end at chr 7, position 2^31 + 5 (low word negative as int32)
    pos_b, pos_e = 5_000_000_123, 2**31 + 5
    def i32(x):
        return int(np.uint32(x & 0xffffffff).astype(np.int32))
    fields = [17, 4242, 1, 3, i32(pos_b), pos_b >> 32, 0, 7, i32(pos_e), pos_e >> 32]
    inp = (C.c_int32 * 10)(*fields)
    words = np.full(12, GUARD, dtype=np.int64).astype(np.int32)
    back, n_out = (C.c_int32 * 10)(), C.c_int32()
    st = E.emu_out_reg(inp, words.ctypes.data_as(C.POINTER(C.c_int32)), 10, C.byref(n_out), back)
    assert st == 0 and n_out.value == 10
    assert words[:10].tolist() == fields and (words[10:] == np.int32(GUARD)).all()         # beg, end, then is_rev, chr, pos_lo, pos_hi of each end
    assert list(back) == fields
    # one word short: ST_OVERFLOW, nine words written and nothing behind them
    words[:] = np.int32(GUARD)
    st = E.emu_out_reg(inp, words.ctypes.data_as(C.POINTER(C.c_int32)), 9, C.byref(n_out), back)
    assert st == 1 and n_out.value == 9 and (words[9:] == np.int32(GUARD)).all()


# ---------------------------------------------------------------- 4. the host's pass over a record, as a program under the sanitizers
FIN_LEFT_ALIGN, FIN_AUX, FIN_EQX, FIN_SUMMARY = 1, 2, 4, 8


def test_host_finish_under_sanitizers(tmp_path):
    """tests/host/finish_check.cpp built with AddressSanitizer and UBSan and run directly: parse_stream and read_finish (every step of
    rec_finish) on the emulation's flag-off streams of c5_sv and c7_rescue.  What it leaves in the records is what the four checkers make
    of the same streams, applied in rec_finish's order: gaps left-aligned, then lists, =/X form and summary of the shifted CIGAR."""
    import eqxcheck as X
    import goldenlib as G
    import lalcheck as LA
    import pafcheck as PF
    import streamwalk as W
    import tagcheck as T
    from lamsa_amd.hp import HpPara
    exe = str(tmp_path / "finish_check")
    host = os.path.join(G.ROOT, "lamsa_amd", "host")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-I", host, "-I", os.path.join(G.ROOT, "include"),
                    "-o", exe, os.path.join(G.ROOT, "tests", "host", "finish_check.cpp"), os.path.join(host, "rescue.cpp"), os.path.join(host, "lamsa_host.cpp"),
                    os.path.join(G.ROOT, "tests", "emu", "emu_api.cpp"), os.path.join(G.ROOT, "tests", "emu", "emu_capi.cpp"),
                    "-I", os.path.join(G.ROOT, "tests", "emu"), "-I", os.path.join(G.ROOT, "lamsa_amd", "csrc"), "-lz", "-lpthread"], check=True)
    for name in ("c5_sv", "c7_rescue"):
        d = tmp_path / name
        d.mkdir()
        ref, reads, args, _ = G.stage_scenario(name, str(d))
        rt, over = G.para_from_args(args)
        lp = reflib.lo_para(rt, **over)
        B = reflib.Batch(ref, reads, lp)
        P = HpPara()
        for n, _ in HpPara._fields_:
            setattr(P, n, getattr(lp, n))
        streams, st = reflib.emu_streams(B, P)
        assert (np.asarray(st) == 0).all()
        rd = [B.read_seq[B.read_off[r]:B.read_off[r + 1]] for r in range(B.n_reads)]
        words = [B.n_reads]
        for r in range(B.n_reads):
            words += [len(rd[r]), len(streams[r])] + rd[r].tolist() + streams[r]
        np.asarray(words, np.int32).tofile(str(d / "in.bin"))
        p = subprocess.run([exe, ref, str(d / "in.bin"), str(d / "out.bin"), str(FIN_LEFT_ALIGN | FIN_AUX | FIN_EQX | FIN_SUMMARY)], capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout.startswith("ok") and p.stderr == "", p.stdout + p.stderr[-3000:]
        got = np.fromfile(str(d / "out.bin"), np.int32).tolist()
        want, n_rec = [], 0
        for r in range(B.n_reads):
            la = LA.stream_left_aligned(streams[r], rd[r], B.pac, B.seq_off)
            ev = T.stream_events(la, rd[r], B.pac, B.seq_off)
            eq = W.records(X.stream_to_eqx(la, rd[r], B.pac, B.seq_off))
            sm = W.records(PF.stream_summaries(la, len(rd[r])), summary=True)
            assert len(ev) == len(eq) == len(sm)
            want.append(0)
            for e, q, s in zip(ev, eq, sm):
                want += q.hdr + q.cig + [len(e)] + e + s.sum
            n_rec += len(ev)
        assert n_rec > 0 and p.stdout.split()[1] == str(n_rec)
        assert got == want, name
