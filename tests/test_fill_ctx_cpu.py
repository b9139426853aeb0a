"""One read context per wave in the fill launches (hp_phase.h), checked on the CPU.

On the GPU the phases of k_fill / k_filllist / k_chain1 / k_chain2 are handed ONE context block per wave that lives as long as
the wave does, so every unit meets what the previous read and line left in it.  The ordinary emulation library gives each call a
fresh local instead.  This file builds a second emulation library from the unmodified tests/emu/emu_api.cpp with
-DHP_PH_CTX_SHARED: the calling-frame overloads of the phases then use one block that lives across calls (pre-filled with a
non-zero pattern), and the emulation runs all lines of all reads through that one "wave".  A field a phase reads without having
set it (rc_ready, flip, cur_read, leaf_on, nodes_ready, the accounting counters) would show here as a different stream.

The emulation's entry points cannot set LAMSA_HP_TAG_MISMATCHES or read_skip as they stand (emu_align_batch binds neither), so the
mismatch lists and refused reads are checked on the GPU only (tests/test_tags_gpu.py, tests/test_fill_ctx_gpu.py); failing reads
are made here with a small line queue (emu_set_unit_cap) and a small slab.
The sizes (everything in the block fits PH_CTX_BYTES; seven waves per SIMD of rows + block fit the CU's LDS) are static_asserts of
hp_phase.h: building either library checks them."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import goldenlib
import reflib

ROOT = reflib.ROOT


def _shared_lib():
    """tests/_build/libhp_emu_ctx.so: tests/emu/emu_api.cpp as it is, plus -DHP_PH_CTX_SHARED."""
    os.makedirs(reflib.EMU_DIR, exist_ok=True)
    out = os.path.join(reflib.EMU_DIR, "libhp_emu_ctx.so")
    srcs = [os.path.join(ROOT, "tests", "emu", "emu_api.cpp")]
    csrc = os.path.join(ROOT, "lamsa_amd", "csrc")
    deps = srcs + [os.path.join(ROOT, "tests", "emu", "hp", "wave.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++"] + reflib.EMU_FLAGS + ["-DHP_PH_CTX_SHARED", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                        "-I", os.path.join(ROOT, "tests", "emu"), "-I", csrc,
                        "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", out] + srcs, check=True, cwd=reflib.EMU_DIR)
    return C.CDLL(out)


@pytest.fixture(scope="module")
def shared():
    reflib.emu()
    return _shared_lib()


@contextlib.contextmanager
def _using(lib):
    """reflib.emu_streams drives whatever library reflib.emu() returns."""
    reflib.emu()
    keep = reflib._emu
    reflib._emu = lib
    try:
        yield
    finally:
        reflib._emu = keep


def _hp_para(lp):
    from lamsa_amd.hp import HpPara
    P = HpPara()
    for n, _ in HpPara._fields_:
        setattr(P, n, getattr(lp, n))
    return P


def _scenario(name, tmp_path):
    ref, reads, args, _ = goldenlib.stage_scenario(name, str(tmp_path))
    rt, over = goldenlib.para_from_args(args)
    lp = reflib.lo_para(rt, **over)
    return reflib.Batch(ref, reads, lp), lp


@pytest.mark.parametrize("mode", [True, "wave-dp"], ids=["phased", "phased-wave-dp"])
@pytest.mark.parametrize("name", goldenlib.SCENARIOS)
def test_reused_context_block_gives_the_same_streams(shared, name, mode, tmp_path):
    """Every golden scenario, both rounds (chain1 / fill / chain2 / fill / publish): the library whose phases reuse one context block
    gives the ordinary library's and the oracle's result stream, word for word, and the same status words."""
    B, lp = _scenario(name, tmp_path)
    P = _hp_para(lp)
    kw = dict(phased=True, lane_dp=mode is True)
    want = reflib.oracle_streams(B, lp)
    plain, st_plain = reflib.emu_streams(B, P, **kw)
    with _using(shared):
        got, st = reflib.emu_streams(B, P, **kw)
    assert [i for i in range(B.n_reads) if got[i] != plain[i]] == []
    assert [i for i in range(B.n_reads) if got[i] != want[i]] == []
    assert (st == st_plain).all() and (st == 0).all()


def _first_strand(B, r):
    s0 = B.seed_off[r]
    h0, h1 = B.hit_off[s0], B.hit_off[B.seed_off[r + 1]]
    return int(B.h_strand[h0]) if h1 > h0 else 0


def test_failing_reads_leave_nothing_behind(shared, tmp_path):
    """One batch in which reads of both strands alternate, and in which some reads fail: an early return of a phase must not
    leave state in the block for the next unit.  Reads fail (ST_OVERFLOW) in the chaining by a line queue with room for a few
    lines only, and in the chaining or the fill by a slab that holds the short reads but not the long ones, the reads ordered
    short / long in turn."""
    B0, lp = _scenario("c3_ont", tmp_path)
    P = _hp_para(lp)
    plus = [r for r in range(B0.n_reads) if _first_strand(B0, r) == 1]
    minus = [r for r in range(B0.n_reads) if _first_strand(B0, r) == -1]
    assert plus and minus
    order = [r for pair in zip(plus, minus) for r in pair]
    order += [r for r in range(B0.n_reads) if r not in order]
    B = B0.take(order)
    want = reflib.oracle_streams(B, lp)
    for kw in (dict(unit_cap=3), dict(unit_cap=B.n_reads)):
        plain, st_plain = reflib.emu_streams(B, P, **kw)
        with _using(shared):
            got, st = reflib.emu_streams(B, P, **kw)
        assert got == plain and (st == st_plain).all()
        lost = [i for i in range(B.n_reads) if st[i] & 1]
        assert lost and len(lost) < B.n_reads
        assert all(len(got[i]) == 3 for i in lost)
        assert all(got[i] == want[i] for i in range(B.n_reads) if not st[i])
    # short and long reads in turn, a slab between what the two need
    length = np.diff(B0.read_off)
    by_len = [int(r) for r in np.argsort(length, kind="stable")]
    half = len(by_len) // 2
    order = [r for pair in zip(by_len[:half], by_len[::-1][:half]) for r in pair]
    B = B0.take(order)
    want = reflib.oracle_streams(B, lp)
    mixed = 0
    for slab in (700 << 10, 1 << 20, 3 << 19, 2 << 20, 3 << 20):
        plain, st_plain = reflib.emu_streams(B, P, slab_bytes=slab)
        with _using(shared):
            got, st = reflib.emu_streams(B, P, slab_bytes=slab)
        assert got == plain and (st == st_plain).all()
        assert all(got[i] == want[i] for i in range(B.n_reads) if not st[i])
        lost = [i for i in range(B.n_reads) if st[i] & 1]
        assert all(len(got[i]) == 3 for i in lost)
        mixed += 0 < len(lost) < B.n_reads
    assert mixed, "no slab size made some reads fail and others pass"
