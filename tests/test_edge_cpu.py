"""The edge classifier in diagonal form without a GPU.  1: hit_diag / edge_dis / edge_class_diag / edge_match_diag (lamsa_amd/csrc/hp_chain.h) and
gap_edge (hp_cluster.h) under the CPU lane emulation against edge_flag_packed, the general 64-bit definition, on a grid that stands on every
boundary of the predicate.  2: the hand-made reads of tests/edge_cases.py through the whole emulated per-read path under each of the three LDS sizes
of the chaining kernels, phased and one-kernel, word for word against the oracle, with the path counters that say the intended routine ran.
3: the pair count of the target loop (r.n_pairs, the bench's pair_evals): its closed form per target against the sum over the blocks the loop
really scans, which is how the count was kept before; and that the block minimum does keep blocks out of a scan.  tests/test_edge_gpu.py puts the same reads through the HIP kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import edge_cases as EC
import reflib

F_MATCH, F_MISMATCH, F_LONG_MISMATCH, F_INSERT, F_DELETE, F_UNCONNECT = 0, 2, 3, 4, 5, 8

_lib = None


def emu_edge():
    """tests/emu/emu_edge.cpp (which includes emu_api.cpp) compiled the way reflib.emu() compiles emu_api.cpp."""
    global _lib
    if _lib is None:
        os.makedirs(reflib.EMU_DIR, exist_ok=True)
        out = os.path.join(reflib.EMU_DIR, "libhp_emu_edge.so")
        root = reflib.ROOT
        srcs = [os.path.join(root, "tests", "emu", "emu_edge.cpp")]
        deps = srcs + [os.path.join(root, "tests", "emu", f) for f in ("emu_api.cpp", os.path.join("hp", "wave.h"))] + \
            [os.path.join(root, "include", "lamsa_hp.h")] + \
            [os.path.join(root, "lamsa_amd", "csrc", f) for f in os.listdir(os.path.join(root, "lamsa_amd", "csrc")) if f.endswith(".h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.run(["g++"] + reflib.EMU_FLAGS + ["-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                            "-I", os.path.join(root, "tests", "emu"), "-I", os.path.join(root, "lamsa_amd", "csrc"),
                            "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", out] + srcs, check=True, cwd=reflib.EMU_DIR)
        _lib = C.CDLL(out)
    return _lib


def _hp_para(lp):
    from lamsa_amd.hp import HpPara
    P = HpPara()
    for n, _ in HpPara._fields_:
        setattr(P, n, getattr(lp, n))
    return P


# ---------------------------------------------------------------- 1. the classifier on a grid
PRESETS = ["default", "pacbio", "ont2d"]
OVERRIDES = [{}, {"SV_len_thd": 10000}, {"SV_len_thd": 50}, {"band_w": 200}]
LEN_DIFS = [-127, -1, 0, 1, 127]
SID0, SID_A = 3, 7                 # the read's first seed id and the seed id of the earlier hit of every pair
POS_A = (1 << 33) + 12345          # its position: beyond 32 bits, so the relative form has something to drop


def _grid(lp):
    """Every grid point of one parameter set as arrays: strand, dsid, the two len_difs and the target dis."""
    step, slen, md = lp.seed_step, lp.seed_len, lp.match_dis
    high_err = lp.aln_mode & 2
    mis3 = 3 * lp.mismatch_thd
    d_min = (slen - 1) // step + 1                      # the smallest seed distance whose span reaches seed_len
    dsids = sorted({1, 2, mis3, mis3 + 1, 40, 399, 16383, max(d_min - 1, 1), d_min, d_min + 1})
    rows = []
    for sp in (1, -1):
        for dsid in dsids:
            mat = md * (dsid if high_err else 1)
            bounds = [mat, -mat, lp.SV_len_thd, -(dsid * step - slen), -(lp.split_len // 2), -lp.SV_len_thd]
            for b in bounds:
                for dis in (b - 1, b, b + 1):
                    for la in LEN_DIFS:
                        for lb in LEN_DIFS:
                            rows.append((sp, dsid, la, lb, dis))
    return np.array(rows, np.int64), dsids, d_min


def _by_definition(lp, dsid, dis):
    """get_fseed_dis' classes (lamsa_dp_con.c:596-634) straight from (dis, dsid): what the grid is expected to cover."""
    step, slen, md = lp.seed_step, lp.seed_len, lp.match_dis
    span = dsid * step
    mat = md * (dsid if lp.aln_mode & 2 else 1)
    if span < slen:
        return F_UNCONNECT
    if -mat <= dis <= mat:
        return F_MATCH if dsid == 1 else (F_MISMATCH if dsid <= 3 * lp.mismatch_thd else F_LONG_MISMATCH)
    if mat < dis < lp.SV_len_thd:
        return F_DELETE
    if (dis < -mat and dis >= -(span - slen)) or (dis < -(lp.split_len // 2) and dis >= -lp.SV_len_thd):
        return F_INSERT
    return F_UNCONNECT


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("over", OVERRIDES, ids=lambda o: "-".join("%s%s" % kv for kv in o.items()) or "preset")
def test_diagonal_classifier_equals_the_definition(preset, over):
    lp = reflib.lo_para(preset, **over)
    P = _hp_para(lp)
    g, dsids, d_min = _grid(lp)
    n = len(g)
    sp, dsid, la, lb, dis = (g[:, k] for k in range(5))
    step = lp.seed_step
    ld = np.where(sp > 0, la, lb)
    # the later hit stands where get_fseed_dis gives exactly `dis`: sp * (pos_b - pos_a) - dsid * step - ld = dis
    apos = np.full(n, POS_A, np.int64)
    bpos = apos + sp * (dis + ld + dsid * step)
    assert (bpos > 0).all()
    base = np.minimum(apos, bpos)                        # the cluster's first hit: relative positions are >= 0
    asid = np.full(n, SID_A, np.int32); bsid = (SID_A + dsid).astype(np.int32)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    i64 = lambda a: np.ascontiguousarray(a, np.int64)
    sp32, la32, lb32 = i32(sp), i32(la), i32(lb)
    apos, bpos, base = i64(apos), i64(bpos), i64(base)
    out = [np.full(n, -1, np.int32) for _ in range(5)]
    E = emu_edge()
    E.emu_edge_grid.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 13
    k24 = E.emu_edge_grid(C.byref(P), n, SID0, sp32.ctypes.data, base.ctypes.data, apos.ctypes.data, asid.ctypes.data, la32.ctypes.data,
                          bpos.ctypes.data, bsid.ctypes.data, lb32.ctypes.data, *[o.ctypes.data for o in out])
    assert k24 == 1
    want, want_rev, diag, match, gap = out
    expect = np.array([_by_definition(lp, int(d), int(x)) for d, x in zip(dsid, dis)], np.int32)
    assert (want == expect).all()                        # the grid stands where it is meant to stand
    assert (want_rev == want).all()
    bad = np.nonzero(diag != want)[0]
    assert len(bad) == 0, ("edge_class_diag", g[bad[:5]].tolist(), diag[bad[:5]].tolist(), want[bad[:5]].tolist())
    bad = np.nonzero(gap != want)[0]
    assert len(bad) == 0, ("gap_edge", g[bad[:5]].tolist(), gap[bad[:5]].tolist(), want[bad[:5]].tolist())
    bad = np.nonzero(match != (want <= F_LONG_MISMATCH))[0]
    assert len(bad) == 0, ("edge_match_diag", g[bad[:5]].tolist())
    # every class is met, on both strands, and the seed distances stand below, at and above seed_len
    for s in (1, -1):
        seen = set(want[sp == s].tolist())
        assert {F_MISMATCH, F_LONG_MISMATCH, F_INSERT, F_DELETE, F_UNCONNECT} <= seen, (s, seen)
        if d_min == 1:
            assert F_MATCH in seen
    assert d_min in dsids and d_min + 1 in dsids
    if d_min > 1:
        assert d_min - 1 in dsids and (want[dsid == d_min - 1] == F_UNCONNECT).all()


# ---------------------------------------------------------------- 2. the hand-made reads, whole path, every LDS size
@pytest.fixture(scope="module")
def oracle_of():
    """The oracle's streams of every case, computed once per case key and LDS size (the capacity cases differ by size)."""
    memo = {}

    def get(W, case):
        k = (W, case.key)
        if k not in memo:
            lp = reflib.lo_para(case.read_type)
            memo[k] = (lp, reflib.oracle_streams(case.batch, lp))
        return memo[k]
    return get


@pytest.mark.parametrize("W", EC.SHAPES)
def test_hand_made_reads_under_the_emulation(W, oracle_of):
    for case in EC.cases(W):
        lp, want = oracle_of(W, case)
        assert all(len(s) > 0 and EC.n_lines(s) >= 1 for s in want), case.key          # the oracle aligns every read
        P = _hp_para(lp)
        for phased in (True, False):
            stats = []
            got, st = reflib.emu_streams(case.batch, P, phased=phased, chain_lds_words=W, stats=stats)
            assert (st == 0).all(), (case.key, phased, st.tolist())
            assert got == want, (case.key, phased, case.aim)
            if phased:                                                                      # the one-kernel path has HP_BOTH_LDS_WORDS, whatever W
                for slot, op, val in case.expect:
                    v = stats[slot]
                    assert {"==": v == val, ">": v > val, ">=": v >= val}[op], (case.key, "counter %d = %d, wanted %s %d" % (slot, v, op, val), case.aim)


# ---------------------------------------------------------------- 3. the pair count of the target loop
def _streams_on_edge_lib(batch, hp_para, W):
    """reflib.emu_streams (phased) on the library of tests/emu/emu_edge.cpp, whose build counts the pairs both ways."""
    from lamsa_amd.hp import HpRef, HpBatch
    E = emu_edge()
    E.emu_set_phased(1); E.emu_set_unit_cap(0); E.emu_set_cl_cap(0); E.emu_set_lane_dp(1); E.emu_set_gap_caps(0, 0); E.emu_set_wave_jobs(1)
    E.emu_set_wj_small(0); E.emu_set_frag_block_min(0); E.emu_stat_reset()
    assert E.emu_set_chain_lds_words(int(W)) == 0
    E.emu_set_lds_shrink(0); E.emu_lds_guard_reset(); E.emu_edge_pairs_reset()
    n = batch.n_reads
    hb = reflib.hp_batch_struct(batch, HpBatch)
    hr = HpRef(batch.pac.ctypes.data, int(batch.l_pac), len(batch.seq_len), batch.seq_off.ctypes.data, batch.seq_len.ctypes.data)
    cap = 4096 + 64 * n + 16 * int(batch.read_off[-1])
    stream = np.zeros(cap, np.int32); nw = C.c_int64(0)
    off = np.zeros(max(n, 1), np.int64); ln = np.zeros(max(n, 1), np.int32); st = np.zeros(max(n, 1), np.int32)
    E.emu_align_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    E.emu_align_batch(C.byref(hp_para), C.byref(hr), C.byref(hb), 1, 256 << 20, stream.ctypes.data, cap, C.byref(nw), off.ctypes.data, ln.ctypes.data, st.ctypes.data)
    E.emu_set_chain_lds_words(reflib.CHAIN_LDS_WORDS[0])
    E.emu_lds_guard_hits.restype = C.c_longlong
    assert E.emu_lds_guard_hits() == 0
    out = (C.c_longlong * 4)()
    E.emu_edge_pairs(out)
    return reflib.split_streams(stream, off[:n], ln[:n]), st[:n].copy(), [int(v) for v in out]


@pytest.mark.parametrize("W", EC.SHAPES)
def test_pair_count_of_the_target_loop(W, oracle_of):
    """Every read: the closed form equals the block-by-block sum.  The reads of more than one block have targets that skip blocks, and a read of n
    hits in one cluster whose targets skipped nothing would count (targets) x n pairs: the count is below that exactly by the blocks skipped."""
    skipped = {}
    for case in EC.cases(W):
        lp, want = oracle_of(W, case)
        got, st, (by_block, formula, blocks_skipped, targets) = _streams_on_edge_lib(case.batch, _hp_para(lp), W)
        assert (st == 0).all() and got == want, case.key
        assert by_block == formula, (case.key, by_block, formula)
        if case.key != "cap+1":
            assert targets > 0 and formula > 0, case.key
        skipped[case.key] = blocks_skipped
    assert skipped["block-64"] == 0 and skipped["block-65"] > 0 and skipped["block-129"] > 0 and skipped["cap"] > 0, skipped
