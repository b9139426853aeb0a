"""The record writers of lamsa_amd/csrc/hp_out.h on the MI355X: every shape of record that out_line writes, on the phased path and on the
one-kernel path, against the oracle's stream put through the four checkers.  The inputs are first shown -- on the CPU, from the
flag-off oracle stream -- to hold CIGARs and mismatch lists below, inside and above the second block of 64 lanes of out_copy, and a
line of several records."""
import os
import sys

import pytest

import eqxcheck as X
import goldenlib as G
import lalcheck as LA
import pafcheck as P
import streamwalk as W
import tagcheck as T

pytestmark = pytest.mark.gpu

SHAPES = {"ont2d": ("ont2d", "ont2d", {}, 21), "sv10k": ("default", "sv10k", {"SV_len_thd": 10000}, 24)}       # read type, simulator profile, parameters, seed
TAG_SETS = (0, 1, 2, 1 | 2, 8, 32)


def size_classes(sizes):
    """(how many below 64, of 64 .. 128, above 128): one, two, more than two trips of out_copy (the second one full or not)"""
    return (sum(n < 64 for n in sizes), sum(64 <= n <= 128 for n in sizes), sum(n > 128 for n in sizes))


def expected(tags, plain, rd, B, para):
    """The stream of one read under `tags` from its flag-off stream, by the checkers; with a list item: (stream without lists, lists)."""
    if tags == 32:
        return P.stream_summaries(plain, len(rd), para)
    s = LA.stream_left_aligned(plain, rd, B.pac, B.seq_off) if tags & 8 else plain
    ev = T.stream_events(s, rd, B.pac, B.seq_off) if tags & 1 else None
    if tags & 2:
        s = X.stream_to_eqx(s, rd, B.pac, B.seq_off)
    return (s, ev) if tags & 1 else s


@pytest.fixture(scope="module")
def cases():
    """Per shape: the handle, the batch, its reads, the oracle's flag-off streams, the parameters, and what the streams exercise."""
    sys.path.insert(0, os.path.join(G.ROOT, "tools"))
    import reflib
    import simbatch
    from lamsa_amd import hp
    ref = simbatch.SimRef(20_000_000, n_contigs=4, seed=9, threads=16)
    out = {}
    for name, (rt, prof, over, seed) in sorted(SHAPES.items()):
        B = simbatch.SimBatch(ref, 32, 4000, prof, seed=seed, threads=16)
        plain = reflib.oracle_streams(B, reflib.lo_para(rt, **over), 16)
        rd = [B.read_seq[B.read_off[r]:B.read_off[r + 1]] for r in range(B.n_reads)]
        cig = [len(x.cig) for s in plain for x in W.records(s)]
        mm = [len(e) for r in range(B.n_reads) for e in T.stream_events(plain[r], rd[r], B.pac, B.seq_off)]
        multi = sum(x[3] > 1 for s in plain for kind, x in W.walk(s) if kind == "line")
        print(name, "records", len(cig), "CIGAR words <64 / 64..128 / >128:", size_classes(cig), "mismatches:", size_classes(mm), "lines of several records:", multi)
        para = hp.make_para(rt, **over)
        h = hp.LamsaHp(para, ref=(ref.pac, ref.l_pac, ref.seq_off, ref.seq_len), device=0)
        out[name] = (h, B, rd, plain, para, cig, mm, multi)
    yield out
    for c in out.values():
        c[0].close()


def test_inputs_reach_every_block_edge(cases):
    """Over the two batches together (no single profile of the simulator has short and long records): CIGARs and mismatch lists of every
    class, and a line of several records."""
    cig = size_classes([n for c in cases.values() for n in c[5]])
    mm = size_classes([n for c in cases.values() for n in c[6]])
    assert min(cig) > 0, cig
    assert min(mm) > 0, mm
    assert sum(c[7] for c in cases.values()) > 0


@pytest.mark.parametrize("one_kernel", [False, True])
@pytest.mark.parametrize("tags", TAG_SETS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_record_shapes(cases, name, tags, one_kernel):
    h, B, rd, plain, para = cases[name][:5]
    h.set_result_tags(tags)
    h.set_scratch_limit(128 << 10 if one_kernel else 0)             # with the limit every read overflows the phased pass and takes the one-kernel path
    try:
        got, st = h.align_batch(B)
        assert [int(x) for x in st] == [s[0] for s in plain]
        if one_kernel:
            assert h.last_kernel_ms(1) > 0
        for r in range(B.n_reads):
            g = T.split_events(got[r]) if tags & 1 else got[r]
            assert g == expected(tags, plain[r], rd[r], B, para), (name, tags, one_kernel, r)
    finally:
        h.set_scratch_limit(0)
        h.set_result_tags(0)
