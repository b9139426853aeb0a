"""Hand-made reads for the main chaining pass on diagonal keys (dp_cluster_lds / cl_targets, cluster_lane, gap_dp_core: hp_cluster.h, hp_gaps.h),
test infrastructure shared by tests/test_edge_cpu.py and tests/test_edge_gpu.py; the builders are those of tests/crafted.py and
tests/track_cases.py.

What the reads rely on (preset "default": seed_len 50, seed_step 100, match_dis 5, first_loci_thd 2; "ont2d": seed_step 25):
  * dp_cluster_lds scans the candidates of a target in blocks of 64 consecutive ranks of the (contig, strand, position) order; lane b of its
    `bmin` holds the smallest seed slot of block b, and a block none of whose hits is of an earlier seed than the target is not read;
  * on the '+' strand a hit that already has a match-class son takes no further son (lamsa_dp_con.c:718-720); on the '-' strand the first
    match-class precursor in scan order (seeds descending, hits ascending) wins outright (:726-733);
  * candidates equal in score and NM are told apart by scan order; when one lane holds the target's maximum there is nothing to tell apart.
Path counters (slots of hp_core.h): 32 clusters through dp_cluster_lds, 33 clusters that did not fit or pack (the HBM way), 34 clusters of two to
six hits on a lane (cluster_lane), 40 / 47 the largest cluster of either kind, 2 gaps on a lane (gap_dp_core), 4 gaps through the wave-wide DP."""

import crafted
import reflib
import track_cases
from crafted import Case, crafted_batch, far_clusters, one_cluster, plain_read, sim_ref   # noqa: F401
from track_cases import minus_read

SHAPES = reflib.CHAIN_LDS_WORDS
STEP = 100

LDS_CL, BIG_CL, LANE_CL, MAX_LDS, MAX_LANE, GAP_LANE, GAP_WAVE = 32, 33, 34, 40, 47, 2, 4


def n_lines(stream):
    """Lines of a read's result stream (word 0 is its status)."""
    return int(stream[1]) if len(stream) > 1 and stream[0] == 0 else 0


def _len(n_seeds):
    return 50 + STEP * (n_seeds - 1)


def both_strands(ref, P):
    """A '+' read with its true locus (12 hits) and a second locus of 8 colinear hits that are marked '-': a '+' and a '-' cluster of more than
    six hits each in one read, so both bodies of the target loop run for it (the '-' one on candidates that are colinear for a '+' read: its
    bookkeeping runs, its winners are few; minus_two_precursors is the '-' read whose edges connect)."""
    B = far_clusters(ref, P, [8])
    far = abs(B.h_pos[:B.n_hits] - B.h_pos[0]) > 4000
    assert int(far.sum()) == 8
    B.h_strand[:B.n_hits][far] = -1
    return B


def minus_two_precursors(ref, n=26):
    """'-' strand, one hit per seed except seed 12, which has two hits two bases apart on the diagonal: the hit of seed 13 has two match-class
    precursors in one seed slot (and more in the slots before); the first in scan order -- the lower hit -- must win outright."""
    return minus_read(ref, 300000, n, lambda s, t: [(t, 0, 0), (t + 2, 0, 0)] if s == 12 else [(t, 0, 0)])


def plus_taken_father(ref, n=24):
    """'+' strand, seed 12 has two hits three bases apart: the first takes the hit of seed 11 as its father, a match-class edge, so that hit is closed
    to the second (:718-720), which has to go one seed further back."""
    return crafted_batch(ref, 300000, _len(n), lambda s, t: [(t, 0, 0), (t + 3, 1, 0)] if s == 12 else [(t, 0, 0)], step=STEP)


def scan_order_tie(ref, n=24):
    """'+' strand.  Seed 1 has two hits four bases apart, neither with a predecessor (score 1, NM 0 both); the hit of seed 2 lies two bases off
    either diagonal: two match-class candidates equal in score and NM, held by two lanes: scan order -- the lower hit -- decides.  Every later
    target's maximum is held by one lane."""
    def hits(s, t):
        if s == 1:
            return [(t, 0, 0), (t + 4, 0, 0)]
        return [(t + 2, 0, 0)]
    return crafted_batch(ref, 300000, _len(n), hits, step=STEP)


def cases(W):
    """(key, read type, reference key, batch, expectations over the path counters of a phased run under W words, aim)."""
    A, Bf = sim_ref("a"), sim_ref("b")
    Pd = reflib.lo_para("default")
    cap = W // 5
    out = []

    def add(key, rt, ref_key, batch, expect, aim):
        out.append(Case(key, rt, ref_key, batch, expect, aim))
    add("lane-6-wave-7", "default", "b", far_clusters(Bf, Pd, [6, 7]), [(LANE_CL, "==", 1), (MAX_LANE, "==", 6), (LDS_CL, "==", 2), (MAX_LDS, "==", 12), (BIG_CL, "==", 0)],
        "a cluster of 6 hits (the last on a lane) and one of 7 (the first through dp_cluster_lds)")
    for n in (64, 65, 129):
        add("block-%d" % n, "ont2d", "a", one_cluster(A, n), [(LDS_CL, "==", 1), (MAX_LDS, "==", n), (BIG_CL, "==", 0)],
            "one cluster of %d hits: %d blocks of the scan, the last of %d; early targets skip the blocks of later seeds" % (n, (n + 63) // 64, (n - 1) % 64 + 1))
    add("cap", "ont2d", "a", one_cluster(A, cap), [(LDS_CL, "==", 1), (MAX_LDS, "==", cap), (BIG_CL, "==", 0)], "one cluster of lds_words / 5 = %d hits" % cap)
    add("cap+1", "ont2d", "a", one_cluster(A, cap + 1), [(LDS_CL, "==", 0), (BIG_CL, "==", 1)], "one cluster of %d hits: one more than fits" % (cap + 1))
    add("both-strands", "default", "b", both_strands(Bf, Pd), [(LDS_CL, "==", 2), (MAX_LDS, "==", 12), (BIG_CL, "==", 0)], "a '+' and a '-' cluster in one read")
    add("minus-two-precursors", "default", "a", minus_two_precursors(A), [(LDS_CL, "==", 1), (MAX_LDS, "==", 27), (BIG_CL, "==", 0)], "'-': two match-class precursors, the first in scan order wins")
    add("plus-taken-father", "default", "a", plus_taken_father(A), [(LDS_CL, "==", 1), (MAX_LDS, "==", 25), (BIG_CL, "==", 0)], "'+': a candidate that already has a match son")
    add("scan-order-tie", "default", "a", scan_order_tie(A), [(LDS_CL, "==", 1), (MAX_LDS, "==", 25), (BIG_CL, "==", 0)], "'+': two candidates equal in score and NM; maxima held by two lanes and by one")
    add("all-min", "ont2d", "a", one_cluster(A, 132), [(LDS_CL, "==", 1), (MAX_LDS, "==", 132), (track_cases.ALL_MIN, "==", 1)], "12 MIN seeds of 52: the first pass takes every hit (all_min)")
    add("min-extension", "default", "a", track_cases.multi_in_cluster(A), [(LDS_CL, "==", 1), (MAX_LDS, "==", 33), (track_cases.ALL_MIN, "==", 0)],
        "21 MIN seeds of 24, MULTI hits in the cluster: the MIN extension of dp_cluster_lds runs")
    add("gap-on-a-lane", "default", "a", plain_read(A, 20, step=STEP, gaps=(10,), gap_hits=6), [(GAP_LANE, "==", 1), (GAP_WAVE, "==", 0), (LDS_CL, "==", 1)],
        "a line whose gap (6 survivors) runs through gap_dp_core")
    assert [c.key for c in out] == CASE_KEYS
    return out


CASE_KEYS = ["lane-6-wave-7", "block-64", "block-65", "block-129", "cap", "cap+1", "both-strands", "minus-two-precursors", "plus-taken-father", "scan-order-tie",
             "all-min", "min-extension", "gap-on-a-lane"]
