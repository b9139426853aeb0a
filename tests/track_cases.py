"""Hand-made reads for branch tracking with the read's largest cluster in LDS (hp_track.h), test infrastructure shared by
tests/test_track_lds_cpu.py and tests/test_track_lds_gpu.py; the builders are those of tests/crafted.py.

What the reads rely on (preset "default": seed_len 50, seed_step 100, match_dis 5, first_loci_thd 2; chaining scores +2 per match-class edge, -2
per insertion / deletion-class edge):
  * a run of seeds with one exact hit each is one chain whose k-th node has score 2 k - 1;
  * on the '+' strand a hit that already has a match-class son takes no further son (son_flag, lamsa_dp_con.c:722); on the '-' strand the first
    match-class precursor in scan order wins outright (:726-733) and a hit may have any number of match-class sons -- the tie rules of
    get_max_son (:808) between match-class sons are therefore met on '-' reads;
  * two hits of one seed slot never connect, so both look for their predecessor among the earlier seeds.
The image holds six words per hit behind the leaf bits, one bit per seed slot: image_cap(W, seed_out) hits (at most 1020)."""

import crafted
import reflib
from crafted import Case, concat, crafted_batch, far_clusters, one_cluster, plain_read, sim_ref   # noqa: F401

SHAPES = reflib.CHAIN_LDS_WORDS
STEP = 100

# path counters of hp_track.h (slots listed in hp_core.h)
RESIDENT, ON_IMAGE, ON_HBM, STEPS, CUT2, NEG_WALK, NEG_CUT, LONG, MAX_RESIDENT, TIE_DIST, TIE_NM, SKIP_CLASS, UNPACKABLE, CUT3, ALL_MIN = 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63


def image_cap(W, seed_out):
    """Hits of the largest cluster that fit the image next to the leaf bits of seed_out seed slots in W words of LDS."""
    return min((W - ((seed_out - 1) // 32 + 1)) // 6, 1020)


def _len(n_seeds):
    return 50 + STEP * (n_seeds - 1)


def minus_read(ref, p0, n_seeds, hits_of_seed):
    """A '-' read: the reverse complement of the reference at p0.  hits_of_seed(k, true_pos) as in crafted_batch, true_pos being the 1-based
    leftmost reference coordinate of seed k of the reversed read (it falls by one step per seed)."""
    L = _len(n_seeds)
    B = crafted_batch(ref, p0, L, lambda s, t: hits_of_seed(s, p0 + L - (s - 1) * STEP - 50 + 1), step=STEP)
    B.read_seq[:L] = (3 - crafted.ref_bases(ref, p0, L))[::-1]
    B.h_strand[:] = -1
    return B


def neg_edge_walk(ref, n=24):
    """n colinear seeds, then one seed whose only hit lies 300 bases off the diagonal: a deletion-class edge (score 2 n - 1 - 2) below the end
    of the stretch.  The walk from that leaf meets a father with one son and a higher score: the negative edge of the walk."""
    return crafted_batch(ref, 300000, _len(n + 1), lambda s, t: [(t, 0, 0)] if s <= n else [(t + 300, 1, 0)], step=STEP)


def neg_edge_cut(ref, n=24):
    """The same stretch, and two hits of the next seed 300 and 600 bases off: two deletion-class sons of the stretch's end.  cut_branch keeps one,
    detaches the other, and the one it kept is still below its father: the negative edge of cut_branch."""
    return crafted_batch(ref, 300000, _len(n + 1), lambda s, t: [(t, 0, 0)] if s <= n else [(t + 300, 1, 0), (t + 600, 2, 0)], step=STEP)


def ties_nm(ref, n=24):
    """'-' strand.  The seed after the stretch has two hits on the diagonal, two bases apart, NM 2 and 0: both are match-class sons of the
    stretch's end.  get_max_son: the second ties the first on max_score and on seed distance and wins on max_NM."""
    return minus_read(ref, 300000, n + 1, lambda s, t: [(t, 0, 0)] if s <= n else [(t, 2, 0), (t + 2, 0, 0)])


def ties_class(ref, n=24):
    """'-' strand.  The seed after the stretch has a hit on the diagonal and one 300 bases off: a match-class son and, after it in hit order, a
    deletion-class son of the stretch's end (on the '+' strand the first would have closed its father to the second).  get_max_son holds the
    first and skips the second for its class."""
    return minus_read(ref, 300000, n + 1, lambda s, t: [(t, 0, 0)] if s <= n else [(t, 0, 0), (t + 300, 1, 0)])


def ties_distance(ref, n=24, nm_far=0):
    """'-' strand.  After the stretch, seed n + 1 has a hit 5 bases off the diagonal and seed n + 2 one 5 bases off the other way: each is match-class
    to the stretch's end (seed distance 1 and 2) and not to the other.  Two leaves, sons of one node, equal max_score, different seed distance;
    nm_far: NM of the farther one (below the nearer one's 1: it wins on max_NM although it is farther)."""
    def hits(s, t):
        if s <= n:
            return [(t, 0, 0)]
        return [(t + 5, 1, 0)] if s == n + 1 else [(t - 5, nm_far, 0)]
    return minus_read(ref, 300000, n + 2, hits)


def three_sons(ref, first, second, n=24):
    """'-' strand, ONE node with THREE sons.  After the stretch, seed n + 1 has the two hits `first` and seed n + 2 the hit `second`, given as
    (offset from the diagonal, NM).  A hit within 5 bases of the diagonal is a match-class son of the stretch's end when no hit of a seed in
    between is within 5 bases of it; a hit 300 bases off is its deletion-class son (the other hit of its seed slot cannot be its father).  The
    sons stand in the list in hit order, so get_max_son walks first -> next -> next, and cut_branch detaches two of them around the one it keeps."""
    def hits(s, t):
        if s <= n:
            return [(t, 0, 0)]
        return [(t + d, m, 0) for (d, m) in (first if s == n + 1 else [second])]
    return minus_read(ref, 300000, n + 2, hits)


def multi_in_cluster(ref, n=24):
    """Seeds 5 - 7 have four hits each (the exact one and three 100, 107, 114 bases off): more than first_loci_thd, so they are not MIN seeds, and
    with 21 MIN seeds of 24 the first pass is NOT all_min: the resident cluster holds hits that take no part in it (MULTI_FLAG), and the exact
    hits of those seeds join it through frag_min_extend."""
    return crafted_batch(ref, 300000, _len(n), lambda s, t: [(t, 0, 0)] + ([(t + 100 + 7 * j, 1, 0) for j in range(3)] if 5 <= s <= 7 else []), step=STEP)


def heavy_nm(ref, n=24):
    """A cluster whose NM sum is beyond 16 bits: three more hits of NM 30 000 around the diagonal of seeds 3 - 5 (they lose every comparison)."""
    return crafted_batch(ref, 300000, _len(n), lambda s, t: [(t, 0, 0)] + ([(t + 3, 30000, 0)] if 3 <= s <= 5 else []), step=STEP)


def second_locus(ref, far=800000):
    """The true locus (24 seeds; seeds 11 - 13 and 21 - 23 have a second hit 300 bases off the diagonal, listed first: a deletion-class son of the
    seed before, a leaf of the resident cluster) and two more loci with colinear runs on seeds 3 - 10 and 14 - 20.  No seed has more than two
    hits, so every hit takes part in the first pass.  Last seed slot to first, the tracks start at resident hits (24 .. 21), at the third locus
    (20), at resident hits (13 .. 11), at the second locus (10): the end nodes of three clusters interleave on the stack."""
    def hits(s, t):
        if 3 <= s <= 10:
            return [(t, 0, 0), (t + far, 0, 0)]
        if 14 <= s <= 20:
            return [(t, 0, 0), (t + 2 * far, 0, 0)]
        if 11 <= s <= 13 or 21 <= s <= 23:
            return [(t + 300, 1, 0), (t, 0, 0)]
        return [(t, 0, 0)]
    return crafted_batch(ref, 300000, _len(24), hits, step=STEP)


def capacity_read(ref, n_hits):
    """One cluster of n_hits hits over 52 seed slots (crafted.one_cluster, preset ont2d)."""
    return one_cluster(ref, n_hits)


def sim_ont_reads(n=16):
    """n simulated 10-kbp ONT reads against a 20-Mbp stand-in (tools/simbatch.py): the reads of the issue's counts."""
    import simbatch
    ref = simbatch.SimRef(20_000_000, seed=5, threads=2)
    return ref, simbatch.SimBatch(ref, n, 10000, "ont2d", seed=1000, threads=2)


def cases(W):
    """(key, read type, reference key, batch, expectations over the path counters of a phased run under W words, aim)."""
    A, Bf = sim_ref("a"), sim_ref("b")
    cap = image_cap(W, 52)
    out = []

    def add(key, rt, ref_key, batch, expect, aim):
        out.append(Case(key, rt, ref_key, batch, expect, aim))
    add("image-cap", "ont2d", "a", capacity_read(A, cap), [(RESIDENT, "==", 1), (MAX_RESIDENT, "==", cap), (ON_IMAGE, ">", 0), (ON_HBM, "==", 0)], "largest cluster of %d hits = the image's capacity" % cap)
    add("image-cap+1", "ont2d", "a", capacity_read(A, cap + 1), [(RESIDENT, "==", 0), (ON_IMAGE, "==", 0), (UNPACKABLE, "==", 0)], "largest cluster of %d hits: one more than fits" % (cap + 1))
    add("second-locus", "default", "b", second_locus(Bf), [(RESIDENT, "==", 1), (MAX_RESIDENT, "==", 30), (ON_IMAGE, ">=", 7), (ON_HBM, "==", 2), (CUT2, ">", 0)], "resident tracks and HBM tracks interleaved by seed slot")
    add("ties-nm", "default", "a", ties_nm(A), [(RESIDENT, "==", 1), (CUT2, ">", 0), (TIE_NM, ">", 0)], "'-' strand: two sons tie on max_score and seed distance, max_NM decides")
    add("ties-class", "default", "a", ties_class(A), [(RESIDENT, "==", 1), (CUT2, ">", 0), (SKIP_CLASS, ">", 0)], "'-' strand: a son beyond F_MATCH_THD after one within")
    add("ties-distance", "default", "a", ties_distance(A, nm_far=1), [(RESIDENT, "==", 1), (CUT2, ">", 0), (TIE_DIST, ">", 0)], "'-' strand: tie on max_score, different seed distance, equal max_NM")
    add("ties-distance-nm", "default", "a", ties_distance(A, nm_far=0), [(RESIDENT, "==", 1), (CUT2, ">", 0), (TIE_DIST, ">", 0)], "'-' strand: tie on max_score, the farther son has the lower max_NM")
    # one node with three sons: [match +5, deletion, match -5 with the lower NM]: the second is skipped for its class, the third ties the first on
    # max_score at another seed distance and wins on max_NM -- the kept son is the LAST of the list, two losers before it
    add("three-sons-last", "default", "a", three_sons(A, [(5, 1), (300, 1)], (-5, 0)), [(RESIDENT, "==", 1), (CUT3, "==", 1), (SKIP_CLASS, "==", 1), (TIE_DIST, "==", 1)],
        "'-' strand: three sons, class skip and distance tie in one list, the last son kept")
    # [deletion, match +5, match -5 with the same NM]: the kept son is the MIDDLE one, a loser detached on either side of it
    add("three-sons-middle", "default", "a", three_sons(A, [(300, 1), (5, 1)], (-5, 1)), [(RESIDENT, "==", 1), (CUT3, "==", 1), (TIE_DIST, "==", 1), (SKIP_CLASS, "==", 0)],
        "'-' strand: three sons, the middle son kept")
    # [match +3 NM 2, match +5 NM 0, match -5 NM 0]: the second ties the first on max_score and distance and wins on max_NM, the third ties on max_score
    add("three-sons-nm", "default", "a", three_sons(A, [(3, 2), (5, 0)], (-5, 0)), [(RESIDENT, "==", 1), (CUT3, "==", 1), (TIE_NM, "==", 1), (TIE_DIST, "==", 1)],
        "'-' strand: three match-class sons, both tie rules in one list")
    add("all-min", "ont2d", "a", capacity_read(A, 132), [(RESIDENT, "==", 1), (ALL_MIN, "==", 1), (MAX_RESIDENT, "==", 132)], "12 MIN seeds of 52: the first pass takes every hit (all_min)")
    add("not-all-min", "default", "a", multi_in_cluster(A), [(RESIDENT, "==", 1), (ALL_MIN, "==", 0), (MAX_RESIDENT, "==", 33)], "21 MIN seeds of 24: MULTI hits inside the resident cluster")
    add("neg-edge-walk", "default", "a", neg_edge_walk(A), [(RESIDENT, "==", 1), (NEG_WALK, ">", 0)], "negative edge met in the walk")
    add("neg-edge-cut", "default", "a", neg_edge_cut(A), [(RESIDENT, "==", 1), (CUT2, ">", 0), (NEG_CUT, ">", 0)], "negative edge met in cut_branch")
    add("long-chain", "default", "a", plain_read(A, 80, step=STEP), [(RESIDENT, "==", 1), (LONG, ">", 0), (STEPS, ">=", 79)], "a chain of 80 nodes on the image")
    add("heavy-nm", "default", "a", heavy_nm(A), [(RESIDENT, "==", 0), (UNPACKABLE, "==", 1), (ON_IMAGE, "==", 0)], "NM sum of the largest cluster beyond 16 bits")
    return out


CASE_KEYS = ["image-cap", "image-cap+1", "second-locus", "ties-nm", "ties-class", "ties-distance", "ties-distance-nm", "three-sons-last", "three-sons-middle", "three-sons-nm", "all-min", "not-all-min", "neg-edge-walk", "neg-edge-cut", "long-chain", "heavy-nm"]
