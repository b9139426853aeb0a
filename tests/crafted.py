"""Hand-made reads (test infrastructure): one '+' read copied from the stand-in reference with seed hits written by hand, so that a read
takes a branch, or meets a capacity of the chaining kernels exactly, that no simulated or GEM-seeded read of the corpus does.

The capacities follow from the LDS words W of a wave of the chaining kernels (2432 / 3392 / 5120, hp_align_api.hip):
  W / 5 hits         a cluster chained out of LDS (dp_cluster_lds) or through HBM (dp_update_range with C.big)   hp_chain.h: chain_first
  2 .. 6 hits        a cluster handled by one lane (cluster_lane), 63 clusters per step of the loop               hp_chain.h: chain_first
  2 * W seed slots   the gaps of a line by cluster (slot table in LDS) or by seed range                           hp_gaps.h: gaps_by_cluster
  6 survivors        a gap's mini DP on one lane or wave-wide; 256 listed hits in registers or through memory     hp_gaps.h
  6 gaps             lines with fewer leave the lanes alone when the gaps are scanned by seed range (HP_GAP_MIN)  hp_gaps.h: line_build
  1024 hits          one block of the bitonic sort in LDS (HP_SORT_BLOCK; W / 2 words are handed to it)           hp_sort.h
  13 * (n + 1) + 64 <= W    the per-line arrays of n lines staged in LDS (lset_stage)                             hp_chain.h
A generator takes the number it aims at; what a read really produced is read off the path counters of the CPU build (HP_STAT /
HP_STAT_MAX, hp_core.h) by tests/test_capacity_cpu.py, which asserts it.  Every case carries those expectations as (slot, op, value)."""
import os
import sys

import numpy as np

import reflib

sys.path.insert(0, os.path.join(reflib.ROOT, "tools"))

SHAPES = reflib.CHAIN_LDS_WORDS
_refs = {}


def sim_ref(key="a"):
    """'a': the 2-Mbp stand-in of tests/test_path_cpu.py; 'b': 8 Mbp without repeats, room for some four hundred loci further apart than a read's
    cluster reach."""
    import simbatch
    if key not in _refs:
        _refs[key] = simbatch.SimRef(2_000_000, n_contigs=1, seed=9, threads=2) if key == "a" else simbatch.SimRef(8_000_000, n_contigs=1, seed=3, threads=2, repeats=False)
    return _refs[key]


def ref_bases(ref, p0, n):
    k = np.arange(p0, p0 + n, dtype=np.int64)
    return ((ref.pac[k >> 2] >> ((~k & 3) << 1)) & 3).astype(np.uint8)                      # _get_pac, src/bntseq.c:242


def crafted_batch(ref, p0, L, hits_of_seed, step=25, seed_len=50):
    """One '+' read copied from contig 1 of `ref` at 0-based offset p0, with hand-made seed hits: hits_of_seed(k, true_pos) -> list of
    (pos, nm, len_dif) for the 1-based seed k whose exact hit is at 1-based true_pos (an empty list: the seed has no slot)."""
    class _B:
        pass
    b = _B()
    k = np.arange(p0, p0 + L, dtype=np.int64)
    read = (ref.pac[k >> 2] >> ((~k & 3) << 1)) & 3                                         # _get_pac, src/bntseq.c:242
    seed_all = (L - seed_len) // step + 1
    seed_id, hit_off, pos, nm, ld = [], [0], [], [], []
    for s in range(1, seed_all + 1):
        hs = hits_of_seed(s, p0 + (s - 1) * step + 1)
        if not hs:
            continue
        seed_id.append(s); hit_off.append(hit_off[-1] + len(hs))
        for (p, m, d) in hs:
            pos.append(p); nm.append(m); ld.append(d)
    nh = len(pos)
    b.n_reads = 1
    b.read_off = np.array([0, L], np.int64); b.read_seq = np.concatenate([read.astype(np.uint8), np.zeros(8, np.uint8)])
    b.seed_all = np.array([seed_all, 0], np.int32); b.last_len = np.array([L - seed_len - (seed_all - 1) * step, 0], np.int32)
    b.seed_off = np.array([0, len(seed_id)], np.int64); b.seed_id = np.array(seed_id + [0] * 4, np.int32); b.hit_off = np.array(hit_off, np.int64)
    b.h_pos = np.array(pos + [0] * 4, np.int64); b.h_chr = np.ones(nh + 4, np.int32); b.h_strand = np.ones(nh + 4, np.int8)
    b.h_nm = np.array(nm + [0] * 4, np.int16); b.h_len_dif = np.array(ld + [0] * 4, np.int16)
    b.h_cig_off = np.arange(nh + 4, dtype=np.int32); b.h_cig_n = np.ones(nh + 4, np.uint8); b.cig = np.full(nh + 8, (seed_len << 4) | 0, np.int32)
    b.n_slots, b.n_hits, b.n_cig = len(seed_id), nh, nh
    b.pac, b.l_pac, b.seq_off, b.seq_len = ref.pac, ref.l_pac, ref.seq_off, ref.seq_len
    return b


def concat(batches, seed_len=50):
    """One-read batches over the same reference as one batch (every crafted hit has the one-element seed CIGAR <seed_len>M)."""
    class _B:
        pass
    b = _B()
    n = len(batches)
    lens = [int(x.read_off[1]) for x in batches]; ns = [int(x.n_slots) for x in batches]; nh = [int(x.n_hits) for x in batches]
    b.n_reads = n
    b.read_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    b.read_seq = np.concatenate([x.read_seq[:l] for x, l in zip(batches, lens)] + [np.zeros(8, np.uint8)])
    b.seed_all = np.array([int(x.seed_all[0]) for x in batches] + [0], np.int32); b.last_len = np.array([int(x.last_len[0]) for x in batches] + [0], np.int32)
    b.seed_off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    b.seed_id = np.concatenate([x.seed_id[:k] for x, k in zip(batches, ns)] + [np.zeros(4, np.int32)]).astype(np.int32)
    hit_off = [np.zeros(1, np.int64)]; base = 0
    for x, k, h in zip(batches, ns, nh):
        hit_off.append(x.hit_off[1:k + 1] + base); base += h
    b.hit_off = np.concatenate(hit_off).astype(np.int64)
    for name in ("h_pos", "h_chr", "h_strand", "h_nm", "h_len_dif"):
        dt = getattr(batches[0], name).dtype
        setattr(b, name, np.concatenate([getattr(x, name)[:h] for x, h in zip(batches, nh)] + [np.zeros(4, dt)]).astype(dt))
    H = base
    b.h_cig_off = np.arange(H + 4, dtype=np.int32); b.h_cig_n = np.ones(H + 4, np.uint8); b.cig = np.full(H + 8, (seed_len << 4) | 0, np.int32)
    b.n_slots, b.n_hits, b.n_cig = int(sum(ns)), H, H
    x = batches[0]
    b.pac, b.l_pac, b.seq_off, b.seq_len = x.pac, x.l_pac, x.seq_off, x.seq_len
    return b


def _read_len(n_seeds, step, seed_len=50):
    return seed_len + step * (n_seeds - 1)


# ---------------------------------------------------------------- the three reads of tests/test_path_cpu.py
def tandem_repeat_gap(ref, far):
    """Two anchors 35 seed slots apart with 34 repetitive seeds in between, every one of their 30 hits within reach of the left anchor; with
    `far` the second half of the hits of every repetitive seed lies at a second locus."""
    def hits(s, t):
        if s <= 5 or s >= 40:
            return [(t, 0, 0)]
        out = [(t + 3 * j - 40, j % 4, 0) for j in range(30)]
        out[13] = (t, 0, 0)
        if far:
            out = out[:15] + [(p + far, m, d) for (p, m, d) in out[15:]]
        return out
    return crafted_batch(ref, 300000, 1500, hits)


def bare_insertion(ref, ins, rng):
    """`ins` foreign bases spliced into the read exactly between two seeds: a junction with read bases and no reference base."""
    p0, cut, L = 400000, 500, 1000 + ins

    def hits(s, t):
        o = (s - 1) * 25                                            # read offset of the seed
        if o + 50 <= cut:
            return [(p0 + o + 1, 0, 0)]
        if o >= cut + ins:
            return [(p0 + o - ins + 1, 0, 0)]
        return []                                                   # a seed that touches the inserted bases has no hit
    B = crafted_batch(ref, p0, L, hits)
    flank = ref_bases(ref, p0, 1000)
    B.read_seq[:L] = np.concatenate([flank[:cut], rng.integers(0, 4, ins, dtype=np.uint8), flank[cut:]])
    return B


def dumped_edge_cluster(ref):
    """The last two seeds hit two other loci and nothing else: a cluster of two two-node lines at the edge of the read that line_filter dumps."""
    def hits(s, t):
        if s <= 12:
            return [(t, 0, 0)]
        if s <= 14:
            return [(t + far, 1, 0) for far in (500000, 700000)]               # two hits: a seed of at most first_loci_thd hits takes part in the main pass
        return []
    return crafted_batch(ref, 300000, 1550, hits, step=100)


# ---------------------------------------------------------------- capacity edges
def one_cluster(ref, n_hits, n_mid=40, step=25, p0=300000):
    """A tandem-repeat locus: six single-hit seeds on either side of n_mid repetitive seeds that share n_hits - 12 hits as evenly as they can,
    three bases apart around the exact one -- all n_hits hits of the read within `cluster_reach` of each other: ONE cluster of n_hits hits."""
    n_seeds = n_mid + 12
    per, extra = divmod(n_hits - 12, n_mid)
    assert per >= 1

    def hits(s, t):
        if s <= 6 or s > 6 + n_mid:
            return [(t, 0, 0)]
        c = per + (1 if s - 7 < extra else 0)
        out = [(t + 3 * (j - c // 2), 1 + j % 3, 0) for j in range(c)]
        out[c // 2] = (t, 0, 0)
        return out
    return crafted_batch(ref, p0, _read_len(n_seeds, step), hits, step=step)


def reach_of(P, n_seeds):
    """cluster_reach (hp_cluster.h) of a read whose seed slots span n_seeds seeds."""
    did = n_seeds - 1
    mdm = P.match_dis * (did if (P.aln_mode & 2) else 1)
    R = max(P.SV_len_thd, did * P.seed_step, mdm + 1) + 128 + did * P.seed_step
    return max(R, did * (P.seed_step + P.match_dis) + 256)


def far_clusters(ref, P, sizes, n_seeds=12, lone=0, p0=100000, big=0):
    """A read of n_seeds seeds, every one with its exact hit, and one cluster of sizes[k] colinear hits (consecutive seeds, one hit each) at locus k
    -- the loci further apart than the read's cluster reach -- plus `lone` single hits at loci of their own: 1 + len(sizes) + lone clusters.  Every
    seed ends up with more than first_loci_thd hits when there are enough loci, so every hit is a MIN hit and every locus makes a line.
    big: this many more hits around the exact ones (three bases apart), which all join the cluster of the read's true locus."""
    step = P.seed_step
    L = _read_len(n_seeds, step)
    gap = reach_of(P, n_seeds) + L + 1000
    per_seed = [[] for _ in range(n_seeds + 1)]
    first = p0 + 2 * gap
    for k, z in enumerate(list(sizes) + [1] * lone):
        assert 1 <= z <= n_seeds
        s0 = 1 + (k * 3) % (n_seeds - z + 1)
        for s in range(s0, s0 + z):
            per_seed[s].append(first + k * gap + (s - 1) * step + 1)
    assert first + (len(sizes) + lone) * gap + L < ref.l_pac, "the reference has no room for %d loci" % (len(sizes) + lone)
    for i in range(big):
        s = 1 + i % n_seeds; j = 1 + i // n_seeds
        per_seed[s].append(p0 + (s - 1) * step + 1 + 3 * j)

    def hits(s, t):
        return [(t, 0, 0)] + [(p, 1 if abs(p - t) < 4000 else 0, 0) for p in per_seed[s]]
    return crafted_batch(ref, p0, L, hits, step=step)


def plain_read(ref, n_seeds, step=25, gaps=(), gap_hits=3, extra_hits=0, p0=300000):
    """A read of n_seeds seeds with one exact hit each -- n_seeds seed slots, n_seeds hits -- except the (1-based) seeds in `gaps`: those have
    gap_hits hits 100, 107, 114, ... bases off the diagonal and none on it, so the read's line has a gap there whose mini DP finds gap_hits
    candidates (deletion-class edges from the gap's head).  extra_hits: that many more off-diagonal hits on seed 3 (more hits, same slots)."""
    gaps = set(gaps)

    def hits(s, t):
        if s in gaps:
            return [(t + 100 + 7 * j, 1, 0) for j in range(gap_hits)]
        if s == 3 and extra_hits:
            return [(t, 0, 0)] + [(t + 100 + 7 * j, 1, 0) for j in range(extra_hits)]
        return [(t, 0, 0)]
    return crafted_batch(ref, p0, _read_len(n_seeds, step), hits, step=step)


def wide_gap(ref, n_listed, n_mid=9, step=100, p0=300000):
    """Five anchors on either side of n_mid seeds that have no hit on the diagonal and n_listed hits between them, all of them candidates of
    the one gap's mini DP: the wave-wide routine lists n_listed hits (256 fit its registers)."""
    per, extra = divmod(n_listed, n_mid)

    def hits(s, t):
        if s <= 5 or s > 5 + n_mid:
            return [(t, 0, 0)]
        c = per + (1 if s - 6 < extra else 0)
        return [(t + 100 + 7 * j, 1, 0) for j in range(c)]
    return crafted_batch(ref, p0, _read_len(n_mid + 10, step), hits, step=step)


def spread_read(ref, P, n_seeds, p0=200000, spacing=900000):
    """A read of n_seeds seeds with ONE exact hit per seed -- n_seeds seed slots -- made of k stretches copied from k loci `spacing` bases apart
    (a rearranged read): the gap pass by cluster gives up on a cluster whose span may not fit 30 bits ((hits - 1) * cluster_reach, hp_gaps.h),
    and a read of thousands of seeds from one locus is such a cluster whatever its slot count.  Every stretch is a cluster of n_seeds / k hits
    with lines of its own.  The shortest read of that many slots: seed_len + (n_seeds - 1) * step."""
    step = P.seed_step
    reach = reach_of(P, n_seeds)
    k = 2
    while (n_seeds // k + 1) * reach > 0x3fffffff:
        k += 1
    L = _read_len(n_seeds, step)
    assert spacing > reach + L and p0 + (k - 1) * spacing + L < ref.l_pac
    blk = -(-n_seeds // k)                                           # seeds per stretch

    def hits(s, t):
        return [(t + ((s - 1) // blk) * spacing, 0, 0)]
    B = crafted_batch(ref, p0, L, hits, step=step)
    for b in range(1, k):
        o0, o1 = b * blk * step, min(L, (b + 1) * blk * step)
        B.read_seq[o0:o1] = ref_bases(ref, p0 + b * spacing + o0, o1 - o0)
    return B


def few_gaps_read(ref, n_seeds, n_anchors, step=50, p0=200000, far=4000000):
    """A read of n_seeds abutting seeds (seed_len = seed_step = 50: neighbours connect, the read's own line has no gap and never enters the gap
    pass) of which n_anchors -- every other seed from seed 101 on -- have a second hit at a far locus: one more line, with a gap after START, one
    between every two anchors and one beyond its end node: n_anchors + 1 gaps, all but the first with a head."""
    second = {101 + 2 * i for i in range(n_anchors)}

    def hits(s, t):
        return [(t, 0, 0)] + ([(t + far, 0, 0)] if s in second else [])
    return crafted_batch(ref, p0, _read_len(n_seeds, step), hits, step=step)


class Case:
    def __init__(self, key, read_type, ref_key, batch, expect, aim, over=()):
        self.key, self.read_type, self.ref_key, self.batch, self.expect, self.aim = key, read_type, ref_key, batch, expect, aim
        self.over = tuple(over)                    # parameters other than the preset's, as (name, value) pairs
        self.seed_out = int(batch.n_slots); self.H = int(batch.n_hits)


def lset_limit(W):
    """The largest number of lines lset_stage (hp_chain.h) keeps in LDS: 13 arrays of n + 1 words and 64 spare words must fit W."""
    return (W - 64) // 13 - 1


# the cases of cases(W), by names that do not depend on W (cap = W / 5, half = W / 2)
BIG_KEYS = ["gaptab-2W", "gaptab-2W+1", "gaptab-2W+1-5gaps", "gaptab-2W+1-6gaps"]
CASE_KEYS = ["cluster-cap-1", "cluster-cap", "cluster-cap+1", "cluster-mix"] + ["clusters-%d" % n for n in (62, 63, 64, 126, 127)] + \
            ["slots-%d" % n for n in (63, 64, 65, 128, 129)] + ["hits-64", "hits-65"] + ["sort-half-1", "sort-half", "sort-half+1", "sort-1023", "sort-1024", "sort-1025"] + \
            BIG_KEYS + ["survivors-6", "survivors-7", "listed-255", "listed-256", "listed-257", "lines-fit", "lines-fit+1",
                        "tandem-repeat-gap", "bare-insertion", "dumped-edge-cluster"]


def cases(W, big_reads=True):
    """The capacity-edge reads for chaining kernels with W words of LDS per wave, in the order of CASE_KEYS.  Case.expect: (slot, op, value) over
    the path counters of a run of that one read under W (slots: hp_core.h).  big_reads=False leaves out BIG_KEYS, the reads of 2 * W seed slots
    and more."""
    P = {rt: reflib.lo_para(rt) for rt in ("default", "ont2d")}
    abut = (("seed_step", 50),)
    A, Bf = sim_ref("a"), sim_ref("b")
    cap, half = W // 5, W // 2
    out = []

    def add(key, rt, ref_key, batch, expect, aim, over=()):
        out.append(Case(key, rt, ref_key, batch, expect, aim, over))
    # a. one cluster of cap - 1 / cap / cap + 1 hits
    for key, n in (("cluster-cap-1", cap - 1), ("cluster-cap", cap), ("cluster-cap+1", cap + 1)):
        fits = n <= cap
        add(key, "ont2d", "a", one_cluster(A, n),
            [(48, "==", 1)] + ([(32, "==", 1), (33, "==", 0), (40, "==", n)] if fits else [(33, "==", 1), (41, "==", n), (32, "==", 0)]), "one cluster of %d hits (cap %d)" % (n, cap))
    #    one oversize cluster next to LDS-sized ones, lane-sized ones and lone hits: dp_update_range with a partly set C.big
    add("cluster-mix", "default", "b", far_clusters(Bf, P["default"], [12, 9, 7, 6, 5, 4, 3, 2, 2, 12, 8], n_seeds=12, lone=5, big=cap + 1 - 12),
        [(33, "==", 1), (41, "==", cap + 1), (32, "==", 5), (34, "==", 6), (48, "==", 17)], "one cluster of cap + 1 = %d hits, 5 of 7 .. 12, 6 of 2 .. 6, 5 lone hits" % (cap + 1))
    # b. clusters of 2, 6 and 7 hits; 62 .. 127 clusters in one read (63 per step of the loop)
    for ncl in (62, 63, 64, 126, 127):
        sizes = [2, 6, 7] + [2] * (ncl - 4)
        add("clusters-%d" % ncl, "default", "b", far_clusters(Bf, P["default"], sizes),
            [(48, "==", ncl), (34, "==", ncl - 2), (47, "==", 6), (32, "==", 2), (33, "==", 0)], "%d clusters: 12 hits, 7 hits, the others 2 .. 6 (one per lane)" % ncl)
    # c. 64-wide ballot loops over the seed slots and over the hits
    for n in (63, 64, 65, 128, 129):
        add("slots-%d" % n, "ont2d", "a", plain_read(A, n, gaps=(n // 2,)), [(0, ">", 0), (1, "==", 0)], "seed_out %d" % n)
    for h in (64, 65):
        add("hits-%d" % h, "ont2d", "a", plain_read(A, 60, extra_hits=h - 60), [], "H %d over 60 seed slots" % h)
    # d. the LDS handed to the two sorts (W / 2 64-bit words) and the block they really sort in LDS (HP_SORT_BLOCK = 1024): clusters_build and
    #    build_sons sort H elements in one block up to 1024 and in several beyond, whatever W is
    for key, h in (("sort-half-1", half - 1), ("sort-half", half), ("sort-half+1", half + 1), ("sort-1023", 1023), ("sort-1024", 1024), ("sort-1025", 1025)):
        add(key, "ont2d", "a", one_cluster(A, h, n_mid=100), [(37, "==", 3), (38, "==", 0)] if h <= 1024 else [(38, "==", 3), (37, "==", 0)], "H %d (W / 2 = %d)" % (h, half))
    # e. the slot table of the gap pass: 2 * W seed slots by cluster, one more by seed range; f. HP_GAP_MIN, which only the scan by seed range looks at
    if big_reads:
        add("gaptab-2W", "ont2d", "b", spread_read(Bf, P["ont2d"], 2 * W), [(0, ">", 0), (1, "==", 0)], "seed_out %d = 2 * W" % (2 * W))
        add("gaptab-2W+1", "ont2d", "b", spread_read(Bf, P["ont2d"], 2 * W + 1), [(1, ">", 0), (0, "==", 0)], "seed_out %d = 2 * W + 1" % (2 * W + 1))
        for g in (5, 6):
            add("gaptab-2W+1-%dgaps" % g, "default", "b", few_gaps_read(Bf, 2 * W + 1, g - 1),
                [(1, "==", 1), (0, "==", 0), (45, "==", g), (39, "==", g - 1 if g >= 6 else 0)], "seed_out %d, the only line with gaps has %d" % (2 * W + 1, g), abut)
    # f. survivors of a gap: 6 on a lane, 7 wave-wide; 255 / 256 listed hits in registers, 257 through memory
    for m in (6, 7):
        add("survivors-%d" % m, "default", "a", plain_read(A, 20, step=100, gaps=(10,), gap_hits=m),
            [(0, ">", 0)] + ([(2, "==", 1), (43, "==", 6), (4, "==", 0)] if m == 6 else [(4, "==", 1), (42, "==", 7), (2, "==", 0)]), "a gap with %d survivors" % m)
    for m in (255, 256, 257):
        add("listed-%d" % m, "default", "a", wide_gap(A, m), [(4, "==", 1), (42, "==", m)] + ([(5, "==", 0)] if m <= 256 else [(5, "==", 1)]), "a gap with %d listed hits" % m)
    # g. lset_stage: 13 * (lines + 1) + 64 <= W
    nl = lset_limit(W)
    for key, n in (("lines-fit", nl), ("lines-fit+1", nl + 1)):
        add(key, "default", "b", far_clusters(Bf, P["default"], [2] * (n - 1)),
            [(44, "==", n)] + ([(35, "==", 1), (36, "==", 0)] if n <= nl else [(36, "==", 1), (35, "==", 0)]), "%d lines (lset_stage holds %d)" % (n, nl))
    # h. the three reads of tests/test_path_cpu.py
    add("tandem-repeat-gap", "ont2d", "a", tandem_repeat_gap(A, 0), [(5, ">", 0)], "mini_line_mem")
    add("bare-insertion", "ont2d", "a", bare_insertion(A, 100, np.random.default_rng(5)), [], "insertion with no reference between its flanks")
    add("dumped-edge-cluster", "default", "a", dumped_edge_cluster(A), [(15, ">", 0)], "dump_edge_cluster")
    assert [c.key for c in out] == [k for k in CASE_KEYS if big_reads or k not in BIG_KEYS]
    return out


OPS = {"==": lambda a, b: a == b, ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}


def check(stats, expect):
    """The expectations of a case that the counters of its run do not meet."""
    return [(slot, op, val, stats[slot]) for (slot, op, val) in expect if not OPS[op](stats[slot], val)]


def groups(case_list):
    """Cases by (read type, parameter overrides, reference): what one device handle can take as one batch."""
    g = {}
    for c in case_list:
        g.setdefault((c.read_type, c.over, c.ref_key), []).append(c)
    return g
