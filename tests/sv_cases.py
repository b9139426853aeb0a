"""Hand-made reads with ONE structural-variant junction each (test infrastructure shared by tests/test_sv_cpu.py and tests/test_sv_gpu.py): reads
that run split_sv (lamsa_amd/csrc/hp_fill.h) and the k-mer split mapper split_indel_map (hp_split.h) through every branch a whole read can reach.
The builders are those of tests/crafted.py.

How a read is made.  A locus of the stand-in reference gets a WINDOW planted into it (`planted`); the read is the reference left of the window,
a hand-made GAP, and the reference right of the window.  Seeds wholly left of the gap hit on the diagonal, seeds at or right of its end hit on the
diagonal shifted by len(window) - len(gap), seeds in between have no slot (`sv_read`).  Chaining makes one line of two fragments, and the junction
between them is split_mapping's (src/frag_check.c:416-564):
    s_qlen = did * seed_step - seed_len = len(gap),   dis = len(window) - len(gap),   s_tlen = len(window)
    dis >  match_dis                 DEL: split_indel_map(gap, window, ref_offset 0); ksw_bi_extend when len(gap) < hash_len
    dis < -match_dis, s_tlen <  2 * hash_step   overlapped INS: two ksw_extend from either side and sw_mid_fix
                      s_tlen >= 2 * hash_step   DUP: the window with hash_len - dis fetched bases on either side, ref_offset = -dis, or 0 when
                                                the contig's end shortened the fetch
So a (gap, window) pair of the window-level tests (tests/test_dp_cpu.py: _split_cases) becomes a whole read, and `window_of` restates which
window split_sv hands to the mapper.  len(gap) has to be did * seed_step - seed_len: 50, 150, ... under "default" (seed_step 100), 0, 25, 50, ...
under "ont2d" (seed_step 25); other lengths take a seed_step override (Case.over).

Path counters of the CPU build (slots listed in lamsa_amd/csrc/hp_core.h):
  split_sv          28 calls; 64 DEL by ksw_bi_extend, 65 DEL by the mapper, 66 overlapped INS, 67 DUP with ref_offset = -dis, 68 DUP with ref_offset 0,
                    69 DUP by ksw_bi_extend (s_tlen < hash_len)
  split_indel_map   30 calls; 70 a window with a unique k-mer (the MIN route), 71 nodes promoted by hash_min_extend, 72 hmini_main_line calls, 13 the
                    MULTI re-update, 73 no anchor; 11 / 12 the F_INSERT sub-classes with b_i < a_i; 90 / 91 hnode_dis on an insertion of split_len / 2
                    bases or more with ref_offset > 0 / == 0
  the anchor walk   left blank 74 ksw_global, 75 ksw_bi_extend, 76 indel_cigar; right blank 77 / 78 / 79 likewise; between anchors 80 ksw_global,
                    81 ksw_bi_extend, 82 overlap on the reference (S and H elements), 83 pure indel; 84 indels of split_pen bases or more (res |= 2);
                    no anchor 85 ksw_global, 86 ksw_bi_extend
  largest values    87 n_codes, 88 matches of a k-mer that was kept; 89 counts the k-mers dropped for more than 50 matches

Branches NO whole read reaches (their counters are asserted to stay 0 over the hand-made reads and the fuzz):
  * 69, the `s_tlen < hash_len` test inside the DUP branch: the branch is entered with s_tlen >= 2 * hash_step, and hash_len / hash_step are set by the
    preset alone (10 / 10 and 8 / 4; the host program has no option for them), so 2 * hash_step >= hash_len always;
  * 11 and 12, the F_INSERT sub-classes with b_i < a_i: every caller of hnode_dis (hnode_init_from, hdp_update) passes a node of an EARLIER slot as a,
    and read_i rises with the slot (head -hash_len, slot s (s - 1) * hash_step, tail read_len), so a_i < b_i in every call.  The two sub-classes with
    b_i > a_i are reached (counters 90 / 91)."""
import numpy as np

import crafted
import reflib
from crafted import Case, concat, crafted_batch, ref_bases, sim_ref   # noqa: F401

SV, MAP = 28, 30
DEL_BI, DEL_MAP, INS_OVL, DUP_OFF, DUP_CUT, DUP_BI = 64, 65, 66, 67, 68, 69
MIN_ROUTE, PROMOTED, MINI, MULTI, NO_ANCHOR, INS_BACK_OFF, INS_BACK_0, LONG_INS_OFF, LONG_INS_0 = 70, 71, 72, 13, 73, 11, 12, 90, 91
L_GLOBAL, L_BI, L_INDEL, R_GLOBAL, R_BI, R_INDEL, B_GLOBAL, B_BI, B_OVERLAP, B_INDEL, BIG_INDEL, NONE_GLOBAL, NONE_BI = 74, 75, 76, 77, 78, 79, 80, 81, 82, 83, 84, 85, 86
MAX_CODES, MAX_KEPT, DROPPED = 87, 88, 89
UNREACHABLE = (DUP_BI, INS_BACK_OFF, INS_BACK_0)
SEED_LEN = 50
LOCUS_GAP = 20000                  # loci of one reference are this far apart: further than a read's cluster reach
_refs = {}


# ---------------------------------------------------------------- references with planted loci
class PlantedRef:
    """A copy of a stand-in reference that loci are written into; the layout of the contigs is its own."""
    def __init__(self, ref, seq_off=None, seq_len=None):
        self.pac = np.array(ref.pac, dtype=np.uint8, copy=True)
        self.l_pac = int(ref.l_pac)
        self.seq_off = np.array(ref.seq_off if seq_off is None else seq_off, np.int64)
        self.seq_len = np.array(ref.seq_len if seq_len is None else seq_len, np.int32)

    def plant(self, at, bases):
        """Write `bases` at the 0-based offset `at` of the packed reference (_set_pac, src/bntseq.c:241)."""
        bases = np.asarray(bases, np.uint8)
        assert bases.size == 0 or (int(bases.max()) <= 3 and 0 <= at and at + len(bases) <= self.l_pac)
        for i, b in enumerate(bases.tolist()):
            k = at + i
            sh = (~k & 3) << 1
            self.pac[k >> 2] = (int(self.pac[k >> 2]) & ~(3 << sh) & 0xff) | (b << sh)
        return self


def planted(ref, at, bases):
    """A copy of `ref` (a crafted.sim_ref) with `bases` written into its .pac at `at`; l_pac, seq_off and seq_len are the same."""
    return PlantedRef(ref).plant(at, bases)


def planted_two_contigs(ref, at, bases, cut):
    """The same, with the one contig cut in two at `cut`: contig 1 ends there and a short second contig carries the rest."""
    assert len(ref.seq_len) == 1 and 0 < cut < ref.l_pac
    return PlantedRef(ref, [0, cut], [cut, ref.l_pac - cut]).plant(at, bases)


# ---------------------------------------------------------------- one read, one junction
def sv_read(ref, p0, read, left_end, right_start, shift, step, strand=1):
    """One read (forward bases `read`, as they lie along the reference from 0-based p0 of contig 1) whose seeds hit as follows: seeds wholly left of
    read offset left_end on the diagonal, seeds starting at or after right_start on the diagonal shifted by `shift`, seeds in between have no
    slot.  strand -1: the batch holds the reverse complement, its seeds counted from the other end (their forward offsets start at last_len)."""
    read = np.asarray(read, np.uint8)
    L = len(read)
    seed_all = (L - SEED_LEN) // step + 1
    base = 0 if strand == 1 else L - SEED_LEN - (seed_all - 1) * step

    def hits(s, t):
        o = base + ((s - 1) if strand == 1 else (seed_all - s)) * step          # forward read offset of seed s
        if o + SEED_LEN <= left_end:
            return [(p0 + o + 1, 0, 0)]
        if o >= right_start:
            return [(p0 + o + shift + 1, 0, 0)]
        return []
    B = crafted_batch(ref, p0, L, hits, step=step)
    B.read_seq[:L] = read if strand == 1 else np.where(read > 3, 4, 3 - np.minimum(read, 3)).astype(np.uint8)[::-1]
    B.h_strand[:] = strand
    return B


def locus_read(R, p0, step, gap, window, strand=1, flank=1000, right_seeds=None, extra=7):
    """Plant `window` into R behind a left flank of about `flank` bases at p0 and make the read left flank + gap + right flank.  len(gap) must be
    did * step - SEED_LEN; `extra` bases that no seed covers end the read ('+') or begin its forward form ('-': last_len).  The batch carries `sv`:
    the forward read, the junction's read interval [qa, qb), dis, the window's 0-based start on the contig and its length."""
    gap, window = np.asarray(gap, np.uint8), np.asarray(window, np.uint8)
    did, rem = divmod(len(gap) + SEED_LEN, step)
    assert rem == 0 and did >= 1, "a gap of %d bases is no whole number of seed steps of %d" % (len(gap), step)
    j1 = max((flank - SEED_LEN) // step, 1)
    nr = right_seeds if right_seeds is not None else j1 + 1
    base = 0 if strand == 1 else extra
    qa = base + j1 * step + SEED_LEN
    qb = qa + len(gap)
    L = (j1 + did + nr - 1) * step + SEED_LEN + extra
    R.plant(p0 + qa, window)
    read = np.concatenate([ref_bases(R, p0, qa), gap, ref_bases(R, p0 + qa + len(window), L - qb)])
    B = sv_read(R, p0, read, qa, qb, len(window) - len(gap), step, strand)
    B.sv = dict(read=read, qa=qa, qb=qb, dis=len(window) - len(gap), win0=p0 + qa, s_tlen=len(window), contig_end=int(R.seq_len[0]))
    B.pac, B.l_pac, B.seq_off, B.seq_len = R.pac, R.l_pac, R.seq_off, R.seq_len
    return B


def window_of(B, P):
    """split_sv's window geometry restated (hp_fill.h, src/frag_check.c:475-545) for a DEL or DUP read made by locus_read: (gap bases, fetched
    bases, window start in them, window length, ref_offset) as split_indel_map gets them, or None when the junction does not reach the mapper."""
    sv = B.sv
    gap = sv["read"][sv["qa"]:sv["qb"]]
    dis, s_tlen, hl = sv["dis"], sv["s_tlen"], P.hash_len
    md = P.match_dis * ((sv["qb"] - sv["qa"] + SEED_LEN) // P.seed_step if (P.aln_mode & 2) else 1)
    R = PlantedRef.__new__(PlantedRef); R.pac = B.pac
    if dis > md:
        n = min(s_tlen, sv["contig_end"] - sv["win0"])
        return (gap, ref_bases(R, sv["win0"], n), 0, n, 0) if len(gap) >= hl else None
    if dis < -md and s_tlen >= 2 * P.hash_step:
        start0, want = sv["win0"] + dis - hl, s_tlen + 2 * (hl - dis)
        n = min(want, sv["contig_end"] - start0)
        return (gap, ref_bases(R, start0, n), hl - dis, s_tlen, -dis if n == want else 0) if s_tlen >= hl else None
    return None


def kmer_matches(gap, window, P):
    """Per read k-mer of the mapper (slot s at gap offset (s - 1) * hash_step): the window positions it matches, N hashed as G."""
    g = np.where(np.asarray(gap) > 3, 2, gap).astype(np.int64); w = np.where(np.asarray(window) > 3, 2, window).astype(np.int64)
    hl, hs = P.hash_len, P.hash_step
    code = lambda a, i: int(sum(int(a[i + k]) << (2 * (hl - 1 - k)) for k in range(hl)))
    wc = [code(w, i) for i in range(max(len(w) - hl + 1, 0))]
    return [[i for i, c in enumerate(wc) if c == code(g, o)] for o in range(0, len(g) - hl + 1, hs)]


# ---------------------------------------------------------------- the hand-made cases
def _uniq(rng, n):
    return rng.integers(0, 4, n, dtype=np.uint8)


def _subs(seq, at):
    s = np.array(seq, np.uint8, copy=True)
    for i in at:
        s[i] = (s[i] + 1) & 3
    return s


def _pad(parts, n):
    """The parts as one gap, which must come to exactly n bases."""
    g = np.concatenate([np.asarray(p, np.uint8) for p in parts])
    assert len(g) == n, (len(g), n)
    return g


def ref_of(key):
    if key not in _refs:
        cases()
    return _refs[key]


_cases = None


def cases():
    """The hand-made reads as crafted.Case objects, in the order of CASE_KEYS; made once.  All reads of a preset without a seed_step override lie
    on one planted reference ("sv"), loci LOCUS_GAP apart, the contig-end read last, next to the cut of the two contigs."""
    global _cases
    if _cases is not None:
        return _cases
    base = sim_ref("b")
    n_loci = 200
    cut = 200000 + n_loci * LOCUS_GAP                        # contig 1 ends here: the contig-end read is built against it
    R = planted_two_contigs(base, 0, [], cut)
    _refs["sv"] = R
    rng = np.random.default_rng(20)
    out, locus = [], [0]

    def p0_next():
        locus[0] += 1
        assert locus[0] < n_loci - 2
        return 200000 + locus[0] * LOCUS_GAP

    def add(key, rt, gap, window, expect, aim, step=None, strand=1, checks=(), **kw):
        P = reflib.lo_para(rt) if step is None else reflib.lo_para(rt, seed_step=step)
        B = locus_read(R, kw.pop("p0", None) or p0_next(), P.seed_step, gap, window, strand, **kw)
        c = Case(key, rt, "sv", B, [(SV, "==", 1)] + list(expect), aim, () if step is None else (("seed_step", step),))
        c.checks = tuple(checks)
        out.append(c)

    for rt in ("default", "ont2d"):
        P = reflib.lo_para(rt)
        hl, hs, st = P.hash_len, P.hash_step, P.seed_step
        t = rt + "-"
        g1 = 150 if rt == "default" else 100                 # a gap the k-mers tile exactly: (g1 - hash_len) % hash_step == 0
        assert (g1 - hl) % hs == 0 and (g1 + SEED_LEN) % st == 0
        mapped = [(MAP, "==", 1)]
        # ---- a. the branches of split_sv
        for q in (hl - 1, hl, hl + 1):
            w = _uniq(rng, q + 40)
            gap = np.concatenate([w[:q // 2], w[len(w) - (q - q // 2):]])
            add(t + "del-q%+d" % (q - hl), rt, gap, w, [(DEL_BI, "==", 1), (MAP, "==", 0)] if q < hl else [(DEL_MAP, "==", 1)] + mapped,
                "DEL, s_qlen %d = hash_len %+d" % (q, q - hl), step=SEED_LEN + q)
        w = _uniq(rng, 950 + 300)
        add(t + "del-long", rt, np.concatenate([w[:480], w[780:]]), w, [(DEL_MAP, "==", 1), (MIN_ROUTE, "==", 1)] + mapped, "DEL of 300 bases, a query of 950")
        for s_tlen in (0, 1, 2 * hs - 1):
            w = _uniq(rng, s_tlen)
            add(t + "ins-ovl-%d" % s_tlen, rt, np.concatenate([_uniq(rng, g1 - s_tlen), w]), w, [(INS_OVL, "==", 1), (MAP, "==", 0)], "overlapped INS, s_tlen %d" % s_tlen)
        w = _uniq(rng, 2 * hs)
        add(t + "dup-2step", rt, np.concatenate([w, _uniq(rng, g1 - 2 * hs)]), w, [(DUP_OFF, "==", 1)] + mapped, "DUP at s_tlen = 2 * hash_step = %d" % (2 * hs))
        # a tandem duplication: the read repeats the 250 / 200 bases in front of window offset 60, so the copy reaches into the left margin
        w = _uniq(rng, 100)
        g2 = g1 + 2 * st * (1 if rt == "default" else 4)     # 350 / 300: the window and a copy of 250 / 200 bases
        p0 = p0_next()
        qa = ((1000 - SEED_LEN) // st) * st + SEED_LEN
        left = ref_bases(R, p0 + qa - 400, 400)
        dup = np.concatenate([left, w[:60]])[-(g2 - 100):]
        add(t + "dup-tandem", rt, np.concatenate([w[:60], dup, w[60:]]), w, [(DUP_OFF, "==", 1), (LONG_INS_OFF, ">", 0), (B_OVERLAP, ">", 0)] + mapped,
            "tandem DUP of %d bases, ref_offset = -dis" % (g2 - 100), p0=p0)
        # ---- b. hnode_dis and the hash DP
        a = g1 // 2 // hs * hs
        w = _uniq(rng, g1 + 100)
        w[a + 40:a + 40 + hl] = w[2 * hs:2 * hs + hl]         # the k-mer of slot 3 once more, inside the deleted stretch: two matches
        add(t + "promote", rt, np.concatenate([w[:a], w[a + 100:]]), w, [(MIN_ROUTE, "==", 1), (PROMOTED, ">", 0), (B_INDEL, ">", 0), (BIG_INDEL, ">", 0)] + mapped,
            "a k-mer with two matches, one on the diagonal of a unique one: hash_min_extend promotes it; the deletion at a k-mer boundary is a pure indel of split_pen bases or more")
        # two unique flanks around a block that the window holds twice: the copies' k-mers are MULTI nodes between two MIN anchors
        blk = _uniq(rng, 6 * hs)
        fl, fr = _uniq(rng, 4 * hs), _uniq(rng, g1 - 10 * hs)
        w = np.concatenate([fl, _uniq(rng, 23), blk, _uniq(rng, 37), blk, _uniq(rng, 41), fr])
        add(t + "mini", rt, _pad([fl, blk, fr], g1), w, [(MIN_ROUTE, "==", 1), (MINI, ">", 0)] + mapped,
            "MULTI nodes of a two-copy block between two MIN anchors: hmini_main_line")
        blk = _uniq(rng, g1)
        w = np.concatenate([blk, _uniq(rng, 33), blk, _uniq(rng, 45), blk])
        add(t + "multi-3copy", rt, blk, w, [(MIN_ROUTE, "==", 0), (MULTI, ">", 0)] + mapped, "the gap is a block the window holds three times: no unique k-mer, the MULTI route")
        w = np.concatenate([blk, _uniq(rng, 61), blk])
        add(t + "multi-2copy", rt, _subs(blk, [g1 // 2]), w, [(MIN_ROUTE, "==", 0), (MULTI, ">", 0)] + mapped, "two copies, the read's copy mutated: the MULTI route")
        unit = np.array([0, 1, 3, 2, 1], np.uint8)
        add(t + "multi-tandem", rt, np.tile(unit, 60)[:g1], np.tile(unit, 80)[:g1 + 55], [(MIN_ROUTE, "==", 0), (MULTI, ">", 0)] + mapped, "a deletion inside a tandem repeat")
        add(t + "none-global", rt, _uniq(rng, 50), _uniq(rng, 95), [(NO_ANCHOR, "==", 1), (NONE_GLOBAL, "==", 1)] + mapped, "a stretch unrelated to the window, both below split_len")
        add(t + "none-bi", rt, _uniq(rng, g1), _uniq(rng, g1 + 80), [(NO_ANCHOR, "==", 1), (NONE_BI, "==", 1)] + mapped, "a stretch unrelated to the window, split_len and more")
        # ---- c. the anchor walk
        w = _uniq(rng, g1 + 120)
        plain = np.concatenate([w[:a], w[a + 120:]])
        add(t + "ends-indel", rt, plain, w, [(L_INDEL, "==", 1), (R_INDEL, "==", 1), (B_INDEL, "==", 1), (BIG_INDEL, "==", 1)] + mapped,
            "first anchor at read offset 0, last one at the read's end, a pure indel between")
        k = 2 * hs
        add(t + "ends-global", rt, _subs(plain, list(range(1, k, hs // 2)) + list(range(g1 - k, g1, hs // 2))), w, [(L_GLOBAL, "==", 1), (R_GLOBAL, "==", 1)] + mapped,
            "left and right blank of %d bases without a matching k-mer: ksw_global" % k)
        w = _uniq(rng, 350 + 130)
        long_ = np.concatenate([w[:170], w[300:]])
        add(t + "ends-bi", rt, _subs(long_, list(range(1, 110, hs // 2)) + list(range(350 - 110, 350, hs // 2))), w, [(L_BI, "==", 1), (R_BI, "==", 1)] + mapped,
            "left and right blank of 110 bases without a matching k-mer: ksw_bi_extend")
        w = _uniq(rng, g1 + 60)
        add(t + "left-window0", rt, np.concatenate([_uniq(rng, 60), w[:g1 - 60 - 3 * hs], w[len(w) - 3 * hs:]]), w, [(L_INDEL, "==", 1)] + mapped,
            "first anchor at window offset 0 behind 60 read bases of its own")
        mid = g1 // 2 // hs * hs
        w = _uniq(rng, g1 + 60)
        add(t + "right-window-end", rt, np.concatenate([w[:3 * hs], w[len(w) - (g1 - 60 - 3 * hs):], _uniq(rng, 60)]), w, [(R_INDEL, "==", 1)] + mapped,
            "last anchor at the window's end in front of 60 read bases of its own")
        w = _uniq(rng, g1 + 40)
        add(t + "between-global", rt, _subs(np.concatenate([w[:mid], w[mid + 40:]]), range(mid - 2 * hs + 1, mid + 2 * hs, hs // 2)), w,
            [(B_GLOBAL, ">", 0)] + mapped, "a deletion of 40 bases inside 4 * hash_step bases without a matching k-mer: ksw_global between anchors")
        w = _uniq(rng, g1 + 200)
        add(t + "between-bi", rt, _subs(np.concatenate([w[:mid], w[mid + 200:]]), range(mid - 2 * hs + 1, mid + 2 * hs, hs // 2)), w,
            [(B_BI, ">", 0)] + mapped, "a deletion of 200 bases inside 4 * hash_step bases without a matching k-mer: ksw_bi_extend between anchors")
        # ---- d. the edges of the lane code
        for nc in (63, 64, 65, 128, 129) if rt == "default" else (63, 64, 65, 66, 128, 129):
            wl = nc + hl - 1
            q = (50 if rt == "default" else 25) if nc < 100 else (50 if rt == "default" else 100)
            w = _uniq(rng, wl)
            h = q // 2 // hs * hs
            gap = np.concatenate([w[:h], w[wl - (q - h):]])
            last = (q - hl) // hs * hs                       # offset of the last read k-mer; it lies in the right part and matches at last + wl - q
            add(t + "codes-%d" % nc, rt, gap, w, [(MAX_CODES, "==", nc), (DEL_MAP, "==", 1)] + mapped, "n_codes %d; the last read k-mer matches window position %d only" % (nc, last + wl - q),
                checks=[("only", last // hs, last + wl - q)])
        for n_rep in (50, 51):
            rep = np.tile(np.array([2, 0, 3], np.uint8), 60)[:3 * 49 + hl]                     # the k-mer of its first hash_len bases 50 times, three bases apart
            m = (hl + hs - 1) // hs * hs                     # the k-mer and what fills its last slot
            w = np.concatenate([_uniq(rng, 4 * hs), rep, _uniq(rng, 130 + g1 - 4 * hs - m)])
            w[4 * hs - 1] = 1; w[4 * hs + len(rep)] = 1                                          # the run ends where the repeat ends
            if n_rep == 51:                                  # the 51st match two blocks of 64 further on: a count that stops at 50 keeps the k-mer
                w[4 * hs + len(rep) + 100:4 * hs + len(rep) + 100 + hl] = rep[:hl]
            gap = np.concatenate([w[:4 * hs], rep[:m], w[len(w) - (g1 - 4 * hs - m):]])
            add(t + "kmer-%d" % n_rep, rt, gap, w, [(MAX_KEPT, "==", 50), (DROPPED, "==", 0)] if n_rep == 50 else [(DROPPED, "==", 1), (MAX_KEPT, "<", 50)],
                "a k-mer with %d matches over several blocks of 64 window positions, more blocks behind them: %s" % (n_rep, "kept" if n_rep == 50 else "dropped"), checks=[("count", 4, n_rep)])
        # an N next to the breakpoint, where the window has G.  Right behind the left part the window holds a decoy of the gap's right part with A
        # there: hashed as G, the N's k-mers match their own place only, and the unique node puts the right part's other k-mers on its diagonal
        w = _uniq(rng, g1)
        w[a + hl // 2] = 2
        decoy = w[a:].copy(); decoy[hl // 2] = 0
        gap = w.copy(); gap[a + hl // 2] = 4
        add(t + "read-n", rt, gap, np.concatenate([w[:a], decoy, _uniq(rng, 40), w[a:]]), [(DEL_MAP, "==", 1), (MIN_ROUTE, "==", 1)] + mapped,
            "an N in the gap where the window has G: its k-mer matches there and nowhere else", checks=[("only", a // hs, a + (g1 - a) + 40)])
        # ---- e. the '-' strand
        w = _uniq(rng, g1 + 120)
        add(t + "minus-del", rt, np.concatenate([w[:a], w[a + 120:]]), w, [(DEL_MAP, "==", 1)] + mapped, "'-' strand: DEL", strand=-1)
        w = _uniq(rng, 100)
        p0 = p0_next()
        left = ref_bases(R, p0 + 7 + qa - 400, 400)
        dup = np.concatenate([left, w[:60]])[-(g2 - 100):]
        add(t + "minus-dup", rt, np.concatenate([w[:60], dup, w[60:]]), w, [(DUP_OFF, "==", 1)] + mapped, "'-' strand: tandem DUP", strand=-1, p0=p0)
        w = _uniq(rng, 1)
        add(t + "minus-ins-ovl", rt, np.concatenate([_uniq(rng, g1 - 1), w]), w, [(INS_OVL, "==", 1), (MAP, "==", 0)], "'-' strand: overlapped INS", strand=-1)
        blk = _uniq(rng, g1)
        add(t + "minus-multi", rt, blk, np.concatenate([blk, _uniq(rng, 33), blk, _uniq(rng, 45), blk]), [(MIN_ROUTE, "==", 0), (MULTI, ">", 0)] + mapped, "'-' strand: the MULTI route", strand=-1)
    # the DUP whose right margin of hash_len - dis bases runs over the contig's end: ref_fetch shortens the window, ref_offset is 0
    w = _uniq(rng, 40)
    for rt in ("default", "ont2d"):
        P = reflib.lo_para(rt)
        g1 = 250 if rt == "default" else 200
        nr = 2 if rt == "default" else 5
        j1 = (1000 - SEED_LEN) // P.seed_step
        did = (g1 + SEED_LEN) // P.seed_step
        L = (j1 + did + nr - 1) * P.seed_step + SEED_LEN + 7
        qb = j1 * P.seed_step + SEED_LEN + g1
        assert L - qb == 157                                 # both presets: the same right flank, so the same window in front of the one contig end
        p0 = cut - (L - qb) - 40 - (qb - g1)                 # the read's last base is the contig's last
        add(rt + "-dup-contig-end", rt, np.concatenate([w[:20], _uniq(rng, g1 - 40), w[20:]]), w, [(DUP_CUT, "==", 1), (MAP, "==", 1)],
            "DUP next to the contig's end: the fetch is shortened, ref_offset 0", p0=p0, right_seeds=nr)
    _cases = out
    return _cases


CASE_KEYS = [rt + "-" + k for rt in ("default", "ont2d") for k in
             ["del-q-1", "del-q+0", "del-q+1", "del-long", "ins-ovl-0", "ins-ovl-1", "ins-ovl-%d" % (19 if rt == "default" else 7), "dup-2step", "dup-tandem", "promote", "mini",
              "multi-3copy", "multi-2copy", "multi-tandem", "none-global", "none-bi", "ends-indel", "ends-global", "ends-bi", "left-window0", "right-window-end", "between-global",
              "between-bi"] + ["codes-%d" % n for n in ((63, 64, 65, 128, 129) if rt == "default" else (63, 64, 65, 66, 128, 129))] +
             ["kmer-50", "kmer-51", "read-n", "minus-del", "minus-dup", "minus-ins-ovl", "minus-multi"]] + ["default-dup-contig-end", "ont2d-dup-contig-end"]


# ---------------------------------------------------------------- fuzz: the five window kinds of tests/test_dp_cpu.py as whole reads
def _mut(rng, s, p):
    """Substitutions, insertions and deletions at rate p each."""
    out = []
    for c in np.asarray(s).tolist():
        x = rng.random()
        if x < p:
            out.append((c + 1 + int(rng.integers(0, 3))) % 4)
        elif x < 2 * p:
            out += [c, int(rng.integers(0, 4))]
        elif x >= 3 * p:
            out.append(c)
    return np.array(out, np.uint8)


def _fit(rng, gap, window, n):
    """The pair with a gap of exactly n bases: surplus bases leave both ends, missing ones are appended to both (dis stays what it was)."""
    k = len(gap) - n
    if k > 0:
        return gap[:n], window[:max(len(window) - k, 0)]
    tail = _uniq(rng, -k)
    return np.concatenate([gap, tail]), np.concatenate([window, tail])


def fuzz(preset, n, seed):
    """n reads of one junction each as ONE batch over a planted reference of its own (returned with it; loci LOCUS_GAP apart): deletions, gaps all
    over a tandem repeat, duplications whose margins are the reference around the window, deleted stretches between two copies of a block, and
    microsatellites on both flanks; 1 % substitutions, insertions and deletions each in the gap, none in the seeds that carry hits."""
    P = reflib.lo_para(preset)
    st, hs = P.seed_step, P.hash_step
    R = PlantedRef(sim_ref("b"))
    assert 200000 + (n + 1) * LOCUS_GAP < R.l_pac
    rng = np.random.default_rng(seed)
    md = lambda q: P.match_dis * ((q + SEED_LEN) // st if (P.aln_mode & 2) else 1)
    qlens = [q for q in range(st - SEED_LEN if st > SEED_LEN else st, 1000, st)]       # what s_qlen can be under this preset
    pick = lambda lo, hi: int(rng.choice([q for q in qlens if lo <= q <= hi]))
    qa = ((1000 - SEED_LEN) // st) * st + SEED_LEN
    batches = []
    for it in range(n):
        p0 = 200000 + it * LOCUS_GAP
        kind = it % 5
        if kind == 0:                                        # deletion
            q = pick(50, 950); D = int(rng.integers(md(q) + 5, 900))
            w = _uniq(rng, q + D); a = int(rng.integers(10, q - 9))
            gap, w = _fit(rng, _mut(rng, np.concatenate([w[:a], w[a + D:]]), 0.01), w, q)
        elif kind == 1:                                      # a tandem repeat all over
            q = pick(50, 450); unit = _uniq(rng, int(rng.integers(2, 7)))
            gap, w = np.tile(unit, 400)[:q], np.tile(unit, 400)[:q + int(rng.integers(md(q) + 5, 200))]
        elif kind == 2:                                      # duplication: the window is the reference's own sequence
            q = pick(100, 950); dup = int(rng.integers(max(15, md(q) + 5), q - 2 * hs - 1)); s_tlen = q - dup
            a = int(rng.integers(0, s_tlen)); k = min(dup, s_tlen - a)
            w = ref_bases(R, p0 + qa, s_tlen)
            gap, w = _fit(rng, _mut(rng, np.concatenate([w[:a + k], ref_bases(R, p0 + qa + a + k - dup, dup), w[a + k:]]), 0.01), w, q)
        elif kind == 3:                                      # two copies of a block around the deleted stretch
            q = pick(150, 350); blk = _uniq(rng, 60)
            w = np.concatenate([_uniq(rng, q // 2 - 20), blk, _uniq(rng, int(rng.integers(50, 400))), blk, _uniq(rng, q - q // 2 - 20)])
            gap, w = _fit(rng, _mut(rng, np.concatenate([w[:q // 2], w[len(w) - (q - q // 2):]]), 0.01), w, q)
        else:                                                # microsatellites on both flanks
            q = pick(150, 250); unit = _uniq(rng, 3)
            w = np.concatenate([np.tile(unit, 40), _uniq(rng, int(rng.integers(30, 300))), np.tile(unit, 40)])
            gap, w = _fit(rng, _mut(rng, np.concatenate([np.tile(unit, 30), np.tile(unit, 30)]), 0.01), w, q)
        batches.append(locus_read(R, p0, st, gap, w))
    return R, batches


OPS = dict(crafted.OPS)
OPS["<"] = lambda a, b: a < b


def check(stats, expect):
    return [(slot, op, val, stats[slot]) for (slot, op, val) in expect if not OPS[op](stats[slot], val)]
