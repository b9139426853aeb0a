// hp_core.h -- per-wave context, bump arena, bounded CIGAR vectors, sequence views.
// Device code (compiled by hipcc for gfx950; the tests also compile it with the CPU
// lane emulation of tests/emu/hp/wave.h).  Wave-uniform unless a comment says otherwise.
#pragma once
#include <hp/wave.h>
#include "../../include/lamsa_hp.h"

namespace hp {

typedef int32_t cig_t;                       // len<<4|op, signed like the reference (src/lamsa_aln.h:210)
enum { C_M = 0, C_I = 1, C_D = 2, C_N = 3, C_S = 4, C_H = 5, C_EQ = 7, C_X = 8 };      // numbered as in SAM; '=' and 'X' only in the result stream (LAMSA_HP_TAG_EQX, hp_eqx.h)
enum { ST_OVERFLOW = LAMSA_HP_ST_OVERFLOW, ST_REFEXIT = LAMSA_HP_ST_REFEXIT, ST_UNSUPPORTED = LAMSA_HP_ST_UNSUPPORTED,
       ST_DEAD = ST_OVERFLOW | ST_REFEXIT | ST_UNSUPPORTED };     // ST_DEAD: the read has no result

#define HP_NEG_INF (-0x40000000)             // MINUS_INF, src/ksw.c:504

// Bump allocator over a slab of HBM owned by this wave.  Stack discipline via mark/release.
struct Arena {
    char *base; size_t cap, top;
};
HP_INL void arena_init(Arena &a, void *base, size_t cap) { a.base = (char *)base; a.cap = cap; a.top = 0; }
HP_INL size_t arena_mark(const Arena &a) { return a.top; }
HP_INL void arena_release(Arena &a, size_t m) { a.top = m; }

// LDS of one wave (= one workgroup): circular H and E rows, staged query bases, direction matrix (see hp_ksw.h).
// Sized for the fill kernel's 8 waves per SIMD = 32 workgroups per CU (the hardware's limit): 32 x 5 KB of the CU's 160 KB.  The fill
// kernel is bound by the latency each wave exposes, and every step up in occupancy paid even though it costs VGPRs (64 at 8 waves) and
// LDS for the direction matrix (measured, ms per step of 65 536 reads: 4 waves / 5 KB matrix 326, 5 / 3.5 KB 322, 6 / 2.1 KB 307,
// 7 / 1.2 KB 295, 8 / 0.5 KB 294 -- profiles/r02_variants_occupancy*.txt).  Bands up to w = 222 use the
// LDS rows (the presets use 10..200); wider ones fall back to rows in HBM.
#ifndef HP_LDS_CELLS
#define HP_LDS_CELLS 512
#endif
#ifndef HP_LDS_Z_BYTES
#define HP_LDS_Z_BYTES 512
#endif
#define HP_LDS_WORDS (2 * HP_LDS_CELLS + HP_LDS_CELLS / 4 + HP_LDS_Z_BYTES / 4)
#ifndef HP_CHAIN_LDS_WORDS
#define HP_CHAIN_LDS_WORDS 2432             // LDS words of a wave of the chaining kernels (>= HP_SORT_BLOCK * 2 for the hit sort; 16 waves per CU)
#endif
// LDS words of a wave that runs BOTH halves (the one-kernel form of the retry pass, the CPU emulation): enough for either
#define HP_BOTH_LDS_WORDS (HP_CHAIN_LDS_WORDS > HP_LDS_WORDS ? HP_CHAIN_LDS_WORDS : HP_LDS_WORDS)
// the lane strips of hp_cluster.h / hp_gaps.h (six words per entry and lane) are cut from the chaining kernels' LDS
#define HP_LANE_STRIP_WORDS HP_CHAIN_LDS_WORDS

struct Ctx {
    const lamsa_hp_para *P;   // parameters (kernel argument copy)
    HP_L int32_t *lds;        // the LDS owned by this wave: at least HP_LDS_WORDS words (the DP rows of hp_ksw.h need those)
    int lds_words;            // its size (the chaining kernels give a wave more: a cluster's node state lives there, hp_cluster.h)
    Arena tmp;                // scratch slab of this wave
    int status;               // ST_* bits for the unit (read / job) being processed
    long long n_cells;        // DP cells updated (accounting: GCUPS)
    long long *prof;          // per-read cycle counters of diagnostic builds (-DHP_PROF), else nullptr
    long long *prof_dp = nullptr;   // -DHP_PROF, wave-per-job launch only: per-routine cycle / cell counters of ksw_extend (else nullptr)
    int lds_epoch;            // bumped by every DP routine that writes the rows' part of the LDS (hp_ksw.h): what a caller parked there (frags_merge's staged CIGARs) is gone
};
// -DHP_PROF_FILL: slots 16 .. 23 time parts of frags_merge (hp_fill.h) instead of parts of the chaining (hp_chain.h, hp_gaps.h)
#if defined(HP_PROF_EDGE) && (defined(HP_PROF_TRACK) || defined(HP_PROF_FILL))
#error "-DHP_PROF_EDGE, -DHP_PROF_TRACK and -DHP_PROF_FILL all use prof slots 16 .. 23: one of them per build"
#endif
#ifdef HP_PROF_FILL
#define HP_PROF_CHAIN_ON 0
#define HP_TADD_FILL(cx, slot, v) HP_TADD(cx, slot, v)
#else
#define HP_PROF_CHAIN_ON 1
#define HP_TADD_FILL(cx, slot, v) do { } while (0)
#endif
#ifdef HP_PROF
#define HP_T0(v) const long long v = wv::clock()
#define HP_TADD(cx, slot, v) do { if ((cx).prof) { (cx).prof[slot] += wv::clock() - (v); (cx).prof[(slot) + 1] += 1; } } while (0)
#else
#define HP_T0(v) do { } while (0)
#define HP_TADD(cx, slot, v) do { } while (0)
#endif

// path counters of the tests' CPU build (tests/emu/emu_api.cpp defines HP_STAT, HP_STAT_ADD and HP_STAT_MAX): which variant of a routine a test
// has really run (HP_STAT, HP_STAT_ADD: counts), and how large the thing was that took it (HP_STAT_MAX: the largest value seen).  Slots:
//  0 lines by cluster, 1 lines by seed range, 2 gaps in lanes, 3 of them from START, 4 gaps through the wave-wide routine, 5 of them through memory (hp_gaps.h),
//  6-8 lines in clusters of <= 6 / <= 16 / more hits, 9 wave jobs published (hp_phase.h), 10 an uncovered region at the read's end (hp_align.h),
//  11-13 the F_INSERT classes and the MULTI re-update of the k-mer split mapper, 30 its calls (hp_split.h), 14 inter-lines, 15 dumped edge clusters (hp_chain.h),
//  16-19, 22, 31 the DP routines of hp_ksw.h, 20-21 head / tail extensions taken from a wave job, 24-29 fragment merging (hp_fill.h), 23 wave jobs on a big slab (emulation),
//  32 clusters chained out of LDS (dp_cluster_lds), 33 clusters sent through HBM, 34 clusters handled one per lane (cluster_lane), 35 / 36 line sets staged in LDS / left in
//  HBM (lset_stage), 37 / 38 sorts in one LDS block / in several (hp_sort.h), 39 gaps of the scan by seed range handed to a lane (gap_lane);
//  largest values: 40 cluster chained out of LDS, 41 cluster sent through HBM, 42 hits listed for a wave-wide gap, 43 survivors of a gap a lane took,
//  44 lines handed to lset_stage, 45 / 46 gaps of a line scanned by seed range / by cluster, 47 cluster handled by a lane, 48 clusters of a read;
//  branch tracking with the largest cluster in LDS (hp_track.h): 49 reads with a resident cluster, 50 tracks on the image, 51 tracks through HBM while
//  an image is resident, 52 walk steps on the image, 53 cut_branch on the image with two or more sons, 54 / 55 negative edges detached on the image in
//  the walk / in cut_branch, 56 end nodes on the image whose chain of more than 64 nodes is marked by the chase through `from`,
//  58 / 59 get_max_son on the image: a son that ties the best on max_score at another seed distance / at the same one (max_NM decides), 60 a son skipped for its edge
//  class once a match-class son is held, 61 largest clusters refused by the packing checks, 62 cut_branch on the image with three or more sons, 63 reads with a resident cluster whose first pass
//  takes every hit (all_min); largest value: 57 resident cluster;
//  SV junctions (tests/sv_cases.py), through HP_STATX_ADD / HP_STATX_MAX (below) only: split_sv (hp_fill.h) 64 DEL through ksw_bi_extend, 65 DEL through the split mapper, 66 overlapped
//  INS, 67 / 68 DUP through the mapper with ref_offset = -dis / 0 (window cut at the contig's end), 69 DUP through ksw_bi_extend; the split mapper (hp_split.h) 70 windows
//  with a unique k-mer (MIN route), 71 nodes promoted by hash_min_extend, 72 hmini_main_line calls, 73 windows without an anchor; its anchor walk: 74 / 75 / 76 the left blank
//  by ksw_global / ksw_bi_extend / indel_cigar, 77 / 78 / 79 the right blank likewise, 80 / 81 between anchors by ksw_global / ksw_bi_extend, 82 overlap on the reference,
//  83 pure indel, 84 indels of split_pen bases or more, 85 / 86 no anchor: ksw_global / ksw_bi_extend; 89 read k-mers dropped for more than HP_HASH_MAX_HITS matches,
//  90 / 91 hnode_dis on an insertion of split_len / 2 bases or more with ref_offset > 0 / == 0; largest values: 87 n_codes, 88 matches of a k-mer that was kept
//  re-bases of the sliding window of ksw_extend_band (hp_ksw.h; tests/rebase_jobs.py), through HP_STATX_ADD / HP_STATX_MAX only: 92 re-bases, 95 / 96 those in the first / last row
//  of a 64-row target block; largest values: 93 lanes freed by one re-base, 94 64 minus the lanes freed by one (so: 64 minus the fewest)
//  the lane-per-job DP in two stages (hp_lanedp.h, phase_filldp of hp_phase.h; tests/lanedp_jobs.py), through HP_STATX_ADD only: 97 / 98 ksw_bi_extend / ksw_global2 jobs a first-stage
//  or one-stage group ran, 99 .. 104 ksw_bi_extend jobs by exit (LJ_X_*: finished after the left extension, global after left, finished after the right extension, global after
//  right, sw_mid_fix S-H, sw_mid_fix global), 105 jobs the first stage put into a hard queue, 106 jobs the second stage ran, 107 hard jobs left to the fill because their queue was full
#ifndef HP_DPLOG
#define HP_DPLOG(kind, qlen, tlen, w, cells) do { } while (0)      // tests' CPU build: one record per DP call (tools/dp_shapes.py)
#endif
#ifndef HP_STAT
#define HP_STAT(i) do { } while (0)
#endif
// (HP_STAT keeps the expansion it has always had: an empty loop and an empty expression are not the same to the compiler's block layout, and
// the device code must not depend on whether a counter is there.  The two forms with a value are empty expressions.)
#ifndef HP_STAT_ADD
#define HP_STAT_ADD(i, n) ((void)0)
#endif
#ifndef HP_STAT_MAX
#define HP_STAT_MAX(i, v) ((void)0)
#endif
// Slots from 64 on (the SV junctions) go through HP_STATX_ADD / HP_STATX_MAX: they count only in a CPU build that says how many slots its array has
// (HP_STAT_SLOTS, tests/emu/emu_api.cpp).  A CPU build whose array ends at slot 63 and the device build see an empty expression, so no slot is
// ever written behind an array that was not made for it.
#ifdef HP_STAT_SLOTS
static_assert(HP_STAT_SLOTS >= 108, "the array of the path counters ends before the last slot the device sources use");
#define HP_STATX_ADD(i, n) HP_STAT_ADD(i, n)
#define HP_STATX_MAX(i, v) HP_STAT_MAX(i, v)
#else
#define HP_STATX_ADD(i, n) ((void)0)
#define HP_STATX_MAX(i, v) ((void)0)
#endif

// returns nullptr (and flags overflow) when the slab is exhausted; callers must cope
HP_INL void *arena_alloc(Ctx &cx, size_t bytes) {
    size_t b = (bytes + 15) & ~(size_t)15;
    if (cx.tmp.top + b > cx.tmp.cap) { cx.status |= ST_OVERFLOW; return nullptr; }
    void *p = cx.tmp.base + cx.tmp.top;
    cx.tmp.top += b;
    return p;
}

// bounded CIGAR vector (storage elsewhere)
struct CigV { cig_t *c; int n, cap; };
HP_INL void cig_bind(CigV &v, cig_t *mem, int cap) { v.c = mem; v.n = 0; v.cap = mem ? cap : 0; }
HP_INL bool cig_alloc(Ctx &cx, CigV &v, int cap) {
    cig_t *m = (cig_t *)arena_alloc(cx, (size_t)cap * sizeof(cig_t));
    cig_bind(v, m, cap);
    return m != nullptr;
}
HP_INL void cig_raw_push(Ctx &cx, CigV &v, cig_t w) {
    if (v.n >= v.cap) { cx.status |= ST_OVERFLOW; return; }
    v.c[v.n++] = w;
}
// _push_cigar0, src/frag_check.h:136-151
HP_INL void cig_push0(Ctx &cx, CigV &v, cig_t w) {
    if (v.n > 0 && (v.c[v.n - 1] & 0xf) == (w & 0xf)) { v.c[v.n - 1] += (w >> 4) << 4; return; }
    cig_raw_push(cx, v, w);
}
// _push_cigar1, src/frag_check.h:153-156
HP_INL void cig_push1(Ctx &cx, CigV &v, cig_t w) { if ((w >> 4) == 0) return; cig_push0(cx, v, w); }
// _push_cigar, src/frag_check.h:158-184 (first word merges; I+S and S+I fuse into S).  The body is copied by the
// lanes (one coalesced pass); source and destination never overlap.
HP_FN void cig_pushv(Ctx &cx, CigV &v, const cig_t *c, int n) {
    if (n == 0) return;
    const HP_G cig_t *src = (const HP_G cig_t *)c;
    HP_G cig_t *dst = (HP_G cig_t *)v.c;
    const int vn = v.n;
    int j = 0;
    if (vn > 0) {
        const cig_t last = dst[vn - 1], c0 = src[0];
        if ((last & 0xf) == (c0 & 0xf)) { dst[vn - 1] = last + ((c0 >> 4) << 4); j = 1; }
        else if (((last & 0xf) == C_I && (c0 & 0xf) == C_S) || ((last & 0xf) == C_S && (c0 & 0xf) == C_I)) {
            dst[vn - 1] = (((last >> 4) + (c0 >> 4)) << 4) | C_S; j = 1;
        }
    }
    const int m = n - j;
    if (vn + m > v.cap) { cx.status |= ST_OVERFLOW; return; }
    for (int b0 = 0; b0 < m; b0 += 64) { WAVE_FOR(l) { const int i = b0 + l; if (i < m) dst[vn + i] = src[j + i]; } }
    v.n = vn + m;
    wv::sync();
}
// _push_cigar with a one-word source held in a register
HP_FN void cig_pushw(Ctx &cx, CigV &v, cig_t w) {
    if (v.n > 0) {
        const cig_t last = v.c[v.n - 1];
        if ((last & 0xf) == (w & 0xf)) { v.c[v.n - 1] = last + ((w >> 4) << 4); return; }
        if (((last & 0xf) == C_I && (w & 0xf) == C_S) || ((last & 0xf) == C_S && (w & 0xf) == C_I)) { v.c[v.n - 1] = (((last >> 4) + (w >> 4)) << 4) | C_S; return; }
    }
    if (v.n + 1 > v.cap) { cx.status |= ST_OVERFLOW; return; }
    v.c[v.n++] = w;
}
// _invert_cigar, src/frag_check.h:124
HP_FN void cig_invert(cig_t *c, int n) {
    HP_G cig_t *g = (HP_G cig_t *)c;
    for (int b0 = 0; b0 < n / 2; b0 += 64) {
        WAVE_FOR(l) { const int a = b0 + l; if (a < n / 2) { const cig_t x = g[a], y = g[n - 1 - a]; g[a] = y; g[n - 1 - a] = x; } }
    }
    wv::sync();
}
// readInCigar (M,I,S) / refInCigar (M,D,H), src/frag_check.c:179,205
HP_FN int cig_readlen(const cig_t *c, int n) {
    const HP_G cig_t *g = (const HP_G cig_t *)c;
    int tot = 0;
    for (int b0 = 0; b0 < n; b0 += 64) {
        wv::Lane<int> x;
        WAVE_FOR(l) { const int i = b0 + l; int v = 0; if (i < n) { const cig_t w = g[i]; const int op = w & 0xf; if (op == C_M || op == C_I || op == C_S) v = w >> 4; } x[l] = v; }
        tot += wv::reduce_sum(x);
    }
    return tot;
}
HP_FN int cig_reflen(const cig_t *c, int n) {
    const HP_G cig_t *g = (const HP_G cig_t *)c;
    int tot = 0;
    for (int b0 = 0; b0 < n; b0 += 64) {
        wv::Lane<int> x;
        WAVE_FOR(l) { const int i = b0 + l; int v = 0; if (i < n) { const cig_t w = g[i]; const int op = w & 0xf; if (op == C_M || op == C_D || op == C_H) v = w >> 4; } x[l] = v; }
        tot += wv::reduce_sum(x);
    }
    return tot;
}

// strided view of a base sequence (stride -1 = reversed), 1 byte/base codes 0..4
struct Seq { const uint8_t *p; int stride; };
HP_INL int seq_at(const Seq &s, int i) { return s.p[(long)i * s.stride]; }
HP_INL Seq seq_fwd(const uint8_t *p) { Seq s; s.p = p; s.stride = 1; return s; }
HP_INL Seq seq_rev(const uint8_t *p, int len) { Seq s; s.p = p + (len > 0 ? len - 1 : 0); s.stride = -1; return s; }

// substitution score: lamsa_fill_mat, src/lamsa_aln.c:1331-1340 (N row/column = -1)
HP_INL int sub_score(const lamsa_hp_para *P, int t, int q) { return (t > 3 || q > 3) ? -1 : (t == q ? P->match : -P->mis); }

HP_INL int iabs(int x) { return x < 0 ? -x : x; }
HP_INL int imin(int a, int b) { return a < b ? a : b; }
HP_INL int imax(int a, int b) { return a > b ? a : b; }

}  // namespace hp
