// hp_seed.h -- seeding in the resident FM index (lamsa_hp_fm_seed, include/lamsa_hp.h): the seeds of a chunk of reads are cut, searched
// and located on the device and come back as the hit records of a lamsa_hp_batch.  The definition -- which seeds a read has, which rows
// become hits, in which order -- is the header's; this file is its device side.
//
// Host+device lane routines in the style of hp_fm.h, whose index routines they call unchanged; the CPU lane emulation of the tests compiles
// this file as it is.  The passes (kernels in hp_api.hip, loops in tests/emu/emu_seed.cpp):
//   seed_search_lane   one seed per lane: (read, seed index) from the flat seed number by a search in the scanned seed counts, fm_match
//                      straight on the read bytes -> lo, the rows to locate (n when 1 .. max_hits, else 0), the over-max flag
//   scan of the row counts (fm_scan_*) -> row_off
//   per slice of the flat row list (bounded device buffers, LAMSA_HP_FM_SLICE rows as in lamsa_hp_fm_search):
//       seed_locate_lane   one row per lane: fm_sa_at, then strand, contig and bounds -> a provisional record and a keep flag
//       scan of the keep flags (fm_scan_*) -> where a kept row goes among the slice's hits
//       seed_hits_lane     one row per lane: a kept row's record to its place; the first row a seed has in the slice adds the seed's
//                          kept rows of the slice to the seed's count (one lane per seed and slice, slices one after the other: no atomics)
//       the slice's hits go to the host; flat row order is seed order, then row order, so they are appended as they come
//   seed_slot_lane     one seed per lane: slot flag = kept > 0 or over-max
//   scans of the slot flags and of the kept counts (fm_scan_*)
//   seed_emit_lane     one seed per lane: seed_id and hit_off of its slot; one read boundary per lane: seed_off
// Nothing on the order-defining path is atomic: the same call gives the same words every time.
#pragma once
#include "hp_fm.h"

#define HP_SEED_MAX_HITS 16383                      // largest max_hits: HP_MAX_HITS_PER_SEED (hp_chain.h), what a seed slot of a batch may hold

namespace hp {

struct SeedArgs {                                   // everything the passes share (device pointers)
    FmIx ix;
    const uint8_t *read_seq; const int64_t *read_off;            // the caller's reads
    const int64_t *sd_off;                                       // [n_reads + 1] exclusive scan of the reads' seed counts (seed_all)
    int32_t n_reads, seed_len, seed_step, max_hits;
    int64_t n_seeds;
    const int64_t *seq_offset; const int32_t *seq_len; int32_t n_seqs; int64_t l_pac;      // the contig table; l_pac = ix.seq_len / 2
    // per seed
    uint64_t *lo; int32_t *cnt, *over, *kept, *slot;             // [n_seeds]
    const int64_t *row_off;                                      // [n_seeds + 1] exclusive scan of cnt
    const int64_t *slot_off, *kept_off;                          // [n_seeds + 1] exclusive scans of slot and kept
    // per row of the slice t0 .. t1 of the flat row list
    int64_t t0, t1;
    int64_t *p_seed, *p_pos; int32_t *p_chr; int32_t *keep;      // [t1 - t0] provisional records (p_chr: contig id, negative on the '-' strand)
    const int64_t *keep_off;                                     // [t1 - t0 + 1] exclusive scan of keep
    int64_t *s_pos; int32_t *s_chr; int8_t *s_strand;            // [kept rows of the slice] the slice's hits, in order
    // the batch
    int32_t *seed_id; int64_t *hit_off, *seed_off;               // [n_slots], [n_slots + 1], [n_reads + 1]
};

HP_FM void seed_search_lane(const SeedArgs &a, int64_t j)
{
    const HP_G int64_t *soff = (const HP_G int64_t *)a.sd_off;
    const int64_t r = fm_last_le(soff, (int64_t)a.n_reads + 1, j);          // a read without seeds shares its offset with the next one: never the last <= j
    const HP_G uint8_t *s = (const HP_G uint8_t *)a.read_seq + ((const HP_G int64_t *)a.read_off)[r] + (j - soff[r]) * a.seed_step;
    uint64_t lo, hi;
    const uint64_t n = fm_match(a.ix, a.seed_len, s, &lo, &hi);
    ((HP_G uint64_t *)a.lo)[j] = lo;
    ((HP_G int32_t *)a.cnt)[j] = n >= 1 && n <= (uint64_t)a.max_hits ? (int32_t)n : 0;
    ((HP_G int32_t *)a.over)[j] = n > (uint64_t)a.max_hits;
    ((HP_G int32_t *)a.kept)[j] = 0;
}

HP_FM void seed_locate_lane(const SeedArgs &a, int64_t t)
{
    const HP_G int64_t *roff = (const HP_G int64_t *)a.row_off;
    const int64_t j = fm_last_le(roff, a.n_seeds + 1, t);                    // seeds without rows share their offset with the next one
    const int64_t p = (int64_t)fm_sa_at(a.ix, ((const HP_G uint64_t *)a.lo)[j] + (uint64_t)(t - roff[j]));
    const bool is_rev = p >= a.l_pac;
    const int64_t f = is_rev ? 2 * a.l_pac - 1 - p : p;                       // forward coordinate of the seed's first text base
    const HP_G int64_t *coff = (const HP_G int64_t *)a.seq_offset;
    const int64_t c = fm_last_le(coff, a.n_seqs, f);                          // the contig that holds f (seq_offset[0] = 0 <= f)
    const int64_t pos = f - coff[c] + 1 - (is_rev ? a.seed_len - 1 : 0);
    const bool keep = pos >= 1 && pos + a.seed_len - 1 <= (int64_t)((const HP_G int32_t *)a.seq_len)[c];
    const int64_t k = t - a.t0;
    ((HP_G int64_t *)a.p_seed)[k] = j; ((HP_G int64_t *)a.p_pos)[k] = pos;
    ((HP_G int32_t *)a.p_chr)[k] = is_rev ? -(int32_t)(c + 1) : (int32_t)(c + 1);
    ((HP_G int32_t *)a.keep)[k] = keep;
}

HP_FM void seed_hits_lane(const SeedArgs &a, int64_t t)
{
    const HP_G int64_t *koff = (const HP_G int64_t *)a.keep_off, *roff = (const HP_G int64_t *)a.row_off;
    const int64_t k = t - a.t0, j = ((const HP_G int64_t *)a.p_seed)[k];
    if (((const HP_G int32_t *)a.keep)[k]) {
        const int64_t o = koff[k];
        const int32_t c = ((const HP_G int32_t *)a.p_chr)[k];
        ((HP_G int64_t *)a.s_pos)[o] = ((const HP_G int64_t *)a.p_pos)[k];
        ((HP_G int32_t *)a.s_chr)[o] = c < 0 ? -c : c;
        ((HP_G int8_t *)a.s_strand)[o] = c < 0 ? -1 : 1;
    }
    const int64_t first = roff[j] > a.t0 ? roff[j] : a.t0;                   // the first row seed j has in this slice
    if (t == first) {
        const int64_t end = roff[j + 1] < a.t1 ? roff[j + 1] : a.t1;
        ((HP_G int32_t *)a.kept)[j] += (int32_t)(koff[end - a.t0] - koff[k]);
    }
}

HP_FM void seed_slot_lane(const SeedArgs &a, int64_t j)
{
    ((HP_G int32_t *)a.slot)[j] = ((const HP_G int32_t *)a.kept)[j] > 0 || ((const HP_G int32_t *)a.over)[j];
}

// x < n_seeds: seed x's slot; then one lane per read boundary 0 .. n_reads
HP_FM void seed_emit_lane(const SeedArgs &a, int64_t x)
{
    const HP_G int64_t *soff = (const HP_G int64_t *)a.sd_off, *sl = (const HP_G int64_t *)a.slot_off, *ko = (const HP_G int64_t *)a.kept_off;
    if (x < a.n_seeds) {
        if (((const HP_G int32_t *)a.slot)[x]) {
            const int64_t r = fm_last_le(soff, (int64_t)a.n_reads + 1, x);
            ((HP_G int32_t *)a.seed_id)[sl[x]] = (int32_t)(x - soff[r]) + 1;
            ((HP_G int64_t *)a.hit_off)[sl[x]] = ko[x];
        }
        if (x == a.n_seeds - 1) ((HP_G int64_t *)a.hit_off)[sl[a.n_seeds]] = ko[a.n_seeds];
        return;
    }
    const int64_t r = x - a.n_seeds;
    ((HP_G int64_t *)a.seed_off)[r] = sl[soff[r]];
}

}  // namespace hp
