// hp_out.h -- the per-read result stream (its format: hp_batch.h, include/lamsa_hp.h): the writers of its words, the line buffers of the
// fill, and every capacity that sizes a buffer of result words or a slab that holds one.  An item added to the stream is added here.
#pragma once
#include "hp_fill.h"
#include "hp_eqx.h"

namespace hp {

struct OutBuf { int32_t *w; int n, cap; };
HP_INL void out_put(Ctx &cx, OutBuf &o, int32_t v) { if (o.n < o.cap) o.w[o.n++] = v; else cx.status |= ST_OVERFLOW; }

// n words from src to dst, 64 per trip, one per lane; S: int32_t words, or cig_t elements widened to words.  No fence in here: a caller
// that copies what other lanes stored, or whose copy other lanes read next, stands its own wv::sync() where it needs one.
template <class S> HP_INL void out_copy(HP_G int32_t *dst, const HP_G S *src, int n) { for (int b0 = 0; b0 < n; b0 += 64) { WAVE_FOR(l) { const int k = b0 + l; if (k < n) dst[k] = (int32_t)src[k]; } } }

// ---- a covered interval of round 1 (get_reg): PH_REG_WORDS words behind a line's records in the line arena of the phased path
enum { PH_REG_WORDS = 10 };
HP_INL void out_reg(Ctx &cx, OutBuf &o, const Regs &G, int k)
{
    out_put(cx, o, G.beg[k]); out_put(cx, o, G.end[k]);
    out_put(cx, o, G.rb[k].is_rev); out_put(cx, o, G.rb[k].chr); out_put(cx, o, (int32_t)(G.rb[k].pos & 0xffffffffll)); out_put(cx, o, (int32_t)(G.rb[k].pos >> 32));
    out_put(cx, o, G.re[k].is_rev); out_put(cx, o, G.re[k].chr); out_put(cx, o, (int32_t)(G.re[k].pos & 0xffffffffll)); out_put(cx, o, (int32_t)(G.re[k].pos >> 32));
}
HP_INL void reg_read(const int32_t *w, Regs &G, int g)          // the same words back into interval g (phase_chain2)
{
    G.beg[g] = w[0]; G.end[g] = w[1];
    G.rb[g].is_rev = w[2]; G.rb[g].chr = w[3]; G.rb[g].pos = (int64_t)(((unsigned long long)(unsigned)w[5] << 32) | (unsigned)w[4]);
    G.re[g].is_rev = w[6]; G.re[g].chr = w[7]; G.re[g].pos = (int64_t)(((unsigned long long)(unsigned)w[9] << 32) | (unsigned)w[8]);
}

// ---- a line: four words, then its records in one of four shapes (hp_batch.h)
enum { HP_SUMREC_WORDS = 15 };   // a record under LAMSA_HP_TAG_SUMMARY: the 7 header words and the 8 of Rec::sum (include/lamsa_hp.h)
HP_FN void out_line(Ctx &cx, OutBuf &o, const LineRes &la)
{
    out_put(cx, o, la.line_score); out_put(cx, o, la.tol_score); out_put(cx, o, la.tol_NM); out_put(cx, o, la.cur_res_n + 1);
    for (int j = 0; j <= la.cur_res_n; ++j) {
        const Rec &rec = la.rec[j];
        if (la.tags & LAMSA_HP_TAG_SUMMARY) {                         // the record's 15 words, one per lane, in one store; its CIGAR stays where it is
            if (o.n + HP_SUMREC_WORDS <= o.cap) {
                HP_G int32_t *dst = (HP_G int32_t *)(o.w + o.n);
                const HP_G int32_t *sum = (const HP_G int32_t *)rec.sum;      // (written by every lane in res_aux: a lane reads its own store)
                const int32_t lo = (int32_t)(rec.offset & 0xffffffffll), hi = (int32_t)(rec.offset >> 32);
                WAVE_FOR(l) {
                    int32_t v = l >= 7 && l < HP_SUMREC_WORDS ? sum[l - 7] : 0;
                    v = l == 0 ? lo : l == 1 ? hi : l == 2 ? rec.chr : l == 3 ? rec.nstrand : l == 4 ? rec.score : l == 5 ? rec.NM : l == 6 ? rec.cig.n : v;
                    if (l < HP_SUMREC_WORDS) dst[l] = v;
                }
                o.n += HP_SUMREC_WORDS;
                wv::sync();
            }
            else cx.status |= ST_OVERFLOW;
            continue;
        }
        out_put(cx, o, (int32_t)(rec.offset & 0xffffffffll)); out_put(cx, o, (int32_t)(rec.offset >> 32));
        out_put(cx, o, rec.chr); out_put(cx, o, rec.nstrand); out_put(cx, o, rec.score); out_put(cx, o, rec.NM);
        if (la.tags & LAMSA_HP_TAG_EQX) {                             // the CIGAR in =/X form (hp_eqx.h): cigar_n is known once the words are written
            const int n = o.n < o.cap ? eqx_words(rec.cig.c, rec.cig.n, rec.mm, rec.n_mm, o.w + o.n + 1, o.cap - o.n - 1) : -1;
            if (n >= 0) { o.w[o.n] = n; o.n += 1 + n; }
            else cx.status |= ST_OVERFLOW;
        }
        else {
            out_put(cx, o, rec.cig.n);
            if (o.n + rec.cig.n <= o.cap) {                           // the record's CIGAR, copied by the lanes (word by word it was 2 500 dependent trips per line: 14 % of the fill kernel)
                wv::sync();
                out_copy((HP_G int32_t *)(o.w + o.n), (const HP_G cig_t *)rec.cig.c, rec.cig.n);
                o.n += rec.cig.n;
                wv::sync();
            }
            else cx.status |= ST_OVERFLOW;
        }
        if (la.tags & LAMSA_HP_TAG_MISMATCHES) {                      // the record's mismatch list (res_aux)
            out_put(cx, o, rec.n_mm);
            if (o.n + rec.n_mm <= o.cap) {
                wv::sync();
                out_copy((HP_G int32_t *)(o.w + o.n), (const HP_G int32_t *)rec.mm, rec.n_mm);
                o.n += rec.n_mm;
                wv::sync();
            }
            else cx.status |= ST_OVERFLOW;
        }
    }
}

// ---- the items of lamsa_hp_set_result_tags
enum { HP_TAGS_LISTS = LAMSA_HP_TAG_MISMATCHES | LAMSA_HP_TAG_EQX };       // either needs the line's mismatch lists (LineRes::ev)
// the items as the fill applies them: under LAMSA_HP_TAG_SUMMARY no CIGAR is shipped and left alignment changes M lengths only -- not a word
// of a summary (include/lamsa_hp.h) -- so the shift is skipped; the item never comes with a list item (lamsa_hp_set_result_tags)
HP_HD int fill_tags(int t) { return (t & LAMSA_HP_TAG_SUMMARY) ? LAMSA_HP_TAG_SUMMARY : t & (HP_TAGS_LISTS | LAMSA_HP_TAG_LEFT_ALIGN); }
// what lamsa_hp_set_result_tags accepts: the four items, LAMSA_HP_TAG_SUMMARY with neither item of HP_TAGS_LISTS (nothing to list or split)
HP_HD bool result_tags_valid(int t) { return !(t & ~(HP_TAGS_LISTS | LAMSA_HP_TAG_LEFT_ALIGN | LAMSA_HP_TAG_SUMMARY)) && !((t & LAMSA_HP_TAG_SUMMARY) && (t & HP_TAGS_LISTS)); }

// ---- capacities: every count of result words and every slab byte that pays for them.  L: read length, scale: 1, or 8 on the second pass
// (one-kernel path only), tags: the items.  LAMSA_HP_TAG_LEFT_ALIGN adds no word and needs no list.  tests/golden/out_caps.json pins them.
// CIGAR elements of a line: cur_buf (the line being merged) holds this many, rec_buf (its records, res_split) 4 * HP_REC_MAX more for the
// clips that every cut adds.  An element per two read bases is far above what a DP emits; a line that needs more flags ST_OVERFLOW.
HP_HD int line_cig_cap(int L, int scale) { return (2 * L + 512) * scale; }
// mismatches of a line (LineRes::ev, under either item of HP_TAGS_LISTS): at most one per aligned read base, and the records of a line
// cover disjoint parts of the read; 64 spare
HP_HD int line_ev_cap(int L) { return L + 64; }
// what LAMSA_HP_TAG_MISMATCHES adds to a line's words: the lists and a count per record
HP_HD int line_ev_words(int L) { return line_ev_cap(L) + HP_REC_MAX; }
// what LAMSA_HP_TAG_EQX adds: a record has at most cigar_n + 2 n_mm words (hp_eqx.h), so two per mismatch of the line
HP_HD int line_eqx_words(int L) { return 2 * line_ev_cap(L); }
// LAMSA_HP_TAG_SUMMARY: a record is HP_SUMREC_WORDS words whatever its CIGAR holds, so a full line is this many and its four line words
HP_HD int line_sum_words() { return HP_SUMREC_WORDS * HP_REC_MAX; }
// ... and per read where the capacity has a term in L (read_out_cap, batch_out_cap: the buffers do not shrink under the item): the words per
// base pay the 8 that stand for a CIGAR wherever the read's CIGARs have 8 elements on average; these pay them for a full line of
// HP_REC_MAX records of fewer elements.  A read with more such records is short of words as any other: ST_OVERFLOW, second pass.
HP_HD int read_sum_words() { return 8 * HP_REC_MAX; }
HP_HD int line_tag_words(int L, int tags) { return ((tags & LAMSA_HP_TAG_MISMATCHES) ? line_ev_words(L) : 0) + ((tags & LAMSA_HP_TAG_EQX) ? line_eqx_words(L) : 0) + ((tags & LAMSA_HP_TAG_SUMMARY) ? line_sum_words() : 0); }
// words of one line on the phased path (phase_fill): 12 per base for the records as on the one-kernel path, its covered intervals, the items.
// Under LAMSA_HP_TAG_SUMMARY that is at least 4 + (HP_SUMREC_WORDS + PH_REG_WORDS) * HP_REC_MAX for every read length, a read of a few
// bases included (12 L alone is not).
HP_HD int line_out_cap(int L, int tags) { return 64 + 12 * L + PH_REG_WORDS * HP_REC_MAX + line_tag_words(L, tags); }
// words of a read's result stream on the one-kernel path (align_read), all its lines; the second pass sizes its arena by it.  12 per base
// flag-off; LAMSA_HP_TAG_MISMATCHES 4 per base (a base is listed once per line that aligns it) and a count per record of four full lines;
// LAMSA_HP_TAG_EQX twice the list words.
HP_HD int64_t read_out_cap(int L, int scale, int tags) { return 64 + (12LL * L + ((tags & LAMSA_HP_TAG_MISMATCHES) ? 4LL * L + 4 * HP_REC_MAX : 0) + ((tags & LAMSA_HP_TAG_EQX) ? 8LL * L + 512 : 0) + ((tags & LAMSA_HP_TAG_SUMMARY) ? read_sum_words() : 0)) * scale; }
// words of a batch's result stream (n reads, n_bases in all): what the reads publish, packed -- a third of read_out_cap per base, a read
// that finds the stream full gets LAMSA_HP_ST_OVERFLOW and the second pass.  The lists are at most one word per aligned base and a count
// per record, the =/X pieces at most two words per aligned base; LAMSA_HP_TAG_SUMMARY as in read_sum_words.
HP_HD int64_t batch_out_cap(int n, int64_t n_bases, int tags) {
    return 1024 + (int64_t)n * 256 + 4 * n_bases + ((tags & LAMSA_HP_TAG_MISMATCHES) ? (int64_t)n * 128 + 2 * n_bases : 0) + ((tags & LAMSA_HP_TAG_EQX) ? (int64_t)n * 128 + 4 * n_bases : 0) +
           ((tags & LAMSA_HP_TAG_SUMMARY) ? (int64_t)n * read_sum_words() : 0);
}

// Bytes of a wave's slab per read base for the result and CIGAR buffers; `line`: the slab of the phased fill (one line), else of the
// one-kernel path (a read, times its scale).  Sums of the buffers where they are buffers, margins where the comment says so.
HP_HD size_t slab_per_base(int tags, bool line)
{
    // flag-off, both paths: the result words (12: read_out_cap, line_out_cap), cur_buf and rec_buf (2 elements each: line_cig_cap) and the
    // reverse complement (1 byte) are 65 bytes; rounded up to 128, a margin that must cover the temporaries of one DP step of fill_line --
    // target bytes, the step's CIGAR, H / E rows: a few bytes per base of the step, never of the read
    const size_t base = sizeof(int32_t) * 12 + sizeof(cig_t) * (2 + 2) + 1 + 63;
    // either item of HP_TAGS_LISTS: LineRes::ev (1 word: line_ev_cap) and the words LAMSA_HP_TAG_MISMATCHES adds (1 a line, 4 a read: line_ev_words,
    // read_out_cap) are 8 / 20 bytes; 24 on both paths, the rest is margin
    const size_t lists = (tags & HP_TAGS_LISTS) ? sizeof(int32_t) * (1 + 4) + 4 : 0;
    // LAMSA_HP_TAG_EQX: its result words (2 a line: line_eqx_words, 8 a read: read_out_cap) are 8 / 32 bytes; 16 / 40 with a margin of 8
    const size_t eqx = (tags & LAMSA_HP_TAG_EQX) ? sizeof(int32_t) * (line ? 2 : 8) + 8 : 0;
    return base + lists + eqx;
}
// LAMSA_HP_TAG_SUMMARY costs nothing per base.  Per wave it adds the words its capacities add to the result buffers: a line's
// line_sum_words on the phased fill, read_sum_words times the scale on the one-kernel path.  (Rec::sum, 8 words in each of a LineRes's
// HP_REC_MAX records with or without the item, is 2 KiB of the slabs' constant 256 KiB, of which the fixed-size records took under 16.)
HP_HD size_t slab_fixed(int tags, int scale, bool line) { return (tags & LAMSA_HP_TAG_SUMMARY) ? sizeof(int32_t) * (size_t)(line ? line_sum_words() : read_sum_words() * scale) : 0; }
// A wave's slab on the one-kernel path (align_read), before rounding: 256 KiB for the fixed-size records (LineRes, Regs, the +512 / +64 of
// the capacities above at scale 8), the buffers above, the node arrays, sort index and line sets of H hits (~424 bytes a hit), and the
// direction matrix of the largest extension: (2 band_w + 1) columns x (L + 2 hash_step) rows, four of them on the second pass.
// Reads that need more flag LAMSA_HP_ST_OVERFLOW and are re-run by the second pass with `scale` = 8.
HP_HD size_t read_slab_bytes(int band_w, int L, int H, int scale, int tags) {
    const size_t z = (2 * (size_t)band_w + 128) * ((size_t)L + 256);
    return ((size_t)256 << 10) + slab_fixed(tags, scale, false) + (size_t)scale * slab_per_base(tags, false) * (size_t)L + 424 * (size_t)H + z * (size_t)(scale > 1 ? 4 : 1);
}
// A wave's slab on the phased fill (phase_fill, phase_filllist, phase_filldp), before rounding: the same for one line, no per-hit arrays
// (they stay with the chaining launches) and no direction matrix (the wave-per-job launch has its own slabs); dp_bytes: what the small DPs
// the fill still runs itself and a lane-DP group need.
HP_HD size_t fill_slab_bytes(int L, int tags, size_t dp_bytes) { return ((size_t)256 << 10) + slab_fixed(tags, 1, true) + slab_per_base(tags, true) * (size_t)L + dp_bytes; }

// ---- the buffers fill_line works in, from the wave's arena in this order: the line's result, the CIGAR being merged, the records' CIGARs,
// and under an item of HP_TAGS_LISTS the line's mismatch lists (res_aux).  la is nullptr when one of them did not fit (ST_OVERFLOW is set).
struct LineBufs { LineRes *la; cig_t *cur_buf, *rec_buf; int cur_cap, rec_cap; };
HP_INL LineBufs line_bufs(Ctx &cx, int L, int scale, int tags)
{
    LineBufs b;
    b.cur_cap = line_cig_cap(L, scale); b.rec_cap = b.cur_cap + 4 * HP_REC_MAX;
    b.la = (LineRes *)arena_alloc(cx, sizeof(LineRes));
    b.cur_buf = (cig_t *)arena_alloc(cx, sizeof(cig_t) * (size_t)b.cur_cap);
    b.rec_buf = (cig_t *)arena_alloc(cx, sizeof(cig_t) * (size_t)b.rec_cap);
    const bool lists = (tags & HP_TAGS_LISTS) != 0;
    const int ev_cap = lists ? line_ev_cap(L) * scale : 0;
    int32_t *ev = lists ? (int32_t *)arena_alloc(cx, sizeof(int32_t) * (size_t)ev_cap) : nullptr;
    if (!b.la || !b.cur_buf || !b.rec_buf || (lists && !ev)) { b.la = nullptr; return b; }
    b.la->ev = ev; b.la->ev_cap = ev_cap; b.la->tags = tags;
    return b;
}

}  // namespace hp
