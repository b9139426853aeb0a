// hp_fm.h -- the FM index of the reference's <ref>.bwt / <ref>.sa resident in HBM: batched exact search (lamsa_hp_fm_search, include/lamsa_hp.h).
//
// Layout, as bwt_restore_bwt / bwt_restore_sa leave it (src/bwt.c:421-462) and lamsa_amd/host/rescue.cpp reads it: the text is the forward
// reference followed by its reverse complement, seq_len symbols; row 0 is the sentinel suffix, row r >= 1 the r-th smallest suffix; `primary`
// is the row of suffix 0, whose BWT symbol (the sentinel) is not stored, so row k > primary lies at stored position k - 1.  The BWT words come
// in blocks of 16: four 64-bit counts (symbols 0..3 in front of the block), then 128 two-bit symbols, the first in the top bits of the first
// word.  A block is 64 bytes and 64-byte aligned: one occurrence count is one block read.  sa[j] is the text position of row j * sa_intv
// (sa[0], row 0, is (uint64_t)-1 as bwt_restore_sa sets it); other rows walk LF steps to a sampled one (bwt_sa, :86).
//
// The index routines are host+device (HP_FM): the CPU lane emulation of the tests compiles this file as it is.  Two kernels use them
// (hp_api.hip): k_fm_search, one k-mer per lane, and k_fm_locate, one suffix-array row per lane.  Both are chains of dependent random
// 64-byte reads and nothing else: no LDS, few registers, as many resident lanes as the SIMDs hold.
#pragma once
#include <hp/wave.h>
#include <stdint.h>

// host+device like HP_HD, and inlined: a routine that is called hands its caller's block (16 registers) over through scratch
#ifdef __HIPCC__
#define HP_FM __host__ __device__ __forceinline__
#else
#define HP_FM static inline
#endif

namespace hp {

struct FmIx {                                   // the resident index (device pointers)
    uint64_t seq_len, primary, L2[5];
    const uint32_t *bwt;                        // padded: a whole block may be read at every block start
    const uint64_t *sa; uint64_t sa_intv;       // sa_intv is a power of two
};

#define HP_FM_TILE 1024                         // counts per wave of the scan (16 per lane)
#define HP_FM_MAX_OCC (1 << 20)                 // largest max_occ: a tile's sum stays below 2^31

HP_FM uint64_t fm_L2(const FmIx &ix, int c)
{   // L2[c], c = 0..4, without a runtime-indexed copy of the kernel argument
    return c == 0 ? ix.L2[0] : c == 1 ? ix.L2[1] : c == 2 ? ix.L2[2] : c == 3 ? ix.L2[3] : ix.L2[4];
}

// A block by value, every word a member of its own: nothing indexes it at run time, so it lives in registers (an int[16] picked
// from by the symbol came out as an array in scratch, read back through a computed address).
struct FmBlock { int c0l, c0h, c1l, c1h, c2l, c2h, c3l, c3h, s0, s1, s2, s3, s4, s5, s6, s7; };

// one of four / eight values by number.  The values come in by value: written as a conditional expression over members of the block, the
// compiler folds the member reads into one read at a computed address and the block is in scratch again.
HP_FM int fm_sel4(int i, int a, int b, int c, int d) { return i == 0 ? a : i == 1 ? b : i == 2 ? c : d; }
HP_FM int fm_sel8(int i, int a, int b, int c, int d, int e, int f, int g, int h) { return (i & 4) ? fm_sel4(i & 3, e, f, g, h) : fm_sel4(i & 3, a, b, c, d); }

// the block that holds stored position k: four 16-byte loads
HP_FM FmBlock fm_load_block(const FmIx &ix, uint64_t k)
{
    const HP_G uint32_t *p = (const HP_G uint32_t *)ix.bwt + ((k >> 7) << 4);
    int a[4], b[4], c[4], d[4];
    hp_load16(p, a); hp_load16(p + 4, b); hp_load16(p + 8, c); hp_load16(p + 12, d);
    FmBlock w;
    w.c0l = a[0]; w.c0h = a[1]; w.c1l = a[2]; w.c1h = a[3]; w.c2l = b[0]; w.c2h = b[1]; w.c3l = b[2]; w.c3h = b[3];
    w.s0 = c[0]; w.s1 = c[1]; w.s2 = c[2]; w.s3 = c[3]; w.s4 = d[0]; w.s5 = d[1]; w.s6 = d[2]; w.s7 = d[3];
    return w;
}

// symbols equal to c among the first n (0 .. 32) symbols of the 32 in (hi, lo), the first in the top bits: the word's equality bits (one
// per symbol, bwt_occ's __occ_aux) masked down to the symbols that count
HP_FM uint64_t fm_word_occ(int hi, int lo, uint64_t xh, uint64_t xl, int n)
{
    const uint64_t y = (uint64_t)(uint32_t)hi << 32 | (uint32_t)lo;
    const uint64_t eq = ((y ^ xh) >> 1) & (y ^ xl) & 0x5555555555555555ull;
    const int m = n < 0 ? 0 : (n > 32 ? 32 : n);
    const uint64_t mask = m ? ~0ull << (64 - 2 * m) : 0;
    return (uint64_t)__builtin_popcountll(eq & mask);
}

// symbols equal to c among the first n (0 .. 128) symbols of a block, plus the block's count for c.  Branch-free over the four symbol
// words.  Because the equality bits are masked, not the symbols, there is nothing to correct for c == 0 afterwards (bwt_occ masks the
// symbols, which then read as 0, and subtracts them again, :124).
HP_FM uint64_t fm_block_occ(const FmBlock &w, int c, int n)
{
    const uint32_t lo = (uint32_t)fm_sel4(c, w.c0l, w.c1l, w.c2l, w.c3l), hi = (uint32_t)fm_sel4(c, w.c0h, w.c1h, w.c2h, w.c3h);
    const uint64_t xh = (c & 2) ? 0 : ~0ull, xl = (c & 1) ? 0 : ~0ull;
    return ((uint64_t)hi << 32 | lo) + fm_word_occ(w.s0, w.s1, xh, xl, n) + fm_word_occ(w.s2, w.s3, xh, xl, n - 32) + fm_word_occ(w.s4, w.s5, xh, xl, n - 64) + fm_word_occ(w.s6, w.s7, xh, xl, n - 96);
}

// bwt_occ (:107): symbols equal to c in rows 0 .. k; k == -1 and k == seq_len as the reference answers them
HP_FM uint64_t fm_occ(const FmIx &ix, uint64_t k, int c)
{
    if (k == ix.seq_len) return fm_L2(ix, c + 1) - fm_L2(ix, c);
    if (k == (uint64_t)-1) return 0;
    k -= (k >= ix.primary);                                       // the sentinel is not stored
    const FmBlock w = fm_load_block(ix, k);
    return fm_block_occ(w, c, (int)(k & 127) + 1);
}

// bwt_2occ (:132): fm_occ(k, c) and fm_occ(l, c) for k <= l, from one block read when both fall into the same block
HP_FM void fm_occ2(const FmIx &ix, uint64_t k, uint64_t l, int c, uint64_t *ok, uint64_t *ol)
{
    const uint64_t kk = k - (k >= ix.primary), ll = l - (l >= ix.primary);
    if ((ll >> 7) != (kk >> 7) || k == (uint64_t)-1 || l == (uint64_t)-1 || l == ix.seq_len || k == ix.seq_len) { *ok = fm_occ(ix, k, c); *ol = fm_occ(ix, l, c); return; }
    const FmBlock w = fm_load_block(ix, kk);
    *ok = fm_block_occ(w, c, (int)(kk & 127) + 1);
    *ol = fm_block_occ(w, c, (int)(ll & 127) + 1);
}

// bwt_match_exact_alt (:241) from the whole index (0, seq_len): the rows lo .. hi whose suffixes start with s[0 .. len); returns their
// number, 0 (and lo = 1, hi = 0) when there is none or a base code is above 3
HP_FM uint64_t fm_match(const FmIx &ix, int len, const HP_G uint8_t *s, uint64_t *lo, uint64_t *hi)
{
    uint64_t k = 0, l = ix.seq_len;
    *lo = 1; *hi = 0;
    for (int i = len - 1; i >= 0; --i) {
        const int c = s[i];
        if (c > 3) return 0;
        uint64_t ok, ol;
        fm_occ2(ix, k - 1, l, c, &ok, &ol);
        k = fm_L2(ix, c) + ok + 1; l = fm_L2(ix, c) + ol;
        if (k > l) return 0;
    }
    *lo = k; *hi = l;
    return l - k + 1;
}

// bwt_sa (:86): the text position of a row; LF steps (bwt_invPsi, :53) until the row is a sampled one.  The row's symbol and its count lie
// in the same block: one read per step.  (For k == seq_len bwt_occ answers L2[c + 1] - L2[c] without a read; the block gives the same number.)
HP_FM uint64_t fm_sa_at(const FmIx &ix, uint64_t k)
{
    uint64_t s = 0;
    const uint64_t mask = ix.sa_intv - 1;
    while (k & mask) {
        ++s;
        if (k == ix.primary) { k = 0; continue; }
        const uint64_t x = k - (k > ix.primary);
        const FmBlock w = fm_load_block(ix, x);
        const int r = (int)(x & 127), word = fm_sel8(r >> 4, w.s0, w.s1, w.s2, w.s3, w.s4, w.s5, w.s6, w.s7);
        const int c = (int)((uint32_t)word >> ((~r & 15) << 1)) & 3;
        k = fm_L2(ix, c) + fm_block_occ(w, c, r + 1);
    }
    return s + ((const HP_G uint64_t *)ix.sa)[k / ix.sa_intv];
}

// ------------------------------------------------------------------ the lanes of the two kernels
struct FmSearchArgs {
    FmIx ix;
    const uint8_t *seq; const int64_t *win_off, *kmer_off;      // window w: seq[win_off[w] .. win_off[w + 1]), k-mers kmer_off[w] .. kmer_off[w + 1]
    int32_t n_win, k, max_occ; int64_t n_kmers;
    uint64_t *lo, *hi;                            // [n_kmers] inclusive row interval, (1, 0) when empty
    int32_t *cnt;                                 // [n_kmers] rows to locate: the interval's size when it is 1 .. max_occ, else 0
};

// the last i in [0, n) with a[i] <= x; a is ascending (equal neighbours allowed), a[0] <= x
HP_FM int64_t fm_last_le(const HP_G int64_t *a, int64_t n, int64_t x)
{
    int64_t lo = 0, hi = n;                       // a[lo] <= x < a[hi] (a[n] = infinity)
    while (hi - lo > 1) { const int64_t mid = lo + ((hi - lo) >> 1); if (a[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

HP_FM void fm_search_lane(const FmSearchArgs &a, int64_t j)
{
    const HP_G int64_t *koff = (const HP_G int64_t *)a.kmer_off;
    const int64_t w = fm_last_le(koff, (int64_t)a.n_win + 1, j);            // an empty window shares its offset with the next one: never the last <= j
    const HP_G uint8_t *s = (const HP_G uint8_t *)a.seq + ((const HP_G int64_t *)a.win_off)[w] + (j - koff[w]);
    uint64_t lo, hi;
    const uint64_t n = fm_match(a.ix, a.k, s, &lo, &hi);
    ((HP_G uint64_t *)a.lo)[j] = lo; ((HP_G uint64_t *)a.hi)[j] = hi;
    ((HP_G int32_t *)a.cnt)[j] = n >= 1 && n <= (uint64_t)a.max_occ ? (int32_t)n : 0;
}

struct FmLocateArgs {
    FmIx ix;
    const uint64_t *lo; const int64_t *pos_off; int64_t n_kmers;             // pos_off: [n_kmers + 1], the exclusive scan of cnt
    int64_t t0, t1;                               // this slice: flat positions t0 .. t1
    uint64_t *pos;                                // [t1 - t0]
};

HP_FM void fm_locate_lane(const FmLocateArgs &a, int64_t t)
{
    const HP_G int64_t *poff = (const HP_G int64_t *)a.pos_off;
    const int64_t j = fm_last_le(poff, a.n_kmers + 1, t);                  // k-mers without positions share their offset with the next one
    ((HP_G uint64_t *)a.pos)[t - a.t0] = fm_sa_at(a.ix, ((const HP_G uint64_t *)a.lo)[j] + (uint64_t)(t - poff[j]));
}

// ------------------------------------------------------------------ exclusive scan of cnt -> pos_off, one wave per tile of HP_FM_TILE counts
// three passes: tile sums; the scan of the tile sums by one wave; the offsets of a tile's counts from its start.  Wave-uniform code.
struct FmScanArgs { const int32_t *cnt; int64_t n; int64_t n_tiles; int32_t *tile_sum; int64_t *tile_off /* [n_tiles + 1] */; int64_t *pos_off /* [n + 1] */; };

HP_INL void fm_scan_sums(const FmScanArgs &a, int64_t tile)
{
    wv::Lane<int> s;
    WAVE_FOR(l) {
        const int64_t b = tile * HP_FM_TILE + (int64_t)l * 16;
        int acc = 0;
        for (int i = 0; i < 16; ++i) acc += b + i < a.n ? a.cnt[b + i] : 0;
        s[l] = acc;
    }
    const int tot = wv::reduce_sum(s);
    if (wv::leader()) a.tile_sum[tile] = tot;
}

HP_INL void fm_scan_tiles(const FmScanArgs &a)
{   // sums of up to 2^31 - 1 each: scanned as two 16-bit halves so that 64 of them stay inside an int
    int64_t run = 0;
    for (int64_t base = 0; base < a.n_tiles; base += 64) {
        wv::Lane<int> lo, hi, lo_e, hi_e;
        WAVE_FOR(l) { const int v = base + l < a.n_tiles ? a.tile_sum[base + l] : 0; lo[l] = v & 0xffff; hi[l] = v >> 16; lo_e[l] = lo[l]; hi_e[l] = hi[l]; }
        wv::scan_add_excl(lo_e); wv::scan_add_excl(hi_e);
        const int tl = wv::reduce_sum(lo), th = wv::reduce_sum(hi);
        WAVE_FOR(l) if (base + l < a.n_tiles) a.tile_off[base + l] = run + lo_e[l] + ((int64_t)hi_e[l] << 16);
        run += tl + ((int64_t)th << 16);
    }
    if (wv::leader()) a.tile_off[a.n_tiles] = run;
}

HP_INL void fm_scan_write(const FmScanArgs &a, int64_t tile)
{
    wv::Lane<int> s;
    WAVE_FOR(l) {
        const int64_t b = tile * HP_FM_TILE + (int64_t)l * 16;
        int acc = 0;
        for (int i = 0; i < 16; ++i) acc += b + i < a.n ? a.cnt[b + i] : 0;
        s[l] = acc;
    }
    wv::scan_add_excl(s);
    WAVE_FOR(l) {
        const int64_t b = tile * HP_FM_TILE + (int64_t)l * 16;
        int64_t run = a.tile_off[tile] + s[l];
        for (int i = 0; i < 16 && b + i < a.n; ++i) {
            a.pos_off[b + i] = run;
            run += a.cnt[b + i];
            if (b + i == a.n - 1) a.pos_off[a.n] = run;
        }
    }
}

}  // namespace hp
