// hp_eqx.h -- LAMSA_HP_TAG_EQX: a record's CIGAR in =/X form, written straight into the result words (out_line, hp_out.h).
//
// Every M element is replaced by its pieces -- maximal runs of aligned bases that equal the reference ('=', op 7) or differ from it
// ('X', op 8; a read N differs, as for NM) -- and every other element is copied.  Pieces never merge across elements.  The inputs are
// the record's CIGAR (M form, left as it is: get_reg and round 2 read it afterwards) and its mismatch list (res_aux, hp_fill.h:
// ref_off << 2 | base, sorted by reference offset), so this is a merge of two sorted sequences, done by the lanes:
//
//   * the elements 64 per block, one per lane: where each starts and ends on the reference is a prefix sum;
//   * the mismatches that fall into the block 64 per pass, one per lane (the list is sorted, so they are the next ones).  A lane finds
//     its element by a binary search over the block's reference ends (lane gathers, as res_aux finds a base's element); it STARTS A RUN
//     when the mismatch before it (one-lane shift, the last lane's carried across passes) is absent, not at ref_off - 1 or in another
//     element, and ENDS one by the mirrored test.  A run start emits ['=' piece before it, if not empty]['X' piece]; the X length is
//     the distance to the first run end at or above the lane (a ballot).  A run that is still open at the end of a pass leaves its slot
//     in scalar registers and is closed by the first run end of a later pass;
//   * then every element emits itself: an M its trailing '=' piece when that is not empty (an M without mismatches is one '='),
//     any other element its own word.
//
// Output slots need no second look at anything.  A run start's first word goes to
//     (elements before its element) - (M elements before it that have no trailing piece) + (run words before it),
// and the middle term is the number of mismatches before the lane that sit on the LAST base of their element -- a prefix count of the
// pass plus a running total.  An element's own word goes to the same expression with the run words of the elements up to itself,
// which the element lanes pick up pass by pass with a second binary search (how many mismatch lanes of the pass lie in elements <= mine)
// and a gather from the inclusive scan of the run words.  All running totals are wave-uniform.
// No lane ever walks the mismatches of an element: a 5-kbp M with 250 mismatches is four passes.
#pragma once
#include "hp_fill.h"

namespace hp {

// Returns the number of words written to dst[0 .. cap), or -1 when they do not fit (nothing is written at or behind dst + cap; every store
// is checked against [0, cap), so a list that did not belong to the CIGAR could not write outside either).
// Every argument is a value: no address of a caller's local is handed over.
HP_NOINL int eqx_words(const cig_t *cig_, int cn, const int32_t *mm_, int n_mm, int32_t *dst_, int cap)
{
    const HP_G cig_t *cig = (const HP_G cig_t *)cig_;
    const HP_G int32_t *mm = (const HP_G int32_t *)mm_;
    HP_G int32_t *dst = (HP_G int32_t *)dst_;
    int kc = 0;                          // mismatches consumed
    int f0 = 0, idx0 = 0;                // reference bases / elements that emit anything, before the block
    int tl0 = 0, rw0 = 0;                // M elements without a trailing piece, and words of runs, so far
    int prev_r = -2;                     // reference offset of mismatch kc - 1
    int open_slot = -1, open_k = 0;      // the X word of a run that has not ended yet, and the run's first mismatch
    wv::sync();                          // the list and the CIGAR were written by other lanes
    for (int c0 = 0; c0 < cn; c0 += 64) {
        wv::Lane<int> wl, fs, fe, idx, pres;
        WAVE_FOR(l) {
            const int i = c0 + l;
            const int w = i < cn ? (int)cig[i] : 0;                 // (lanes behind the end: an empty M)
            const int op = w & 0xf, len = w >> 4;
            wl[l] = w;
            fe[l] = (op == C_M || op == C_D) ? len : 0;
            pres[l] = i < cn && !(op == C_M && len == 0);           // an empty M has no pieces
        }
        fs = fe; wv::scan_add_excl(fs);
        idx = pres; wv::scan_add_excl(idx);
        WAVE_FOR(l) { fs[l] += f0; fe[l] += fs[l]; idx[l] += idx0; }
        const int f1 = wv::bcast(fe, 63);                           // reference bases before the next block
        const int rwB = rw0, tlB = tl0;
        wv::Lane<int> accrw, lastr;                                 // per element: run words of the block's elements up to it; its last mismatch
        WAVE_FOR(l) { accrw[l] = 0; lastr[l] = fs[l] - 1; }
        int cnt = 0;
        do {
            wv::Lane<int> rr, val;
            WAVE_FOR(l) { const int k = kc + l; const int r = k < n_mm ? (int)(mm[k] >> 2) : 0x7fffffff; rr[l] = r; val[l] = r < f1; }
            cnt = __builtin_popcountll(wv::ballot(val));            // the list is sorted: the lanes below cnt
            if (cnt == 0) break;
            const int peek = kc + 64 < n_mm ? (int)(mm[kc + 64] >> 2) : 0x7fffffff;
            // the element of each mismatch: how many of the block's elements end at or before it
            wv::Lane<int> e;
            WAVE_FOR(l) { e[l] = 0; }
#pragma unroll
            for (int step = 32; step >= 1; step >>= 1) {
                wv::Lane<int> probe;
                WAVE_FOR(l) { probe[l] = e[l] + step - 1; }
                const wv::Lane<int> v = wv::gather(fe, probe);
                WAVE_FOR(l) { if (v[l] <= rr[l]) e[l] += step; }
            }
            const wv::Lane<int> es = wv::gather(fs, e), ee = wv::gather(fe, e), ei = wv::gather(idx, e);
            wv::Lane<int> pr = rr, nx, up;
            wv::shr1(pr, prev_r);
            WAVE_FOR(l) { up[l] = l < 63 ? l + 1 : 63; }                 // (lane 63 takes `peek` below; no index leaves 0 .. 63)
            nx = wv::gather(rr, up);
            wv::Lane<int> st, en, eq, w, t;
            WAVE_FOR(l) {
                const int r = rr[l], nxt = l < 63 ? nx[l] : peek;
                st[l] = val[l] && (pr[l] != r - 1 || r == es[l]);
                en[l] = val[l] && (nxt != r + 1 || r == ee[l] - 1);
                eq[l] = st[l] ? (pr[l] >= es[l] ? r - pr[l] - 1 : r - es[l]) : 0;
                w[l] = st[l] ? 1 + (eq[l] > 0) : 0;
                t[l] = val[l] && r == ee[l] - 1;
                if (!val[l]) e[l] = 64;
            }
            wv::Lane<int> P = w, T = t;
            wv::scan_add_excl(P); wv::scan_add_excl(T);
            const unsigned long long S = wv::ballot(st), E = wv::ballot(en);
            if (open_slot >= 0 && E != 0) {                         // the run left open ends at the first run end of this pass
                if ((unsigned)open_slot < (unsigned)cap) dst[open_slot] = (int32_t)(((kc + __builtin_ctzll(E) - open_k + 1) << 4) | C_X);
                open_slot = -1;
            }
            wv::Lane<int> xs;
            WAVE_FOR(l) {
                const int slot = ei[l] - (tl0 + T[l]) + rw0 + P[l];
                xs[l] = slot + (eq[l] > 0);
                if (st[l]) {
                    if (eq[l] > 0 && (unsigned)slot < (unsigned)cap) dst[slot] = (int32_t)((eq[l] << 4) | C_EQ);
                    const unsigned long long m = E >> l;
                    if (m != 0 && (unsigned)xs[l] < (unsigned)cap) dst[xs[l]] = (int32_t)(((__builtin_ctzll(m) + 1) << 4) | C_X);
                }
            }
            if (S != 0) {
                const int hs = 63 - __builtin_clzll(S);             // the last run start of the pass: the only one that can stay open
                if ((E >> hs) == 0) { open_slot = wv::bcast(xs, hs); open_k = kc + hs; }
            }
            // the element lanes: how many mismatches of this pass lie in the elements up to mine, and what they emitted
            wv::Lane<int> cle;
            WAVE_FOR(l) { cle[l] = 0; }
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                const int step = q < 6 ? 32 >> q : 1;               // 32 .. 1, and 1 again: the count reaches 64
                wv::Lane<int> probe;
                WAVE_FOR(l) { const int q_ = cle[l] + step - 1; probe[l] = q_ < 63 ? q_ : 63; }
                const wv::Lane<int> v = wv::gather(e, probe);
                WAVE_FOR(l) { if (cle[l] + step <= 64 && v[l] <= l) cle[l] += step; }
            }
            wv::Lane<int> clt = cle, last, Pi;
            wv::shr1(clt, 0);
            WAVE_FOR(l) { last[l] = cle[l] > 0 ? cle[l] - 1 : 0; Pi[l] = P[l] + w[l]; }      // (unused where cle is 0)
            const wv::Lane<int> gp = wv::gather(Pi, last), gr = wv::gather(rr, last);
            WAVE_FOR(l) {
                if (cle[l] > 0) accrw[l] += gp[l];
                if (cle[l] > clt[l]) lastr[l] = gr[l];
            }
            rw0 += wv::reduce_sum(w);
            tl0 += __builtin_popcountll(wv::ballot(t));
            prev_r = wv::bcast(rr, cnt - 1);
            kc += cnt;
        } while (cnt == 64);
        // the elements themselves
        wv::Lane<int> tl, word;
        WAVE_FOR(l) {
            const int op = wl[l] & 0xf, tail = fe[l] - 1 - lastr[l];
            tl[l] = pres[l] && op == C_M && tail == 0;
            word[l] = op == C_M ? (tail << 4) | C_EQ : wl[l];
        }
        wv::Lane<int> TL = tl;
        wv::scan_add_excl(TL);
        WAVE_FOR(l) {
            const int slot = idx[l] - (tlB + TL[l]) + rwB + accrw[l];
            if (pres[l] && !tl[l] && (unsigned)slot < (unsigned)cap) dst[slot] = (int32_t)word[l];
        }
        f0 = f1; idx0 += __builtin_popcountll(wv::ballot(pres));
    }
    wv::sync();
    const int total = idx0 - tl0 + rw0;
    return total <= cap ? total : -1;
}

}  // namespace hp
