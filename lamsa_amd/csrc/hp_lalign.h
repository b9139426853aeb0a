// hp_lalign.h -- LAMSA_HP_TAG_LEFT_ALIGN: the gaps of a record's CIGAR shifted as far left as they go, in place, before res_aux counts.
//
// The definition (include/lamsa_hp.h) is a loop over the elements in ascending order: a gap (I / D) with an M on either side moves left
// one base at a time while the M before it keeps a base and the base that leaves the gap on its right equals the one that enters on its
// left (reference bases for a D, read bases for an I).  Only M lengths change.  Here the lanes do it, 64 elements per block, one per lane:
//
//   * where each element starts on the read and on the reference is a prefix sum (as in res_aux);
//   * ROOM of a movable gap = (length of the M before it) - 1; C = the prefix sum of the rooms over all elements of the record so far;
//   * a movable gap whose second neighbour to the left is not one starts a SEGMENT; Cs = C in front of the segment's first gap (a prefix
//     maximum over the segment starts: C never decreases);
//   * FREE SHIFT f of a gap: how many bases it could move if only the bases decided, counted by the lane up to C - Cs, the room there is
//     between the segment's start and the gap -- no gap of the segment can move further;
//   * the shifts obey s_i = min(f_i, room_i + s_{i-2}), s_{i-2} counting only for a movable gap: the M between the two has grown by it.
//     Unrolled that is s_i = C_i + min over the segment's gaps j <= i of (f_j - C_j), a min-plus prefix.  Because of the cap every
//     C_j - f_j of a segment is >= its Cs and every one of an earlier segment is <= it, so one prefix maximum over C - f of ALL lanes is
//     the segmented one;
//   * every M takes len += s(left neighbour) - s(right neighbour).
//
// Across blocks three running values (C, the maximum of C - f, the maximum of Cs) and the last two lanes' (movable, s) are carried in
// scalars; the block's last element is stored by the next block, which knows its right neighbour's shift.
// A record with an empty M (room -1: the recurrence would need a clamp) is walked by the definition itself; the DP routines emit none.
#pragma once
#include "hp_core.h"

namespace hp {

// the definition, element by element (wave-uniform: every lane walks the same elements): only for a record with an empty M element
HP_INL void lalign_seq(HP_G cig_t *c, int cn, const HP_G uint8_t *R, int rl, const HP_G uint8_t *T, int tl)
{
    int q = 0, p = 0;
    for (int i = 0; i < cn; ++i) {
        const int w = c[i], op = w & 0xf, k = w >> 4;
        if ((op == C_I || op == C_D) && i > 0 && i < cn - 1 && (c[i - 1] & 0xf) == C_M && (c[i + 1] & 0xf) == C_M && k >= 0) {
            const HP_G uint8_t *X = op == C_D ? T : R;
            const int xl = op == C_D ? tl : rl;
            int x = op == C_D ? p : q, room = (int)(c[i - 1] >> 4) - 1, s = 0;
            while (s < room && x >= 1 && x + k <= xl && X[x - 1] == X[x + k - 1]) { --x; ++s; }
            if (s > 0) { c[i - 1] -= s << 4; c[i + 1] += s << 4; q -= s; p -= s; wv::sync(); }
        }
        if (op == C_M || op == C_I || op == C_S) q += k;
        if (op == C_M || op == C_D) p += k;
    }
}

// Left-aligns cig[0 .. cn) (M form) in place; R = the read on the record's strand (rl bases), T = the forward reference from the record's
// offset (tl bases).  Returns the number of gaps that moved (0 on the walk by the definition): res_aux has no use for it, the emulation's
// tests (tests/emu/emu_lalign.cpp) compare it with the checker's count.  No base outside R[0 .. rl) / T[0 .. tl) is read and no word outside
// cig[0 .. cn) is written, whatever the CIGAR holds.  Every argument is a value: no address of a caller's local is handed over.
HP_NOINL int lalign_cigar(cig_t *cig_, int cn, const uint8_t *R_, int rl, const uint8_t *T_, int tl)
{
    HP_G cig_t *cig = (HP_G cig_t *)cig_;
    const HP_G uint8_t *R = (const HP_G uint8_t *)R_, *T = (const HP_G uint8_t *)T_;
    wv::sync();                                                         // the CIGAR and the window were written by other lanes
    {   // an empty (or negative) M anywhere: by the definition itself
        bool empty = false;
        for (int c0 = 0; c0 < cn && !empty; c0 += 64) {
            wv::Lane<int> z;
            WAVE_FOR(l) { const int i = c0 + l; const int w = i < cn ? (int)cig[i] : 1 << 4; z[l] = (w & 0xf) == C_M && (w >> 4) < 1; }
            empty = wv::ballot(z) != 0;
        }
        if (empty) { lalign_seq(cig, cn, R, rl, T, tl); wv::sync(); return 0; }
    }
    int q0 = 0, p0 = 0;                                                 // read / reference bases before the block
    int c_run = 0, v_run = 0, cs_run = 0;                               // C, max(C - f), max(Cs) so far
    int prev_w = C_S, prev_new = 0;                                     // the element before the block as it was, and as it is to be stored
    int mov62 = 0, mov63 = 0, s63 = 0;                                  // the last two lanes of the block before: movable gap? / the last one's shift
    int moved = 0;
    for (int c0 = 0; c0 < cn; c0 += 64) {
        wv::Lane<int> wl, pw, nw, up, rinc, finc, mov, room;
        WAVE_FOR(l) {
            const int i = c0 + l;
            const int w = i < cn ? (int)cig[i] : C_S;                   // (behind the end: an empty clip)
            const int op = w & 0xf, len = w >> 4;
            wl[l] = w;
            rinc[l] = (op == C_M || op == C_I || op == C_S) ? len : 0;
            finc[l] = (op == C_M || op == C_D) ? len : 0;
            up[l] = l < 63 ? l + 1 : 63;
        }
        pw = wl; wv::shr1(pw, prev_w);
        nw = wv::gather(wl, up);
        const int next_w = c0 + 64 < cn ? (int)cig[c0 + 64] : C_S;      // lane 63's right neighbour
        wv::Lane<int> rs = rinc, fs = finc;
        wv::scan_add_excl(rs); wv::scan_add_excl(fs);
        const int r_tot = wv::reduce_sum(rinc), f_tot = wv::reduce_sum(finc);
        WAVE_FOR(l) {
            const int op = wl[l] & 0xf, len = wl[l] >> 4, nx = l < 63 ? nw[l] : next_w;
            mov[l] = (op == C_I || op == C_D) && len >= 0 && (pw[l] & 0xf) == C_M && (nx & 0xf) == C_M;
            room[l] = mov[l] ? (pw[l] >> 4) - 1 : 0;
        }
        wv::Lane<int> Cx = room, m2 = mov, cs, v, vm, s;
        wv::scan_add_excl(Cx);
        wv::shr1(m2, mov63); wv::shr1(m2, mov62);                    // m2[l] = mov of lane l - 2
        WAVE_FOR(l) { Cx[l] += c_run; cs[l] = mov[l] && !m2[l] ? Cx[l] : 0; }
        {   wv::Lane<int> t = cs; wv::scan_max_excl(t, 0);
            WAVE_FOR(l) { const int a = t[l] > cs[l] ? t[l] : cs[l]; cs[l] = a > cs_run ? a : cs_run; } }
        // the free shifts: a lane compares base pairs one step further left each round, at most as many as its segment has room so far
        WAVE_FOR(l) {
            int n = 0;
            if (mov[l]) {
                const bool del = (wl[l] & 0xf) == C_D;
                const HP_G uint8_t *X = del ? T : R;
                const int x = del ? p0 + fs[l] : q0 + rs[l], k = wl[l] >> 4, xl = del ? tl : rl;
                int cap = Cx[l] + room[l] - cs[l];
                if (cap > x) cap = x;
                if (x + k > xl || x < 0) cap = 0;                       // (a CIGAR longer than its read or window: res_aux flags it)
                while (n < cap && X[x - 1 - n] == X[x + k - 1 - n]) ++n;
            }
            v[l] = mov[l] ? Cx[l] + room[l] - n : 0;
        }
        vm = v; wv::scan_max_excl(vm, 0);
        WAVE_FOR(l) {
            int a = vm[l] > v[l] ? vm[l] : v[l];
            a = a > v_run ? a : v_run;
            vm[l] = a;
            s[l] = mov[l] ? Cx[l] + room[l] - a : 0;
        }
        wv::Lane<int> sl = s, sr = wv::gather(s, up), g;
        wv::shr1(sl, s63);
        const int s0 = wv::bcast(s, 0);
        WAVE_FOR(l) {
            const int i = c0 + l;
            g[l] = s[l] > 0;
            if ((wl[l] & 0xf) == C_M) {
                const int d = sl[l] - (l < 63 ? sr[l] : 0);
                wl[l] += d * 16;                                        // (lane 63: its right neighbour's shift comes with the next block)
                if (d != 0 && i < cn) cig[i] = (cig_t)wl[l];
            }
            if (l == 0 && c0 > 0 && s0 > 0) cig[c0 - 1] = (cig_t)(prev_new - (s0 << 4));
        }
        moved += __builtin_popcountll(wv::ballot(g));
        prev_w = wv::bcast(nw, 62);                                     // lane 63 as it was: lane 62's right neighbour
        prev_new = wv::bcast(wl, 63);
        mov62 = wv::bcast(mov, 62); mov63 = wv::bcast(mov, 63); s63 = wv::bcast(s, 63);
        c_run = wv::bcast(Cx, 63) + wv::bcast(room, 63);
        v_run = wv::bcast(vm, 63); cs_run = wv::bcast(cs, 63);
        q0 += r_tot; p0 += f_tot;
    }
    wv::sync();
    return moved;
}

}  // namespace hp
