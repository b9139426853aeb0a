// emu_fm.cpp -- TEST INFRASTRUCTURE: lamsa_hp_fm_load / lamsa_hp_fm_search of include/lamsa_hp.h on the CPU lane emulation: the index
// routines, the lanes of the two kernels and the scan between them are lamsa_amd/csrc/hp_fm.h as the device compiles it; only the
// launches are loops here.  Linked into tests/_build/lamsa_emu_fm (the host program with --rescue-gpu, no GPU), into the planner check
// (tests/host/fm_plan_check.cpp) and, alone, into a shared library that tests/test_fm_cpu.py calls.  A handle is only a key here (the
// emulated handle of emu_capi.cpp knows nothing of an index), so any non-null pointer serves as one.
#include <map>
#include <string>
#include <vector>
#include <stdlib.h>
#include "../../include/lamsa_hp.h"
#include "hp_fm.h"

using namespace hp;

namespace {
struct EmuFm {
    lamsa_hp_fm_index ix; std::vector<uint32_t> bwt; std::vector<uint64_t> sa;
    std::vector<int64_t> kmer_off, pos_off; std::vector<uint64_t> lo, hi, pos;
};
std::map<const void *, EmuFm> g_fm;
long long g_slices = 0;
}

extern "C" long long emu_fm_last_slices() { return g_slices; }      // locate slices of the last search

extern "C" int lamsa_hp_fm_load(lamsa_hp_handle *h, const lamsa_hp_fm_index *ix)
{
    if (!h) return LAMSA_HP_EINVAL;
    g_fm.erase(h);
    if (!ix || !ix->bwt || !ix->sa) return LAMSA_HP_EINVAL;
    bool ok = ix->seq_len > 0 && ix->primary >= 1 && ix->primary <= ix->seq_len && ix->L2[0] == 0 && ix->L2[4] == ix->seq_len && ix->sa_intv > 0 && (ix->sa_intv & (ix->sa_intv - 1)) == 0;
    for (int c = 0; ok && c < 4; ++c) ok = ix->L2[c] <= ix->L2[c + 1];
    ok = ok && ix->bwt_words >= ((ix->seq_len + 15) >> 4) + ((ix->seq_len + 127) >> 7) * 8 && ix->n_sa == (ix->seq_len + ix->sa_intv) / ix->sa_intv;
    if (!ok) return LAMSA_HP_EINVAL;
    EmuFm &f = g_fm[h];
    f.ix = *ix;
    f.bwt.assign(ix->bwt, ix->bwt + ix->bwt_words); f.bwt.resize(f.bwt.size() + 16, 0);      // as the device copy: a whole block behind the last word
    f.sa.assign(ix->sa, ix->sa + ix->n_sa);
    return LAMSA_HP_OK;
}

extern "C" int lamsa_hp_fm_search(lamsa_hp_handle *h, const lamsa_hp_fm_queries *q, lamsa_hp_fm_out *out)
{
    if (!h || !q || !out) return LAMSA_HP_EINVAL;
    auto it = g_fm.find(h);
    if (it == g_fm.end()) return LAMSA_HP_EINVAL;
    EmuFm &f = it->second;
    if (q->k < 1 || q->k > 255 || q->max_occ < 0 || q->max_occ > HP_FM_MAX_OCC || q->n_win < 0 || q->seq_bytes < 0 || (q->n_win > 0 && (!q->win_off || !q->seq))) return LAMSA_HP_EINVAL;
    const int nw = q->n_win;
    if (nw > 0 && q->win_off[0] < 0) return LAMSA_HP_EINVAL;
    for (int w = 0; w < nw; ++w) if (q->win_off[w + 1] < q->win_off[w]) return LAMSA_HP_EINVAL;
    if (nw > 0 && q->win_off[nw] > q->seq_bytes) return LAMSA_HP_EINVAL;
    f.kmer_off.assign((size_t)nw + 1, 0);
    for (int w = 0; w < nw; ++w) { const int64_t len = q->win_off[w + 1] - q->win_off[w]; f.kmer_off[(size_t)w + 1] = f.kmer_off[(size_t)w] + (len >= q->k ? len - q->k + 1 : 0); }
    const int64_t n = f.kmer_off[(size_t)nw];
    f.lo.assign((size_t)n + 1, 0); f.hi.assign((size_t)n + 1, 0); f.pos_off.assign((size_t)n + 1, 0); f.pos.assign(1, 0);
    out->n_kmers = n; out->kmer_off = f.kmer_off.data(); out->lo = f.lo.data(); out->hi = f.hi.data(); out->pos_off = f.pos_off.data(); out->pos = f.pos.data();
    g_slices = 0;
    if (n == 0) return LAMSA_HP_OK;
    FmIx ix;
    ix.seq_len = f.ix.seq_len; ix.primary = f.ix.primary; for (int c = 0; c < 5; ++c) ix.L2[c] = f.ix.L2[c];
    ix.bwt = f.bwt.data(); ix.sa = f.sa.data(); ix.sa_intv = f.ix.sa_intv;
    std::vector<int32_t> cnt((size_t)n, 0);
    FmSearchArgs a;
    a.ix = ix; a.seq = q->seq; a.win_off = q->win_off; a.kmer_off = f.kmer_off.data(); a.n_win = nw; a.k = q->k; a.max_occ = q->max_occ; a.n_kmers = n;
    a.lo = f.lo.data(); a.hi = f.hi.data(); a.cnt = cnt.data();
    for (int64_t j = 0; j < n; ++j) fm_search_lane(a, j);
    if (q->max_occ == 0) return LAMSA_HP_OK;
    const int64_t n_tiles = (n + HP_FM_TILE - 1) / HP_FM_TILE;
    std::vector<int32_t> tsum((size_t)n_tiles, 0); std::vector<int64_t> toff((size_t)n_tiles + 1, 0);
    FmScanArgs sc;
    sc.cnt = cnt.data(); sc.n = n; sc.n_tiles = n_tiles; sc.tile_sum = tsum.data(); sc.tile_off = toff.data(); sc.pos_off = f.pos_off.data();
    for (int64_t t = 0; t < n_tiles; ++t) fm_scan_sums(sc, t);
    fm_scan_tiles(sc);
    for (int64_t t = 0; t < n_tiles; ++t) fm_scan_write(sc, t);
    const int64_t total = f.pos_off[(size_t)n];
    f.pos.assign((size_t)total + 1, 0);
    out->pos = f.pos.data();
    const int64_t slice = getenv("LAMSA_HP_FM_SLICE") ? (atoll(getenv("LAMSA_HP_FM_SLICE")) > 0 ? atoll(getenv("LAMSA_HP_FM_SLICE")) : 1) : ((int64_t)4 << 20);
    std::vector<uint64_t> buf;
    FmLocateArgs la;
    la.ix = ix; la.lo = f.lo.data(); la.pos_off = f.pos_off.data(); la.n_kmers = n;
    for (int64_t t0 = 0; t0 < total; t0 += slice, ++g_slices) {
        la.t0 = t0; la.t1 = total < t0 + slice ? total : t0 + slice;
        buf.assign((size_t)(la.t1 - la.t0), 0);                    // exactly the slice: a store outside it is one outside the allocation
        la.pos = buf.data();
        for (int64_t t = la.t0; t < la.t1; ++t) fm_locate_lane(la, t);
        for (int64_t t = la.t0; t < la.t1; ++t) f.pos[(size_t)t] = buf[(size_t)(t - la.t0)];
    }
    return LAMSA_HP_OK;
}
