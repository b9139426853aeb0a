// emu_seed.cpp -- TEST INFRASTRUCTURE: lamsa_hp_fm_seed of include/lamsa_hp.h on the CPU lane emulation: the lanes are
// lamsa_amd/csrc/hp_seed.h as the device compiles it, the scans hp_fm.h's; only the launches are loops here, and every per-slice buffer is
// allocated at exactly the slice's size, so that a store outside it is one outside the allocation.  The index is the one emu_fm.cpp keeps
// (lamsa_hp_fm_load), in an unnamed namespace: that file is included as text, and this file is linked in its place
// (tests/seedlib.py: a shared library, the emulated host program with --seed-fm, the sanitizer check program).
#include "emu_fm.cpp"
#include "hp_seed.h"

namespace {
struct EmuSeed {
    std::vector<int32_t> all, last, seed_id, chr; std::vector<int64_t> sd_off, seed_off, hit_off, pos;
    std::vector<int8_t> strand; std::vector<int16_t> nm, len_dif; std::vector<uint8_t> cig_n, cig8;
};
std::map<const void *, EmuSeed> g_seed;
long long g_seed_slices = 0;

void scan_counts(const int32_t *cnt, int64_t n, int64_t *off)
{
    const int64_t n_tiles = (n + HP_FM_TILE - 1) / HP_FM_TILE;
    std::vector<int32_t> tsum((size_t)n_tiles, 0); std::vector<int64_t> toff((size_t)n_tiles + 1, 0);
    FmScanArgs sc;
    sc.cnt = cnt; sc.n = n; sc.n_tiles = n_tiles; sc.tile_sum = tsum.data(); sc.tile_off = toff.data(); sc.pos_off = off;
    for (int64_t t = 0; t < n_tiles; ++t) fm_scan_sums(sc, t);
    fm_scan_tiles(sc);
    for (int64_t t = 0; t < n_tiles; ++t) fm_scan_write(sc, t);
}
}

extern "C" long long emu_seed_last_slices() { return g_seed_slices; }      // locate slices of the last seeding call

extern "C" int lamsa_hp_fm_seed(lamsa_hp_handle *h, const lamsa_hp_seed_queries *q, lamsa_hp_batch *out)
{
    if (!h || !q || !out) return LAMSA_HP_EINVAL;
    auto it = g_fm.find(h);
    if (it == g_fm.end()) return LAMSA_HP_EINVAL;
    EmuFm &f = it->second;
    if (q->seed_len < 1 || q->seed_len > 63 || q->seed_step < 1 || q->max_hits < 1 || q->max_hits > HP_SEED_MAX_HITS) return LAMSA_HP_EINVAL;
    const int n = q->n_reads, nc = q->n_seqs;
    if (n < 0 || (n > 0 && (!q->read_off || !q->read_seq))) return LAMSA_HP_EINVAL;
    if (nc < 1 || !q->seq_offset || !q->seq_len || q->seq_offset[0] != 0) return LAMSA_HP_EINVAL;
    for (int c = 0; c < nc; ++c) if (q->seq_len[c] < 0 || (c + 1 < nc && q->seq_offset[c + 1] != q->seq_offset[c] + q->seq_len[c])) return LAMSA_HP_EINVAL;
    const int64_t l_pac = q->seq_offset[nc - 1] + q->seq_len[nc - 1];
    if ((f.ix.seq_len & 1) || (uint64_t)l_pac != f.ix.seq_len / 2) return LAMSA_HP_EINVAL;
    if (n > 0 && q->read_off[0] != 0) return LAMSA_HP_EINVAL;
    EmuSeed &e = g_seed[h];
    e.all.assign((size_t)n + 1, 0); e.last.assign((size_t)n + 1, 0); e.sd_off.assign((size_t)n + 1, 0); e.seed_off.assign((size_t)n + 1, 0);
    for (int r = 0; r < n; ++r) {
        const int64_t L = q->read_off[r + 1] - q->read_off[r];
        if (L < 0 || L > (1 << 24)) return LAMSA_HP_EINVAL;
        const int64_t sa = L < q->seed_len ? 0 : 1 + (L - q->seed_len) / q->seed_step;
        e.all[(size_t)r] = (int32_t)sa; e.last[(size_t)r] = (int32_t)(L - q->seed_len - (sa - 1) * q->seed_step);
        e.sd_off[(size_t)r + 1] = e.sd_off[(size_t)r] + sa;
    }
    const int64_t n_bases = n ? q->read_off[n] : 0, N = e.sd_off[(size_t)n];
    for (int64_t i = 0; i < n_bases; ++i) if (q->read_seq[i] > 4) return LAMSA_HP_EINVAL;
    e.seed_id.assign(1, 0); e.hit_off.assign(1, 0); e.pos.assign(1, 0); e.chr.assign(1, 0); e.strand.assign(1, 0);
    e.nm.assign(1, 0); e.len_dif.assign(1, 0); e.cig_n.assign(1, 0); e.cig8.assign(1, 0);
    static const int64_t zero64 = 0; static const uint8_t zero8 = 0;
    int64_t n_hits = 0;
    auto hand_out = [&]() {
        out->n_reads = n; out->read_off = q->read_off ? q->read_off : &zero64; out->read_seq = q->read_seq ? q->read_seq : &zero8;
        out->seed_all = e.all.data(); out->last_len = e.last.data(); out->seed_off = e.seed_off.data(); out->seed_id = e.seed_id.data(); out->hit_off = e.hit_off.data();
        out->h_pos = e.pos.data(); out->h_chr = e.chr.data(); out->h_strand = e.strand.data(); out->h_nm = e.nm.data(); out->h_len_dif = e.len_dif.data();
        out->h_cig_off = nullptr; out->h_cig_n = e.cig_n.data(); out->cig = nullptr; out->n_cig = n_hits; out->cig8 = e.cig8.data();
    };
    hand_out();
    g_seed_slices = 0;
    if (N == 0) return LAMSA_HP_OK;

    const size_t nN = (size_t)N;
    std::vector<uint64_t> lo(nN); std::vector<int32_t> cnt(nN), over(nN), kept(nN, -1), slot(nN);
    std::vector<int64_t> row_off(nN + 1), slot_off(nN + 1), kept_off(nN + 1);
    SeedArgs a; memset(&a, 0, sizeof a);
    a.ix.seq_len = f.ix.seq_len; a.ix.primary = f.ix.primary; for (int c = 0; c < 5; ++c) a.ix.L2[c] = f.ix.L2[c];
    a.ix.bwt = f.bwt.data(); a.ix.sa = f.sa.data(); a.ix.sa_intv = f.ix.sa_intv;
    a.read_seq = q->read_seq; a.read_off = q->read_off; a.sd_off = e.sd_off.data();
    a.n_reads = n; a.seed_len = q->seed_len; a.seed_step = q->seed_step; a.max_hits = q->max_hits; a.n_seeds = N;
    a.seq_offset = q->seq_offset; a.seq_len = q->seq_len; a.n_seqs = nc; a.l_pac = l_pac;
    a.lo = lo.data(); a.cnt = cnt.data(); a.over = over.data(); a.kept = kept.data(); a.slot = slot.data();
    a.row_off = row_off.data(); a.slot_off = slot_off.data(); a.kept_off = kept_off.data();
    for (int64_t j = 0; j < N; ++j) seed_search_lane(a, j);
    scan_counts(cnt.data(), N, row_off.data());
    const int64_t total = row_off[nN];
    const int64_t slice = getenv("LAMSA_HP_FM_SLICE") ? (atoll(getenv("LAMSA_HP_FM_SLICE")) > 0 ? atoll(getenv("LAMSA_HP_FM_SLICE")) : 1) : ((int64_t)4 << 20);
    e.pos.clear(); e.chr.clear(); e.strand.clear();
    for (int64_t t0 = 0; t0 < total; t0 += slice, ++g_seed_slices) {
        a.t0 = t0; a.t1 = total < t0 + slice ? total : t0 + slice;
        const size_t m = (size_t)(a.t1 - a.t0);
        std::vector<int64_t> p_seed(m), p_pos(m), keep_off(m + 1); std::vector<int32_t> p_chr(m), keep(m);
        a.p_seed = p_seed.data(); a.p_pos = p_pos.data(); a.p_chr = p_chr.data(); a.keep = keep.data(); a.keep_off = keep_off.data();
        for (int64_t t = a.t0; t < a.t1; ++t) seed_locate_lane(a, t);
        scan_counts(keep.data(), (int64_t)m, keep_off.data());
        const size_t got = (size_t)keep_off[m];
        std::vector<int64_t> s_pos(got); std::vector<int32_t> s_chr(got); std::vector<int8_t> s_strand(got);      // exactly the kept rows
        a.s_pos = s_pos.data(); a.s_chr = s_chr.data(); a.s_strand = s_strand.data();
        for (int64_t t = a.t1 - 1; t >= a.t0; --t) seed_hits_lane(a, t);                                           // (lanes run in no particular order)
        e.pos.insert(e.pos.end(), s_pos.begin(), s_pos.end()); e.chr.insert(e.chr.end(), s_chr.begin(), s_chr.end()); e.strand.insert(e.strand.end(), s_strand.begin(), s_strand.end());
        n_hits += (int64_t)got;
    }
    for (int64_t j = 0; j < N; ++j) seed_slot_lane(a, j);
    scan_counts(slot.data(), N, slot_off.data());
    scan_counts(kept.data(), N, kept_off.data());
    const int64_t n_slots = slot_off[nN];
    if (kept_off[nN] != n_hits) return LAMSA_HP_EKERNEL;
    e.seed_id.assign((size_t)n_slots, 0); e.hit_off.assign((size_t)n_slots + 1, 0);                                 // exactly the slots
    a.seed_id = e.seed_id.data(); a.hit_off = e.hit_off.data(); a.seed_off = e.seed_off.data();
    for (int64_t x = N + n; x >= 0; --x) seed_emit_lane(a, x);
    e.seed_id.resize((size_t)n_slots + 1, 0);
    e.pos.resize((size_t)n_hits + 1); e.chr.resize((size_t)n_hits + 1); e.strand.resize((size_t)n_hits + 1);
    e.nm.assign((size_t)n_hits + 1, 0); e.len_dif.assign((size_t)n_hits + 1, 0); e.cig_n.assign((size_t)n_hits + 1, 1); e.cig8.assign((size_t)n_hits + 1, (uint8_t)q->seed_len);
    hand_out();
    return LAMSA_HP_OK;
}
