// emu_lanedp.cpp -- TEST INFRASTRUCTURE: explicit job sets through the lane DP of the read path (phase_filldp, hp_phase.h) under the CPU lane
// emulation, with its two stages or in one (tests/lanedp_jobs.py).  Everything of emu_api.cpp is part of this library too, so the path counters
// (emu_stat) and the whole-read entry points see the same build.
int g_emu_lj_hard_cap = 1 << 30;       // tests: entries a hard queue of the lane DP takes (a full one leaves its jobs to the fill)
#define HP_LJ_HARD_CAP_RT(cap) (g_emu_lj_hard_cap < (cap) ? g_emu_lj_hard_cap : (cap))
#include "emu_api.cpp"

// Jobs of type 1 (ksw_bi_extend(100, 100)) or 2 (ksw_global2(band_w)), queries of 1 .. HP_LJ_QSMALL and targets of up to HP_LJ_TSMALL bases without N, listed into
// the queues as the lister would (kind and query class, in job order) and run by the driver loop of emu_api.cpp: every queue in ascending order, groups of 64.
// stages 0: PhaseCtl::lj_one_stage.  hard_cap > 0: the capacity of a hard queue.  Per job: has (the slot was published), cells (what the job added to
// its read's cell count: every job is its own read), hard (the job went through a hard queue), the CIGAR (HP_LJ_CIG words each).
extern "C" int emu_lane_stages(const lamsa_hp_para *P, int n, const uint8_t *seq, const int64_t *q_off, const int32_t *qlen, const int64_t *t_off, const int32_t *tlen,
                               const int32_t *type, int stages, int hard_cap, int32_t *has, int32_t *cells, int32_t *hard, int32_t *cig_n, int32_t *cig)
{
    if (!lj_params_ok(P)) return -2;
    int64_t tot = 0;
    for (int i = 0; i < n; ++i) { if (qlen[i] < 1 || qlen[i] > HP_LJ_QSMALL || tlen[i] < 0 || tlen[i] > HP_LJ_TSMALL || (type[i] != 1 && type[i] != 2)) return -1; tot += tlen[i]; }
    std::vector<uint8_t> pac((size_t)tot / 4 + 8, 0);
    PhaseArgs p; memset((void *)&p, 0, sizeof p);
    PhaseCtl ctl; memset(&ctl, 0, sizeof ctl);
    ctl.lj_one_stage = stages ? 0 : 1;
    g_emu_lj_hard_cap = hard_cap > 0 ? hard_cap : 1 << 30;
    p.P = *P; p.ctl = &ctl; p.in.read_seq = seq; p.ref.pac = pac.data();
    p.lj_cap = n + 1;
    std::vector<LjRec> ljv((size_t)p.lj_cap + 1); std::vector<int32_t> ljq((size_t)LJ_NBUCKET * p.lj_cap + 1, -1);
    std::vector<int32_t> fl((size_t)GS_WORDS * (n + 1), 0), jobsv((size_t)n * HP_LJ_CIG + 64);
    std::vector<RdMeta> meta((size_t)n + 1); memset((void *)meta.data(), 0, sizeof(RdMeta) * meta.size());
    p.ljobs = ljv.data(); p.lj_bucket = ljq.data(); p.fl_base = fl.data(); p.job_base = jobsv.data(); p.job_cap = (int64_t)n * HP_LJ_CIG; p.meta = meta.data();
    const size_t slab_bytes = sizeof(cig_t) * 3 * HP_LJ_CIG * 64 + (size_t)HP_LJ_QSMALL * HP_LJ_TSMALL * 64 + 64;
    std::vector<char> slab(slab_bytes);
    p.slab = slab.data(); p.slab_fill = slab_bytes;
    int64_t k = 0;
    for (int i = 0; i < n; ++i) {
        LjRec &R = ljv[i];
        R.qaddr = q_off[i]; R.tk = k; R.slot = (int64_t)GS_WORDS * i; R.rd = i; R.tlen = (uint16_t)tlen[i]; R.qlen = (uint8_t)qlen[i]; R.type_comp = (int8_t)type[i];
        for (int j = 0; j < tlen[i]; ++j, ++k) { if (seq[t_off[i] + j] > 3) return -1; pac[k >> 2] |= (uint8_t)((seq[t_off[i] + j] & 3) << ((~k & 3) << 1)); }
        const int b = lj_bucket_of(type[i], qlen[i]);
        ljq[(size_t)b * p.lj_cap + ctl.lj_bucket_n[0][b]++] = i;
        ++ctl.lj_n[0];
    }
    EMU_LDS(lds_lj, HP_LJ_LDS_WORDS(HP_LJ_QCAP));
    const int round = 0;
    for (int b = 0; b < LJ_NBUCKET; ++b)
        for (int off = 0; off < lj_queue_n(p, round, b); off += 64) emu_guarded(lds_lj, HP_LJ_LDS_WORDS(HP_LJ_QSMALL), [&] { phase_filldp(p, round, b, off, 0, lds_lj, HP_LJ_QSMALL); });
    for (int i = 0; i < n; ++i) {
        const int32_t *slot = fl.data() + (size_t)GS_WORDS * i;
        has[i] = slot[GS_HAS]; cells[i] = meta[i].cells; hard[i] = 0; cig_n[i] = slot[GS_HAS] ? slot[GS_N] : 0;
        if (slot[GS_HAS]) memcpy(cig + (size_t)i * HP_LJ_CIG, jobsv.data() + slot[GS_OFF], sizeof(int32_t) * (size_t)slot[GS_N]);
    }
    for (int b = LJ_NORD; b < LJ_NBUCKET; ++b)
        for (int q = 0; q < lj_queue_n(p, round, b); ++q) hard[ljq[(size_t)b * p.lj_cap + q]] = 1;
    g_emu_lj_hard_cap = 1 << 30;
    return 0;
}

// how lj_bi_extend(100, 100) ends each job (LJ_X_*, hp_lanedp.h), one job at a time: the labels tests/lanedp_jobs.py keeps for its pool
extern "C" int emu_lane_exits(const lamsa_hp_para *P, int n, const uint8_t *seq, const int64_t *q_off, const int32_t *qlen, const int64_t *t_off, const int32_t *tlen, int32_t *exit_code)
{
    if (!lj_params_ok(P)) return -2;
    std::vector<uint8_t> z((size_t)HP_LJ_QCAP * HP_LJ_TCAP * 64 + 64);
    std::vector<cig_t> cb((size_t)3 * HP_LJ_CIG);
    EMU_LDS(lds_lj, HP_LJ_LDS_WORDS(HP_LJ_QCAP));
    for (int i = 0; i < n; ++i) {
        if (qlen[i] < 1 || qlen[i] > HP_LJ_QCAP || tlen[i] < 0 || tlen[i] > HP_LJ_TCAP) return -1;
        std::vector<uint8_t> pac((size_t)tlen[i] / 4 + 8, 0);
        for (int j = 0; j < tlen[i]; ++j) pac[j >> 2] |= (uint8_t)((seq[t_off[i] + j] & 3) << ((~j & 3) << 1));
        LaneJob J; J.q = seq + q_off[i]; J.qs = 1; J.qcomp = 0; J.qlen = qlen[i]; J.pac = pac.data(); J.tk = 0; J.ts = 1; J.tlen = tlen[i]; J.z = z.data(); J.zl = 0; J.zs = HP_LJ_QCAP; J.cells = 0;
        J.row = lds_lj; J.qrow = (uint8_t *)(lds_lj + (HP_LJ_QCAP + 2) * 64); J.rev = 0; J.exit = -1;
        lj_stage_query(J);
        LCig out, Lc, Rc; out.c = cb.data(); out.n = 0; Lc.c = out.c + HP_LJ_CIG; Lc.n = 0; Rc.c = Lc.c + HP_LJ_CIG; Rc.n = 0;
        lj_bi_extend(P, J, 100, 100, Lc, Rc, out);
        exit_code[i] = J.exit;
    }
    return 0;
}

extern "C" void emu_set_lj_hard_cap(int cap) { g_emu_lj_hard_cap = cap > 0 ? cap : 1 << 30; }      // for the whole-read path (emu_align_batch) of this library
