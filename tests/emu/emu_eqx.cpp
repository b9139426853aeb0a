// emu_eqx.cpp -- TEST INFRASTRUCTURE (tests/test_eqx_cpu.py): the =/X routine of the device sources (lamsa_amd/csrc/hp_eqx.h) on
// explicit inputs, and the whole per-read path with result tags set, both under the CPU lane emulation.  The set-up (the emulation's
// globals, LDS guards, sort widths) is emu_api.cpp's, which is included as it is.
#include "emu_api.cpp"

// One record (its CIGAR in M form and its mismatch list) serialised by out_line with LAMSA_HP_TAG_EQX into out[0 .. cap): returns the
// status bits, *n_out = words written.  The record's words start at out[4]: 6 header words, cigar_n, the =/X words.
extern "C" int emu_eqx_record(const int32_t *cig, int cn, const int32_t *mm, int n_mm, int32_t *out, int cap, int32_t *n_out)
{
    std::vector<cig_t> c(cig, cig + cn); c.push_back(0);
    std::vector<int32_t> m(mm, mm + n_mm); m.push_back(0);
    std::vector<LineRes> lav(1);
    LineRes &la = lav[0];
    memset(&la, 0, sizeof la);
    la.cur_res_n = 0; la.ev = m.data(); la.ev_cap = n_mm; la.tags = LAMSA_HP_TAG_EQX;
    Rec &r = la.rec[0];
    cig_bind(r.cig, c.data(), cn); r.cig.n = cn;
    r.mm = m.data(); r.n_mm = n_mm; r.chr = 1; r.nstrand = 1; r.offset = 1;
    Ctx cx; memset(&cx, 0, sizeof cx);
    OutBuf o; o.w = out; o.n = 0; o.cap = cap;
    out_line(cx, o, la);
    *n_out = o.n;
    for (size_t i = 0; i < (size_t)cn; ++i) if (c[i] != cig[i]) return -1;       // the record's own CIGAR stays in M form
    return cx.status;
}

// emu_align_batch (emu_api.cpp) with BatchIn::tags set: the phased path for scale 1 (unless `phased` is 0), else the one-kernel path.
extern "C" int emu_align_batch_tags(const lamsa_hp_para *P, const lamsa_hp_ref *ref, const lamsa_hp_batch *B, int scale, int phased, int tags, size_t slab_bytes,
                                    int32_t *stream, int64_t stream_cap, int64_t *n_words, int64_t *read_off, int32_t *read_len, int32_t *status)
{
    AlignArgs a;
    a.P = *P;
    a.ref.pac = ref->pac; a.ref.l_pac = ref->l_pac; a.ref.n_seqs = ref->n_seqs; a.ref.seq_off = ref->seq_offset; a.ref.seq_len = ref->seq_len;
    a.in.n_reads = B->n_reads; a.in.read_skip = nullptr; a.in.read_off = B->read_off; a.in.read_seq = B->read_seq; a.in.seed_all = B->seed_all; a.in.last_len = B->last_len;
    a.in.seed_off = B->seed_off; a.in.seed_id = B->seed_id; a.in.hit_off = B->hit_off; a.in.h_pos = B->h_pos; a.in.h_chr = B->h_chr;
    const int64_t n_hits_all = B->n_reads ? B->hit_off[B->seed_off[B->n_reads]] : 0;
    std::vector<int64_t> off64((size_t)n_hits_all + 1, 0); std::vector<int32_t> words;
    { int64_t run = 0; for (int64_t k = 0; k < n_hits_all; ++k) { off64[k] = B->h_cig_off ? (int64_t)B->h_cig_off[k] : run; run += B->h_cig_n[k]; } }
    if (B->cig8) { words.resize((size_t)B->n_cig + 1); for (int64_t i = 0; i < B->n_cig; ++i) words[i] = ((B->cig8[i] & 63) << 4) | (B->cig8[i] >> 6); }
    a.in.h_cig_off = off64.data(); a.in.h_nm = B->h_nm; a.in.h_len_dif = B->h_len_dif; a.in.h_strand = B->h_strand; a.in.h_cig_n = B->h_cig_n; a.in.cig = B->cig8 ? words.data() : B->cig;
    a.in.tags = tags;
    emu_sort_widths(a.in, B->n_reads, a.sort_pb, a.sort_cb);
    unsigned long long cursor = 0;
    a.out.stream = stream; a.out.stream_cap = stream_cap; a.out.cursor = &cursor;
    a.out.read_out_off = read_off; a.out.read_out_len = read_len; a.out.read_status = status; a.out.read_tbases = nullptr; a.out.read_work = nullptr; a.out.diag = nullptr;
    std::vector<char> slab(slab_bytes);
    EMU_LDS(lds, EMU_CHAIN_LDS_MAX);
    if (scale == 1 && phased) {
        PhaseArgs p;
        p.P = a.P; p.ref = a.ref; p.in = a.in; p.out = a.out; p.slab = slab.data(); p.slab_per_wave = slab_bytes; p.slab_fill = slab_bytes; p.slab_wj = slab_bytes; p.slab_wjb = slab_bytes; p.wjb_off = 0; p.n_wjb = 1;
        p.sort_pb = a.sort_pb; p.sort_cb = a.sort_cb; p.order = nullptr; p.n_reads = B->n_reads; p.prof = nullptr;
        const int n = B->n_reads;
        const int64_t n_hits = n ? B->hit_off[B->seed_off[n]] : 0, n_bases = n ? B->read_off[n] : 0;
        std::vector<NodeS> nd((size_t)(n_hits + n) + 1); std::vector<int32_t> nseed((size_t)(n_hits + n) + 1), sidx(2 * (size_t)(n_hits + n) + 2);
        std::vector<RdMeta> meta((size_t)n + 1); memset(meta.data(), 0, sizeof(RdMeta) * meta.size());
        p.unit_cap = 8 * n + 64;
        std::vector<UnitRec> units(2 * (size_t)p.unit_cap); std::vector<int32_t> bq(2 * (size_t)PH_NBUCKET * p.unit_cap);
        p.line_cap = stream_cap + 16 * 2 * (int64_t)p.unit_cap;
        p.fl_cap = 32 * (n_hits + n) + 4096 * (int64_t)n + 4096;
        p.job_cap = 4096 + 1024 * (int64_t)n + 8 * n_bases;
        std::vector<int32_t> fl((size_t)p.fl_cap), lines((size_t)p.line_cap), jobsv((size_t)p.job_cap + 4);
        p.job_base = jobsv.data();
        p.lj_cap = (int)(1024 + 64 * (int64_t)n + n_bases / 8);
        std::vector<LjRec> ljv((size_t)p.lj_cap + 1); std::vector<int32_t> ljq((size_t)LJ_NBUCKET * p.lj_cap + 1);
        p.ljobs = ljv.data(); p.lj_bucket = ljq.data();
        p.wj_cap = p.lj_cap;
        std::vector<WjRec> wjv((size_t)p.wj_cap + 1); std::vector<int32_t> wjq((size_t)WJ_NBUCKET * p.wj_cap + 1);
        p.wjobs = wjv.data(); p.wj_bucket = wjq.data();
        EMU_LDS(lds_lj, HP_LJ_LDS_WORDS(HP_LJ_QCAP));
        EMU_LDS(lds_wj, HP_WJ_LDS_WORDS);
        const int cw = HP_CHAIN_LDS_WORDS;
        PhaseCtl ctl; memset(&ctl, 0, sizeof ctl);
        p.g_nd = nd.data(); p.g_nseed = nseed.data(); p.g_sidx = sidx.data(); p.meta = meta.data(); p.units = units.data(); p.bucket_q = bq.data();
        p.fl_base = fl.data(); p.line_base = lines.data(); p.ctl = &ctl;
        auto fill_all = [&](int round) {
            for (int b = 0; b < PH_NBUCKET; ++b)
                for (int i = 0; i < ctl.bucket_n[round][b]; ++i) emu_guarded(lds, 0, [&] { phase_filllist(p, round, bq[((size_t)round * PH_NBUCKET + b) * p.unit_cap + i], 0, lds); });
            int nw = 0, nwb = 0;
            for (int b = 0; b < WJ_NBUCKET; ++b) { const int k = wj_queue_n(p, round, b); if (b < WJ_NBIG) nwb += k; else nw += k; }
            for (int g = 0; g < nwb; ++g) emu_guarded(lds_wj, HP_WJ_LDS_WORDS, [&] { phase_wavejob(p, round, g, true, 0, lds_wj); });
            for (int g = 0; g < nw; ++g) emu_guarded(lds_wj, HP_WJ_LDS_WORDS, [&] { phase_wavejob(p, round, g, false, 0, lds_wj); });
            for (int b = 0; b < LJ_NBUCKET; ++b)
                for (int off = 0; off < lj_queue_n(p, round, b); off += 64) emu_guarded(lds_lj, HP_LJ_LDS_WORDS(HP_LJ_QSMALL), [&] { phase_filldp(p, round, b, off, 0, lds_lj, HP_LJ_QSMALL); });
            for (int b = 0; b < PH_NBUCKET; ++b)
                for (int i = 0; i < ctl.bucket_n[round][b]; ++i) emu_guarded(lds, HP_LDS_WORDS, [&] { phase_fill(p, round, bq[((size_t)round * PH_NBUCKET + b) * p.unit_cap + i], 0, lds); });
        };
        for (int r = 0; r < n; ++r) emu_guarded(lds, cw, [&] { phase_chain1(p, r, 0, lds, cw); });
        fill_all(0);
        for (int r = 0; r < n; ++r) emu_guarded(lds, cw, [&] { phase_chain2(p, r, 0, lds, cw); });
        fill_all(1);
        for (int r = 0; r < n; ++r) phase_publish(p, r);
        *n_words = (int64_t)cursor;
        return 0;
    }
    a.slab = slab.data(); a.slab_per_wave = slab_bytes; a.counter = nullptr; a.order = nullptr; a.n_units = B->n_reads; a.scale = scale; a.prof = nullptr;
    for (int r = 0; r < B->n_reads; ++r) emu_guarded(lds, HP_BOTH_LDS_WORDS, [&] { align_read(a, r, 0, lds); });
    *n_words = (int64_t)cursor;
    return 0;
}
