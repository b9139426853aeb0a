// emu_summary.cpp -- TEST INFRASTRUCTURE (tests/test_paf_cpu.py): the per-read path with LAMSA_HP_TAG_SUMMARY under the CPU lane emulation.
// The path itself is emu_align_batch_tags of emu_eqx.cpp, which is included as it is and brings emu_api.cpp (the emulation's globals, LDS
// guards, sort widths) with it; what is added here is what lamsa_hp_set_result_tags does in front of it -- the device sources' own check of
// the flags -- and one record through out_line, so that the 15-lane store is seen next to guard words.
#include "emu_eqx.cpp"

// 1 if lamsa_hp_set_result_tags accepts `flags` (result_tags_valid, hp_out.h: the product's routine calls the same function)
extern "C" int emu_result_tags_valid(int flags) { return result_tags_valid(flags) ? 1 : 0; }

// emu_align_batch_tags behind that check: LAMSA_HP_EINVAL and nothing written for flags the product refuses
extern "C" int emu_align_batch_checked(const lamsa_hp_para *P, const lamsa_hp_ref *ref, const lamsa_hp_batch *B, int scale, int phased, int tags, size_t slab_bytes,
                                       int32_t *stream, int64_t stream_cap, int64_t *n_words, int64_t *read_off, int32_t *read_len, int32_t *status)
{
    if (!result_tags_valid(tags)) return LAMSA_HP_EINVAL;
    return emu_align_batch_tags(P, ref, B, scale, phased, tags, slab_bytes, stream, stream_cap, n_words, read_off, read_len, status);
}

// One record serialised by out_line with LAMSA_HP_TAG_SUMMARY into out[0 .. cap): hdr = offset_lo, offset_hi, chr, nstrand, score, NM;
// cigar_n is cn, sum the eight words res_aux would have left in the record.  Returns the status bits, *n_out = words written (4 line
// words, then the record).
extern "C" int emu_summary_record(const int32_t *hdr, const int32_t *cig, int cn, const int32_t *sum, int32_t *out, int cap, int32_t *n_out)
{
    std::vector<cig_t> c(cig, cig + cn); c.push_back(0);
    std::vector<LineRes> lav(1);
    LineRes &la = lav[0];
    memset(&la, 0, sizeof la);
    la.cur_res_n = 0; la.tags = LAMSA_HP_TAG_SUMMARY;
    Rec &r = la.rec[0];
    cig_bind(r.cig, c.data(), cn); r.cig.n = cn;
    r.offset = (int64_t)(((uint64_t)(uint32_t)hdr[1] << 32) | (uint32_t)hdr[0]); r.chr = hdr[2]; r.nstrand = hdr[3]; r.score = hdr[4]; r.NM = hdr[5];
    for (int k = 0; k < 8; ++k) r.sum[k] = sum[k];
    Ctx cx; memset(&cx, 0, sizeof cx);
    OutBuf o; o.w = out; o.n = 0; o.cap = cap;
    out_line(cx, o, la);
    *n_out = o.n;
    return cx.status;
}
