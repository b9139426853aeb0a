// emu_out.cpp -- TEST INFRASTRUCTURE (tests/test_out_cpu.py): the record-stream helpers of lamsa_amd/csrc/hp_out.h under the CPU lane
// emulation -- the capacity table, the lane copy next to guard words, and a covered interval written by out_reg and read back by reg_read.
#include "emu_api.cpp"

// Every capacity of hp_out.h for one (L, scale, tags), in the order of "names" in tests/golden/out_caps.json; n reads of L bases for the
// batch's stream, band_w and H hits for the one-kernel slab.  The last value is the arena bytes line_bufs takes.  Returns the count.
extern "C" int emu_out_caps(int L, int scale, int tags, int n, int band_w, int H, int64_t *v)
{
    int k = 0;
    const int ft = fill_tags(tags);
    v[k++] = line_ev_cap(L); v[k++] = line_ev_words(L); v[k++] = line_eqx_words(L); v[k++] = line_sum_words(); v[k++] = read_sum_words();
    v[k++] = line_tag_words(L, ft);
    v[k++] = line_cig_cap(L, scale);
    v[k++] = line_out_cap(L, ft);
    v[k++] = read_out_cap(L, scale, ft);
    v[k++] = batch_out_cap(n, (int64_t)n * L, tags);
    v[k++] = (int64_t)slab_per_base(tags, false); v[k++] = (int64_t)slab_per_base(tags, true);
    v[k++] = (int64_t)slab_fixed(tags, scale, false); v[k++] = (int64_t)slab_fixed(tags, 1, true);
    v[k++] = (int64_t)read_slab_bytes(band_w, L, H, scale, tags);
    v[k++] = (int64_t)fill_slab_bytes(L, tags, sizeof(cig_t) * 3 * HP_LJ_CIG * 64 + (size_t)HP_LJ_QSMALL * HP_LJ_TSMALL * 64 + 64);      // dp_bytes as slab_plan passes them (hp_align_api.hip)
    std::vector<char> slab((size_t)64 << 20);
    Ctx cx; memset(&cx, 0, sizeof cx); arena_init(cx.tmp, slab.data(), slab.size());
    const LineBufs b = line_bufs(cx, L, scale, ft);
    v[k++] = b.la && b.la->tags == ft && b.la->ev_cap == ((ft & HP_TAGS_LISTS) ? line_ev_cap(L) * scale : 0) && (b.la->ev != nullptr) == ((ft & HP_TAGS_LISTS) != 0) ? (int64_t)cx.tmp.top : -1;
    return k;
}

// out_copy of n elements into dst; width 4: the source is int32 words, width 2: int16 elements that the copy widens
extern "C" void emu_out_copy(int width, const void *src, int n, int32_t *dst)
{
    if (width == 4) out_copy(dst, (const int32_t *)src, n);
    else out_copy(dst, (const int16_t *)src, n);
}

// One covered interval -- in: beg, end, then is_rev, chr, pos_lo, pos_hi of its two reference ends -- through out_reg into words[0 .. cap),
// and those words back through reg_read (what phase_chain2 does) into `back`, same order.  Returns the status bits, *n_out the words written.
extern "C" int emu_out_reg(const int32_t *in, int32_t *words, int cap, int32_t *n_out, int32_t *back)
{
    int32_t be[2] = {in[0], in[1]}, be2[2] = {0, 0};
    RegB ends[2], ends2[2];
    for (int e = 0; e < 2; ++e) { ends[e].is_rev = in[2 + 4 * e]; ends[e].chr = in[3 + 4 * e]; ends[e].pos = (int64_t)(((uint64_t)(uint32_t)in[5 + 4 * e] << 32) | (uint32_t)in[4 + 4 * e]); }
    Regs G; memset(&G, 0, sizeof G); G.n = 1; G.beg = be; G.end = be + 1; G.rb = ends; G.re = ends + 1;
    Ctx cx; memset(&cx, 0, sizeof cx);
    OutBuf o; o.w = words; o.n = 0; o.cap = cap;
    out_reg(cx, o, G, 0);
    *n_out = o.n;
    if (o.n == PH_REG_WORDS) {
        Regs B; memset(&B, 0, sizeof B); B.beg = be2; B.end = be2 + 1; B.rb = ends2; B.re = ends2 + 1;
        reg_read(words, B, 0);
        back[0] = be2[0]; back[1] = be2[1];
        for (int e = 0; e < 2; ++e) { back[2 + 4 * e] = ends2[e].is_rev; back[3 + 4 * e] = ends2[e].chr; back[4 + 4 * e] = (int32_t)(ends2[e].pos & 0xffffffffll); back[5 + 4 * e] = (int32_t)(ends2[e].pos >> 32); }
    }
    return cx.status;
}
