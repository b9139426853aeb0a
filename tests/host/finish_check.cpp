// finish_check.cpp -- TEST INFRASTRUCTURE (tests/test_out_cpu.py): parse_stream and read_finish of lamsa_amd/host on result streams that a
// test wrote, as a program of its own so that it can be built with -fsanitize=address,undefined and run directly.
// usage: finish_check <index prefix> <in> <out> <what>.  <in>: int32 words -- n_reads, then per read L, n_words, the L base codes (a word
// each), the n_words of its flag-off stream.  <out>: per read its status, then per record of rounds 1 and 2 the seven header words
// (cigar_n of the finished CIGAR), the CIGAR, n_mm and the list, reg_beg, reg_end and the six summary fields.  Prints "ok <records>".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "rescue.h"

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    lamsa::Index ix; std::string err;
    if (!lamsa::load_index(argv[1], ix, err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
    std::vector<int32_t> in;
    { FILE *f = fopen(argv[2], "rb"); if (!f) return 2; int32_t w; while (fread(&w, 4, 1, f) == 1) in.push_back(w); fclose(f); }
    const int what = atoi(argv[4]);
    std::vector<int32_t> out;
    long n_rec = 0;
    size_t i = 1;
    lamsa::ReadResult R;                                   // one for all reads, as the host program reuses its own
    for (int r = 0; r < in[0]; ++r) {
        const int L = in[i], nw = in[i + 1]; i += 2;
        std::vector<uint8_t> codes(in.begin() + (long)i, in.begin() + (long)i + L); i += (size_t)L;
        lamsa::parse_stream(in.data() + i, nw, L, R, 0); i += (size_t)nw;
        lamsa::read_finish(R, codes.data(), L, ix, what);
        out.push_back(R.status);
        for (int st = 0; st < 2; ++st)
            for (const lamsa::Line &ln : R.stage[st])
                for (const lamsa::Rec &x : ln.rec) {
                    const int32_t hdr[7] = {(int32_t)(x.offset & 0xffffffffll), (int32_t)(x.offset >> 32), x.chr, x.nstrand, x.score, x.NM, (int32_t)x.cigar.size()};
                    out.insert(out.end(), hdr, hdr + 7); out.insert(out.end(), x.cigar.begin(), x.cigar.end());
                    out.push_back((int32_t)x.mm.size()); out.insert(out.end(), x.mm.begin(), x.mm.end());
                    const int32_t sum[8] = {x.reg_beg, x.reg_end, x.ref_span, x.m_bases, x.ins_bases, x.del_bases, x.ins_runs, x.del_runs};
                    out.insert(out.end(), sum, sum + 8);
                    ++n_rec;
                }
    }
    if (i != in.size()) { printf("input not consumed\n"); return 1; }
    { FILE *f = fopen(argv[3], "wb"); if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2; fclose(f); }
    printf("ok %ld\n", n_rec);
    return 0;
}
