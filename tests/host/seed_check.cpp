// seed_check.cpp -- TEST INFRASTRUCTURE (tests/test_seed_cpu.py): lamsa_hp_fm_seed (tests/emu/emu_seed.cpp here: the lanes of
// lamsa_amd/csrc/hp_seed.h in loops) against the host's own FmIndex (lamsa_amd/host/rescue.cpp), one seed at a time, on the reads of a
// FASTA file read with the host's reader -- the host code a chunk goes through before and after the call.  A program of its own so that it
// can be built with -fsanitize=address,undefined and run directly.
// usage: seed_check <index prefix> <reads.fa>.  Every parameter set is seeded in one call, in slices of 7 rows and of 1000 rows.
// Prints "ok <calls> <seeds> <slots> <hits>"; exit code 1 and the first difference otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rescue.h"

using namespace lamsa;

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: seed_check <index prefix> <reads.fa>\n"); return 2; }
    Index ix; FmIndex fm; std::string err;
    if (!load_index(argv[1], ix, err) || !fm.load(argv[1], err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
    lamsa_hp_para P; lamsa_hp_para_init(&P); lamsa_hp_para_finish(&P);
    lamsa_hp_ref ref; ref.pac = ix.pac.data(); ref.l_pac = ix.l_pac; ref.n_seqs = (int32_t)ix.off.size(); ref.seq_offset = ix.off.data(); ref.seq_len = ix.len.data();
    lamsa_hp_handle *h = nullptr;
    if (lamsa_hp_create(&h, &P, &ref, 0) != LAMSA_HP_OK) return 2;
    lamsa_hp_fm_index fx; memset(&fx, 0, sizeof fx);
    fx.seq_len = fm.seq_len; fx.primary = fm.primary; for (int c = 0; c < 5; ++c) fx.L2[c] = fm.L2[c];
    fx.bwt = fm.bwt.data(); fx.bwt_words = (uint64_t)fm.bwt.size() - 4; fx.sa = fm.sa.data(); fx.n_sa = fm.n_sa; fx.sa_intv = fm.sa_intv;
    if (lamsa_hp_fm_load(h, &fx) != LAMSA_HP_OK) { fprintf(stderr, "lamsa_hp_fm_load failed\n"); return 2; }

    FastxReader rd;
    if (!rd.open(argv[2])) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    std::vector<int64_t> read_off(1, 0); std::vector<uint8_t> seq;
    Read r;
    while (rd.next(r)) {
        for (char ch : r.seq) seq.push_back(ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4);
        read_off.push_back((int64_t)seq.size());
    }
    const int n = (int)read_off.size() - 1;
    std::vector<uint8_t> exact(seq);                       // handed over without a byte to spare: a read behind the last base is one outside the allocation
    static const uint8_t none = 0;

    static const int sets[][3] = {{50, 100, 200}, {50, 25, 150}, {50, 25, 149}, {20, 10, 200}, {63, 63, 200}, {1, 1, 16383}};
    long calls = 0, seeds = 0, slots = 0, hits = 0;
    for (const auto &st : sets) for (const char *slice : {"7", "1000"}) {
        if (st[0] == 1 && slice[0] == '7') continue;        // (every base of every read, tens of thousands of rows each: once is enough)
        setenv("LAMSA_HP_FM_SLICE", slice, 1);
        const int sl = st[0], ss = st[1], mh = st[2];
        lamsa_hp_seed_queries q; memset(&q, 0, sizeof q);
        q.n_reads = n; q.read_off = read_off.data(); q.read_seq = exact.empty() ? &none : exact.data(); q.seed_len = sl; q.seed_step = ss; q.max_hits = mh;
        q.n_seqs = ref.n_seqs; q.seq_offset = ref.seq_offset; q.seq_len = ref.seq_len;
        lamsa_hp_batch b; memset(&b, 0, sizeof b);
        if (lamsa_hp_fm_seed(h, &q, &b) != LAMSA_HP_OK) { printf("set %d/%d/%d: lamsa_hp_fm_seed failed\n", sl, ss, mh); return 1; }
        ++calls;
#define FAIL(what) do { printf("set %d/%d/%d slice %s read %d seed %d: %s\n", sl, ss, mh, slice, rr, i + 1, what); return 1; } while (0)
        int64_t s = 0, k = 0;
        for (int rr = 0; rr < n; ++rr) {
            const int64_t L = read_off[(size_t)rr + 1] - read_off[(size_t)rr];
            const int sa = L < sl ? 0 : (int)(1 + (L - sl) / ss);
            int i = -1;
            if (b.seed_all[rr] != sa || b.last_len[rr] != L - sl - (int64_t)(sa - 1) * ss || b.seed_off[rr] != s) FAIL("seed_all / last_len / seed_off");
            for (i = 0; i < sa; ++i, ++seeds) {
                uint64_t lo = 0, hi = fm.seq_len;                                  // (in: the interval to start from, the whole index)
                const uint64_t cnt = fm.match(sl, seq.data() + read_off[(size_t)rr] + (int64_t)i * ss, &lo, &hi);
                std::vector<int64_t> pos; std::vector<int> chr, strand;
                for (uint64_t row = lo; cnt >= 1 && cnt <= (uint64_t)mh && row <= hi; ++row) {
                    const int64_t p = (int64_t)fm.sa_at(row);
                    const bool is_rev = p >= ix.l_pac;
                    const int64_t f = is_rev ? 2 * ix.l_pac - 1 - p : p;
                    int c = 0;
                    while (c + 1 < (int)ix.off.size() && ix.off[(size_t)c + 1] <= f) ++c;
                    const int64_t sp = f - ix.off[(size_t)c] + 1 - (is_rev ? sl - 1 : 0);
                    if (sp < 1 || sp + sl - 1 > ix.len[(size_t)c]) continue;
                    pos.push_back(sp); chr.push_back(c + 1); strand.push_back(is_rev ? -1 : 1);
                }
                const bool slot = !pos.empty() || cnt > (uint64_t)mh;
                if (!slot) continue;
                if (s >= b.seed_off[n] || b.seed_id[s] != i + 1 || b.hit_off[s] != k || b.hit_off[s + 1] != k + (int64_t)pos.size()) FAIL("slot");
                for (size_t x = 0; x < pos.size(); ++x, ++k)
                    if (b.h_pos[k] != pos[x] || b.h_chr[k] != chr[x] || b.h_strand[k] != strand[x] || b.h_nm[k] != 0 || b.h_len_dif[k] != 0 || b.h_cig_n[k] != 1 || b.cig8[k] != sl) FAIL("hit record");
                ++s;
            }
        }
        { const int rr = n, i = -1; if (b.seed_off[n] != s || b.hit_off[s] != k || b.n_cig != k || b.h_cig_off || b.cig) FAIL("totals"); }
#undef FAIL
        slots += (long)s; hits += (long)k;
    }
    printf("ok %ld %ld %ld %ld\n", calls, seeds, slots, hits);
    lamsa_hp_destroy(h);
    return 0;
}
