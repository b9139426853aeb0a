// seed_fm_ab.cpp -- one process that seeds the same reads twice: through the host FmIndex of lamsa_amd/host/rescue.cpp on N threads, a seed
// at a time, and through lamsa_hp_fm_seed on the GPU (--seed-fm).  tools/seed_fm_ab.py builds the index and this program and writes
// profiles/seed_fm_ab.txt from what it prints.
// usage: seed_fm_ab <index prefix> <reads> <read length> <threads>
// The reads are cut from the forward text at random places (seeded), every other one reverse-complemented, and every base is replaced by
// another one with the error rate (substitutions only).  Seeds: 50 bases every 100, at most 200 hits.  At 1 % error both sides make the
// hit records of the definition in include/lamsa_hp.h and the records are compared; at 5 % and 12 % only the device runs, for the shares
// of seeds with a hit and of reads with fewer than two seeded slots.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>
#include "rescue.h"

using namespace lamsa;
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Hit { int64_t pos; int32_t chr; int8_t strand; };

int main(int argc, char **argv)
{
    if (argc != 5) { fprintf(stderr, "usage: seed_fm_ab <index prefix> <reads> <read length> <threads>\n"); return 2; }
    const int n = atoi(argv[2]), rlen = atoi(argv[3]), threads = atoi(argv[4]), sl = 50, ss = 100, mh = 200;
    Index ix; FmIndex fm; std::string err;
    if (!load_index(argv[1], ix, err) || !fm.load(argv[1], err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
    const int per = rlen < sl ? 0 : 1 + (rlen - sl) / ss;
    lamsa_hp_para P; lamsa_hp_para_init(&P); lamsa_hp_para_finish(&P);
    lamsa_hp_handle *h = nullptr;
    if (lamsa_hp_create(&h, &P, nullptr, 0) != LAMSA_HP_OK) { fprintf(stderr, "no device\n"); return 2; }
    lamsa_hp_fm_index fx; memset(&fx, 0, sizeof fx);
    fx.seq_len = fm.seq_len; fx.primary = fm.primary; for (int c = 0; c < 5; ++c) fx.L2[c] = fm.L2[c];
    fx.bwt = fm.bwt.data(); fx.bwt_words = (uint64_t)fm.bwt.size() - 4; fx.sa = fm.sa.data(); fx.n_sa = fm.n_sa; fx.sa_intv = fm.sa_intv;
    const double tl = now_s();
    if (lamsa_hp_fm_load(h, &fx) != LAMSA_HP_OK) { fprintf(stderr, "lamsa_hp_fm_load: %s\n", lamsa_hp_last_error(h)); return 2; }
    printf("index: %llu symbols, sa_intv %llu, loaded to the device in %.3f s (%.2f GB); %d reads of %d bases: %lld seeds of %d every %d, max_hits %d\n", (unsigned long long)fm.seq_len,
           (unsigned long long)fm.sa_intv, now_s() - tl, (fm.bwt.size() * 4.0 + fm.sa.size() * 8.0) / 1e9, n, rlen, (long long)n * per, sl, ss, mh);
    std::vector<int64_t> read_off((size_t)n + 1, 0);
    for (int r = 0; r <= n; ++r) read_off[(size_t)r] = (int64_t)r * rlen;
    int bad_total = 0;
    for (const double err_rate : {0.01, 0.05, 0.12}) {
        std::mt19937_64 rng(4711);
        std::vector<uint8_t> seq((size_t)n * rlen + 16, 0);
        for (int r = 0; r < n; ++r) {
            const int64_t p = (int64_t)(rng() % (uint64_t)(ix.l_pac - rlen));
            const bool rev = r & 1;
            for (int i = 0; i < rlen; ++i) {
                const int64_t x = rev ? p + rlen - 1 - i : p + i;
                uint8_t b = ix.pac[(size_t)(x >> 2)] >> ((~x & 3) << 1) & 3;
                if (rev) b = (uint8_t)(3 - b);
                if ((double)(rng() >> 11) / 9007199254740992.0 < err_rate) b = (uint8_t)((b + 1 + rng() % 3) & 3);
                seq[(size_t)r * rlen + i] = b;
            }
        }
        lamsa_hp_seed_queries q; memset(&q, 0, sizeof q);
        q.n_reads = n; q.read_off = read_off.data(); q.read_seq = seq.data(); q.seed_len = sl; q.seed_step = ss; q.max_hits = mh;
        q.n_seqs = (int32_t)ix.off.size(); q.seq_offset = ix.off.data(); q.seq_len = ix.len.data();
        lamsa_hp_batch b; memset(&b, 0, sizeof b);
        printf("\nerror rate %.2f\n", err_rate);
        for (int rep = 0; rep < (err_rate < 0.02 ? 3 : 1); ++rep) {
            const double t2 = now_s();
            if (lamsa_hp_fm_seed(h, &q, &b) != LAMSA_HP_OK) { fprintf(stderr, "lamsa_hp_fm_seed: %s\n", lamsa_hp_last_error(h)); return 2; }
            const double w = now_s() - t2;
            printf("device call %d%s: %.3f s wall with copies (%.0f reads/s); HIP events: search + row scan %.3f ms, locate + compaction %.3f ms, slots + emit %.3f ms; %lld slots, %lld hits\n", rep,
                   rep == 0 && err_rate < 0.02 ? " (first: allocates)" : "", w, n / w, lamsa_hp_last_kernel_ms(h, 21), lamsa_hp_last_kernel_ms(h, 22), lamsa_hp_last_kernel_ms(h, 23),
                   (long long)b.seed_off[n], (long long)b.hit_off[b.seed_off[n]]);
        }
        long long with_hit = 0, few = 0;
        for (int64_t s = 0; s < b.seed_off[n]; ++s) with_hit += b.hit_off[s + 1] > b.hit_off[s];
        for (int r = 0; r < n; ++r) few += b.seed_off[r + 1] - b.seed_off[r] < 2;
        printf("seeds with at least one hit: %.4f; reads with fewer than two seeded slots: %.4f\n", (double)with_hit / ((double)n * per), (double)few / n);
        if (err_rate > 0.02) continue;

        // host: the same definition through the host index, a seed at a time, reads split over the threads
        std::vector<std::vector<Hit>> hh((size_t)threads); std::vector<std::vector<int32_t>> hslot((size_t)threads);      // per thread: hits, and (read, seed id, hits) per slot
        const int rper = (n + threads - 1) / threads;
        const double t0 = now_s();
        {
            std::vector<std::thread> th;
            for (int t = 0; t < threads; ++t) th.emplace_back([&, t]() {
                for (int r = t * rper; r < n && r < (t + 1) * rper; ++r)
                    for (int i = 0; i < per; ++i) {
                        uint64_t a = 0, l = fm.seq_len;
                        const uint64_t c = fm.match(sl, seq.data() + (size_t)r * rlen + (size_t)i * ss, &a, &l);
                        int kept = 0;
                        for (uint64_t m = a; c >= 1 && c <= (uint64_t)mh && m <= l; ++m) {
                            const int64_t p = (int64_t)fm.sa_at(m);
                            const bool is_rev = p >= ix.l_pac;
                            const int64_t f = is_rev ? 2 * ix.l_pac - 1 - p : p;
                            size_t lo = 0, hi = ix.off.size();
                            while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (ix.off[mid] <= f) lo = mid; else hi = mid; }
                            const int64_t sp = f - ix.off[lo] + 1 - (is_rev ? sl - 1 : 0);
                            if (sp < 1 || sp + sl - 1 > ix.len[lo]) continue;
                            hh[(size_t)t].push_back(Hit{sp, (int32_t)lo + 1, (int8_t)(is_rev ? -1 : 1)}); ++kept;
                        }
                        if (kept || c > (uint64_t)mh) { hslot[(size_t)t].push_back(r); hslot[(size_t)t].push_back(i + 1); hslot[(size_t)t].push_back(kept); }
                    }
            });
            for (auto &x : th) x.join();
        }
        const double host_s = now_s() - t0;
        size_t host_hits = 0; for (auto &v : hh) host_hits += v.size();
        printf("host: %d threads, %.3f s wall (%.0f reads/s; %lld seeds, %zu hits)\n", threads, host_s, n / host_s, (long long)n * per, host_hits);
        long long bad = 0; int64_t s = 0, k = 0;
        for (int t = 0; t < threads && !bad; ++t) {
            size_t x = 0;
            for (size_t j = 0; j + 2 < hslot[(size_t)t].size() + 0 && !bad; j += 3, ++s) {
                const int r = hslot[(size_t)t][j];
                bad += s >= b.seed_off[n] || s < b.seed_off[r] || s >= b.seed_off[r + 1] || b.seed_id[s] != hslot[(size_t)t][j + 1] || b.hit_off[s] != k || b.hit_off[s + 1] != k + hslot[(size_t)t][j + 2];
                for (int m = 0; m < hslot[(size_t)t][j + 2] && !bad; ++m, ++k, ++x) bad += b.h_pos[k] != hh[(size_t)t][x].pos || b.h_chr[k] != hh[(size_t)t][x].chr || b.h_strand[k] != hh[(size_t)t][x].strand;
            }
        }
        bad += s != b.seed_off[n] || k != b.hit_off[s];
        printf("answers: %s\n", bad ? "DIFFER" : "identical (slots, seed ids, hit records)");
        bad_total += bad != 0;
    }
    lamsa_hp_destroy(h);
    return bad_total ? 1 : 0;
}
