// fm_gpu_ab.cpp -- one process that searches the same k-mer set twice: through the host FmIndex of lamsa_amd/host/rescue.cpp on N threads
// (what stage 4 does by default) and through lamsa_hp_fm_search on the GPU (--rescue-gpu).  tools/fm_gpu_ab.py builds the index and this
// program and writes profiles/fm_gpu_ab.txt from what it prints.
// usage: fm_gpu_ab <index prefix> <windows> <window length> <error rate> <threads>
// The windows are cut from the forward text at random places (seeded) and every base is replaced by another one with the error rate.
// Both sides answer the interval of every k-mer (k = 19) and the positions of those with 1 .. 500 rows; the answers are compared.
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

int main(int argc, char **argv)
{
    if (argc != 6) { fprintf(stderr, "usage: fm_gpu_ab <index prefix> <windows> <window length> <error rate> <threads>\n"); return 2; }
    const int n_win = atoi(argv[2]), wlen = atoi(argv[3]), threads = atoi(argv[5]), k = 19, max_occ = 500;
    const double err_rate = atof(argv[4]);
    Index ix; FmIndex fm; std::string err;
    if (!load_index(argv[1], ix, err) || !fm.load(argv[1], err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
    std::mt19937_64 rng(12345);
    std::vector<uint8_t> seq((size_t)n_win * wlen + 16, 0); std::vector<int64_t> win_off((size_t)n_win + 1, 0);
    for (int w = 0; w < n_win; ++w) {
        const int64_t p = (int64_t)(rng() % (uint64_t)(ix.l_pac - wlen));
        for (int i = 0; i < wlen; ++i) {
            const int64_t x = p + i;
            uint8_t b = ix.pac[(size_t)(x >> 2)] >> ((~x & 3) << 1) & 3;
            if ((double)(rng() >> 11) / 9007199254740992.0 < err_rate) b = (uint8_t)((b + 1 + rng() % 3) & 3);
            seq[(size_t)w * wlen + i] = b;
        }
        win_off[(size_t)w + 1] = (int64_t)(w + 1) * wlen;
    }
    const int per = wlen - k + 1; const int64_t n = (int64_t)n_win * per;
    printf("index: %llu symbols, sa_intv %llu; %d windows of %d bases, error rate %.3f: %lld %d-mers, max_occ %d\n", (unsigned long long)fm.seq_len, (unsigned long long)fm.sa_intv, n_win, wlen, err_rate, (long long)n, k, max_occ);

    // host: the planner's search, a k-mer at a time, windows split over the threads
    std::vector<uint64_t> hlo((size_t)n), hhi((size_t)n); std::vector<std::vector<uint64_t>> hpos((size_t)threads);
    const double t0 = now_s();
    {
        std::vector<std::thread> th;
        const int wper = (n_win + threads - 1) / threads;
        for (int t = 0; t < threads; ++t) th.emplace_back([&, t]() {
            for (int w = t * wper; w < n_win && w < (t + 1) * wper; ++w)
                for (int i = 0; i < per; ++i) {
                    uint64_t a = 0, l = fm.seq_len; const int64_t j = (int64_t)w * per + i;
                    const uint64_t c = fm.match(k, seq.data() + (size_t)w * wlen + i, &a, &l);
                    hlo[(size_t)j] = c ? a : 1; hhi[(size_t)j] = c ? l : 0;
                    if (c >= 1 && c <= (uint64_t)max_occ) for (uint64_t m = a; m <= l; ++m) hpos[(size_t)t].push_back(fm.sa_at(m));
                }
        });
        for (auto &x : th) x.join();
    }
    const double host_s = now_s() - t0;
    size_t host_located = 0; for (auto &v : hpos) host_located += v.size();
    printf("host: %d threads, %.3f s wall (%lld intervals, %zu rows located)\n", threads, host_s, (long long)n, host_located);

    lamsa_hp_para P; lamsa_hp_para_init(&P); lamsa_hp_para_finish(&P);
    lamsa_hp_handle *h = nullptr;
    if (lamsa_hp_create(&h, &P, nullptr, 0) != LAMSA_HP_OK) { fprintf(stderr, "no device\n"); return 2; }
    lamsa_hp_fm_index fx; memset(&fx, 0, sizeof fx);
    fx.seq_len = fm.seq_len; fx.primary = fm.primary; for (int c = 0; c < 5; ++c) fx.L2[c] = fm.L2[c];
    fx.bwt = fm.bwt.data(); fx.bwt_words = (uint64_t)fm.bwt.size() - 4; fx.sa = fm.sa.data(); fx.n_sa = fm.n_sa; fx.sa_intv = fm.sa_intv;
    const double t1 = now_s();
    if (lamsa_hp_fm_load(h, &fx) != LAMSA_HP_OK) { fprintf(stderr, "lamsa_hp_fm_load: %s\n", lamsa_hp_last_error(h)); return 2; }
    printf("device: index loaded in %.3f s (%.2f GB)\n", now_s() - t1, (fm.bwt.size() * 4.0 + fm.sa.size() * 8.0) / 1e9);
    lamsa_hp_fm_queries q; memset(&q, 0, sizeof q);
    q.n_win = n_win; q.seq = seq.data(); q.seq_bytes = (int64_t)seq.size(); q.win_off = win_off.data(); q.k = k; q.max_occ = max_occ;
    lamsa_hp_fm_out o; memset(&o, 0, sizeof o);
    for (int rep = 0; rep < 3; ++rep) {
        const double t2 = now_s();
        if (lamsa_hp_fm_search(h, &q, &o) != LAMSA_HP_OK) { fprintf(stderr, "lamsa_hp_fm_search: %s\n", lamsa_hp_last_error(h)); return 2; }
        printf("device call %d%s: %.3f s wall with copies; HIP events: k_fm_search %.3f ms, scan %.3f ms, k_fm_locate %.3f ms; %lld rows located\n", rep, rep == 0 ? " (first: allocates)" : "",
               now_s() - t2, lamsa_hp_last_kernel_ms(h, 21), lamsa_hp_last_kernel_ms(h, 23), lamsa_hp_last_kernel_ms(h, 22), (long long)o.pos_off[o.n_kmers]);
    }
    // the same answers?
    long long bad = o.n_kmers != n;
    for (int64_t j = 0; j < n && !bad; ++j) bad += o.lo[j] != hlo[(size_t)j] || o.hi[j] != hhi[(size_t)j];
    {
        const int wper = (n_win + threads - 1) / threads; int64_t at = 0;
        for (int t = 0; t < threads && !bad; ++t) {
            const int64_t j0 = (int64_t)std::min(n_win, t * wper) * per;
            bad += o.pos_off[j0] != at;
            for (size_t i = 0; i < hpos[(size_t)t].size() && !bad; ++i) bad += o.pos[at + (int64_t)i] != hpos[(size_t)t][i];
            at += (int64_t)hpos[(size_t)t].size();
        }
        bad += at != o.pos_off[o.n_kmers];
    }
    printf("answers: %s\n", bad ? "DIFFER" : "identical (intervals and positions)");
    lamsa_hp_destroy(h);
    return bad ? 1 : 0;
}
