// fm_plan_check.cpp -- TEST INFRASTRUCTURE (tests/test_fm_cpu.py): the stage-4 planner of lamsa_amd/host from both seed sources -- the host
// FmIndex one query at a time (rescue_plan) and the answers of one lamsa_hp_fm_search (rescue_windows / rescue_plan_found; the call is
// tests/emu/emu_fm.cpp here) -- on reads made for the purpose.  A program of its own so that it can be built with
// -fsanitize=address,undefined and run directly.
// usage: fm_plan_check <index prefix> <cases>.  A case is a line "achr aoff schr soff len": the read is 200 reference bases of contig achr
// (1-based) from offset aoff, then len bases of contig schr from soff, then the 200 bases of achr that follow aoff + 200 + len; its two
// flanks are records of round 1, so the middle is an uncovered region with an anchor on either side.
// Prints "ok <regions> <lines> <jobs> <k-mers> <located>"; exit code 1 and the first difference when the two plans differ.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rescue.h"

using namespace lamsa;

static uint8_t base_at(const Index &ix, int chr, int64_t off) { const int64_t k = ix.off[(size_t)chr - 1] + off; return ix.pac[(size_t)(k >> 2)] >> ((~k & 3) << 1) & 3; }

#define SAME(a, b, what) do { if (!((a) == (b))) { printf("case %d: %s differs\n", ci, what); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: fm_plan_check <index prefix> <cases>\n"); return 2; }
    Index ix; FmIndex fm; std::string err;
    if (!load_index(argv[1], ix, err) || !fm.load(argv[1], err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
    lamsa_hp_para P; lamsa_hp_para_init(&P); lamsa_hp_para_finish(&P);
    lamsa_hp_handle *h = nullptr;
    if (lamsa_hp_create(&h, &P, nullptr, 0) != LAMSA_HP_OK) return 2;
    lamsa_hp_fm_index fx; memset(&fx, 0, sizeof fx);
    fx.seq_len = fm.seq_len; fx.primary = fm.primary; for (int c = 0; c < 5; ++c) fx.L2[c] = fm.L2[c];
    fx.bwt = fm.bwt.data(); fx.bwt_words = (uint64_t)fm.bwt.size() - 4; fx.sa = fm.sa.data(); fx.n_sa = fm.n_sa; fx.sa_intv = fm.sa_intv;
    if (lamsa_hp_fm_load(h, &fx) != LAMSA_HP_OK) { fprintf(stderr, "lamsa_hp_fm_load failed\n"); return 2; }

    FILE *fp = fopen(argv[2], "r");
    if (!fp) return 2;
    std::vector<std::vector<uint8_t>> reads; std::vector<ReadResult> RR;
    int achr, schr, len; long aoff, soff;
    while (fscanf(fp, "%d %ld %d %ld %d", &achr, &aoff, &schr, &soff, &len) == 5) {
        std::vector<uint8_t> rd;
        for (int i = 0; i < 200; ++i) rd.push_back(base_at(ix, achr, aoff + i));
        for (int i = 0; i < len; ++i) rd.push_back(base_at(ix, schr, soff + i));
        for (int i = 0; i < 200; ++i) rd.push_back(base_at(ix, achr, aoff + 200 + len + i));
        ReadResult R;
        Line la; la.tol_score = 400;
        Rec a; a.chr = achr; a.nstrand = 1; a.offset = aoff + 1; a.reg_beg = 1; a.reg_end = 200; a.cigar = {200 << 4, ((len + 200) << 4) | 4};
        Rec b; b.chr = achr; b.nstrand = 1; b.offset = aoff + 200 + len + 1; b.reg_beg = 201 + len; b.reg_end = 400 + len; b.cigar = {((200 + len) << 4) | 4, 200 << 4};
        la.rec.push_back(a); la.rec.push_back(b);
        R.stage[0].push_back(la);
        reads.push_back(rd); RR.push_back(R);
    }
    fclose(fp);

    const int n = (int)reads.size();
    std::vector<RescuePlan> host((size_t)n), dev((size_t)n);
    RescueJobs hj, dj; RescueWindows wins;
    for (int r = 0; r < n; ++r) rescue_plan(RR[(size_t)r], reads[(size_t)r].data(), (int)reads[(size_t)r].size(), ix, fm, P, host[(size_t)r], hj);
    for (int r = 0; r < n; ++r) rescue_windows(RR[(size_t)r], reads[(size_t)r].data(), (int)reads[(size_t)r].size(), P, dev[(size_t)r], wins);
    if (wins.win_off.empty()) wins.win_off.push_back(0);
    lamsa_hp_fm_queries q; memset(&q, 0, sizeof q);
    q.n_win = (int32_t)wins.win_off.size() - 1; q.seq = wins.seq.data(); q.seq_bytes = (int64_t)wins.seq.size(); q.win_off = wins.win_off.data(); q.k = P.bwt_seed_len; q.max_occ = 500;
    lamsa_hp_fm_out found; memset(&found, 0, sizeof found);
    if (lamsa_hp_fm_search(h, &q, &found) != LAMSA_HP_OK) { fprintf(stderr, "lamsa_hp_fm_search failed\n"); return 2; }
    for (int r = 0; r < n; ++r)
        if (!rescue_plan_found(reads[(size_t)r].data(), (int)reads[(size_t)r].size(), ix, found, 0, P, dev[(size_t)r], dj)) { printf("case %d: the answers do not fit the windows\n", r); return 1; }

    long n_regions = 0, n_lines = 0;
    for (int ci = 0; ci < n; ++ci) {
        const RescuePlan &A = host[(size_t)ci], &B = dev[(size_t)ci];
        SAME(A.regions.size(), B.regions.size(), "the number of regions");
        SAME(A.lines.size(), B.lines.size(), "the number of lines");
        SAME(A.region_of, B.region_of, "region_of");
        n_regions += (long)A.regions.size(); n_lines += (long)A.lines.size();
        for (size_t i = 0; i < A.lines.size(); ++i) {
            const RescueLine &x = A.lines[i], &y = B.lines[i];
            SAME(x.ref_id, y.ref_id, "ref_id"); SAME(x.is_rev, y.is_rev, "is_rev"); SAME(x.reg_beg, y.reg_beg, "reg_beg"); SAME(x.reg_len, y.reg_len, "reg_len");
            SAME(x.left.read_pos, y.left.read_pos, "left.read_pos"); SAME(x.left.ref_pos, y.left.ref_pos, "left.ref_pos");
            SAME(x.right.read_pos, y.right.read_pos, "right.read_pos"); SAME(x.right.ref_pos, y.right.ref_pos, "right.ref_pos");
            SAME(x.left_eta, y.left_eta, "left_eta"); SAME(x.right_eta, y.right_eta, "right_eta"); SAME(x.extra_beg, y.extra_beg, "extra_beg"); SAME(x.extra_end, y.extra_end, "extra_end");
            SAME(x.ref_start, y.ref_start, "ref_start"); SAME(x.ref_len, y.ref_len, "ref_len");
            SAME(x.query, y.query, "query"); SAME(x.target, y.target, "target"); SAME(x.lq, y.lq, "lq"); SAME(x.lt, y.lt, "lt");
            SAME(x.job_mid, y.job_mid, "job_mid"); SAME(x.job_left, y.job_left, "job_left"); SAME(x.job_right, y.job_right, "job_right");
            SAME(x.left_qlen, y.left_qlen, "left_qlen"); SAME(x.right_qlen, y.right_qlen, "right_qlen");
        }
    }
    { const int ci = -1;
      SAME(hj.seq, dj.seq, "job sequences"); SAME(hj.q_off, dj.q_off, "q_off"); SAME(hj.t_off, dj.t_off, "t_off"); SAME(hj.qlen, dj.qlen, "qlen"); SAME(hj.tlen, dj.tlen, "tlen");
      SAME(hj.kind, dj.kind, "kind"); SAME(hj.w, dj.w, "w"); SAME(hj.h0, dj.h0, "h0"); }
    printf("ok %ld %ld %ld %lld %lld\n", n_regions, n_lines, (long)hj.qlen.size(), (long long)found.n_kmers, (long long)found.pos_off[found.n_kmers]);
    lamsa_hp_destroy(h);
    return 0;
}
