// rescue.h -- stage (4) of the per-read pipeline: the BWT rescue of short read regions that rounds (2)/(3) and
// (2')/(3') left uncovered (reference src/bwt_aln.c).  Host work around the GPU's DP batch:
//   plan    (host threads)  uncovered regions of a read -> exact 19-mer hits through the FM index of the reference's
//                           <ref>.bwt / <ref>.sa -> seed chains -> per chain one global and two extension DP jobs
//   DP      (GPU)           all jobs of a chunk in one lamsa_hp_dp_batch() call (ksw_global2 / ksw_extend_core)
//   finish  (host threads)  CIGAR assembly, NM / AS, the read-type filter -> lines of a_res[2]
#pragma once
#include <string>
#include <vector>
#include "lamsa_host.h"

namespace lamsa {

// FM index in the reference's on-disk format (a BWA 0.7 .bwt with occurrence checkpoints every 128 symbols interleaved,
// and a sampled suffix array); bwt_restore_bwt / bwt_restore_sa, src/bwt.c:421-462
struct FmIndex {
    uint64_t primary = 0, L2[5] = {0, 0, 0, 0, 0}, seq_len = 0;
    std::vector<uint32_t> bwt;
    uint64_t sa_intv = 0, n_sa = 0;
    std::vector<uint64_t> sa;
    bool load(const std::string &prefix, std::string &err);
    uint64_t occ(uint64_t k, int c) const;                                   // bwt_occ :107
    uint64_t sa_at(uint64_t k) const;                                        // bwt_sa :86
    uint64_t match(int len, const uint8_t *s, uint64_t *k, uint64_t *l) const;   // bwt_match_exact_alt :241
};

struct RescueBound { int read_pos; int64_t ref_pos; };

// an uncovered read region beg .. end (1-based, inclusive) and the ends of the records next to it (get_remain_reg, src/lamsa_aln.c:583)
struct RescueAnchor { int is_rev, chr; int64_t pos; };
struct RescueRegion { int beg, end; std::vector<RescueAnchor> rb, re; };

struct RescueLine {                  // one seed chain that goes to bwt_aln_res (:200-303)
    int ref_id = 0, is_rev = 0, reg_beg = 0, reg_len = 0;
    RescueBound left, right;
    int left_eta = 0, right_eta = 0, extra_beg = 0, extra_end = 0;
    int64_t ref_start = 0; int ref_len = 0;
    std::vector<uint8_t> query, target, lq, lt;      // window of the read (strand of the hit), of the reference; reversed left flanks
    int job_mid = -1, job_left = -1, job_right = -1; // indices into the plan's job list (-1: no such extension)
    int left_qlen = 0, right_qlen = 0;
};

struct RescueJobs {                  // the DP jobs of a chunk, in lamsa_hp_dp_batch form
    std::vector<uint8_t> seq; std::vector<int64_t> q_off, t_off; std::vector<int32_t> qlen, tlen, kind, w, h0;
    int add(const uint8_t *q, int ql, const uint8_t *t, int tl, int kind_, int w_, int h0_);
};

struct RescuePlan {                  // of one read
    std::vector<RescueLine> lines;
    std::vector<int> region_of;      // region index of every line (lines of one region are consecutive)
    std::vector<int> job_base;       // unused by callers; kept for debugging
    std::vector<RescueRegion> regions;   // the read's uncovered regions, in order
    int64_t first_win = 0;           // --rescue-gpu: the window of regions[0] in the RescueWindows the read was listed into
};

// --rescue-gpu: the uncovered regions of many reads as the windows of one lamsa_hp_fm_search (one list per host thread)
struct RescueWindows { std::vector<uint8_t> seq; std::vector<int64_t> win_off; };

// plan: `bseq` = the read's base codes (0..4).  Jobs are appended to `jobs` (one job list per host thread).
void rescue_plan(const ReadResult &R, const uint8_t *bseq, int read_len, const Index &ix, const FmIndex &fm, const lamsa_hp_para &P, RescuePlan &plan, RescueJobs &jobs);

// The same plan in three steps, the search of all reads of a chunk in one call on the device between the two host steps:
//   rescue_windows     regions of the read -> plan.regions, one window per region appended to `wins`
//   lamsa_hp_fm_search (include/lamsa_hp.h) over the windows of the chunk, k = P.bwt_seed_len, max_occ = 5 * 100
//   rescue_plan_found  seeds -> chains -> jobs from the answers; win_base: where the windows of `wins` begin in the call's window list.
//                      false: the answers do not belong to these windows
// Both ways share the code that turns a seed's rows into hits, chains and jobs; the plans and the jobs are the same.
void rescue_windows(const ReadResult &R, const uint8_t *bseq, int read_len, const lamsa_hp_para &P, RescuePlan &plan, RescueWindows &wins);
bool rescue_plan_found(const uint8_t *bseq, int read_len, const Index &ix, const lamsa_hp_fm_out &found, int64_t win_base, const lamsa_hp_para &P, RescuePlan &plan, RescueJobs &jobs);

struct DpResults { const int32_t *score, *qle, *tle; const int64_t *cig_off; const int32_t *cigar; int64_t base; };   // base: first job of this thread's list

// lamsa_res_aux's walk over one record (src/frag_check.c:793-848): `rd` = the read's base codes on the record's strand (reverse
// complement for '-'), reference bases from the index's .pac.  Counts what NM and AS are made of and lists the record's mismatches in
// r.mm as the device does (ref_off << 2 | base, LAMSA_HP_TAG_MISMATCHES).  false: the CIGAR does not fit the read or the contig (the
// reference exits with "Unmatched length").
struct AuxCounts { int n_mm = 0, n_m = 0, n_io = 0, n_ie = 0, n_do = 0, n_de = 0; };
bool rec_aux(const Index &ix, const uint8_t *rd, int read_len, Rec &r, AuxCounts &k);

// What the host does to a record after the device (or stage 4) has made it, always in the order the device applies the items of
// lamsa_hp_set_result_tags in: gaps left-aligned (rec_left_align), mismatches listed and counted (rec_aux), =/X form (rec_to_eqx), summary.
enum { FIN_LEFT_ALIGN = 1, FIN_AUX = 2, FIN_EQX = 4, FIN_SUMMARY = 8 };
// the steps of `what` on one record; counts: what rec_aux counted.  false: rec_aux failed (the caller flags LAMSA_HP_ST_REFEXIT), no later step was made
bool rec_finish(Rec &r, const uint8_t *oriented_read, int read_len, const Index &ix, int what, AuxCounts *counts = nullptr);
// the read on a record's strand: bseq for '+', else its reverse complement, made in `rc` the first time a '-' record of the read asks
const uint8_t *oriented_read(const uint8_t *bseq, int read_len, int nstrand, std::vector<uint8_t> &rc);
// rec_finish on the records of rounds 1 and 2 of a read that has status 0
void read_finish(ReadResult &R, const uint8_t *bseq, int read_len, const Index &ix, int what);

// finish: DP results -> R.stage[2], every record through rec_finish(what | FIN_AUX): its score and NM come from that walk
void rescue_finish(ReadResult &R, const uint8_t *bseq, int read_len, const Index &ix, const lamsa_hp_para &P, RescuePlan &plan, const DpResults &dp, int what = 0);

}  // namespace lamsa
