/*
 * lamsa_hp.h -- C-ABI of the MI355X hot-path library (liblamsa_hp.so).
 *
 * This is the drop-in boundary for LAMSA's per-read seed-chain-extend path: the batch
 * form of the reference's per-read worker
 *     int lamsa_main_aln(thread_aux_t *aux)            reference src/lamsa_aln.c:825-891
 * which the reference calls once per thread over a chunk of reads
 * (src/lamsa_aln.c:1143-1162).  Stages (2) chaining, (3) gap-fill/extension and the
 * second round (2')/(3') run on the GPU behind lamsa_hp_align_batch(); seeding,
 * FASTA/FASTQ + GEM-map parsing, the BWT rescue (stage 4), result ranking and SAM
 * output stay with the host caller, exactly as SURVEY.md section 8(b) draws the line.
 * Two calls move work of the host side onto an FM index resident in HBM: lamsa_hp_fm_search (the exact search of stage 4) and
 * lamsa_hp_fm_seed (seeding itself, exact seeds, straight into the hit records of a lamsa_hp_batch; no mapper, no map text).
 *
 * Plain pointers and sizes only; every buffer handed in is caller-owned host memory,
 * every buffer handed out is callee-owned and valid until the next call on the same
 * handle (or lamsa_hp_destroy).  One handle per GPU; a handle is not thread-safe.
 * All entry points return 0 on success or a negative LAMSA_HP_E* code -- never exit(),
 * unlike the reference (src/frag_check.c:173, src/bntseq.c:471, ...).
 */
#ifndef LAMSA_HP_H
#define LAMSA_HP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LAMSA_HP_OK          0
#define LAMSA_HP_ENODEV     -1   /* no usable HIP device / HIP runtime error            */
#define LAMSA_HP_EINVAL     -2   /* malformed arguments                                  */
#define LAMSA_HP_ENOMEM     -3   /* device allocation failed                             */
#define LAMSA_HP_EKERNEL    -4   /* kernel launch / execution failure                    */

/* per-read / per-job status bits (out arrays) */
#define LAMSA_HP_ST_OVERFLOW   1  /* a device work buffer was too small; result invalid   */
#define LAMSA_HP_ST_REFEXIT    2  /* input on which the reference itself exit(1)s         */
#define LAMSA_HP_ST_UNSUPPORTED 4 /* the read is beyond what the device keeps (more than 32767 seeds, or a seed hit with
                                     |len_dif| > 127): not aligned, empty result; the rest of the batch is unaffected */

/* Alignment parameters after presets: the fields of the reference's lamsa_aln_para
 * (src/lamsa_aln.h:386-436) read on the hot path.  Fill with lamsa_hp_para_init() +
 * overrides + lamsa_hp_para_finish(), which mirror init_aln_para (src/lamsa_aln.c:1281),
 * lamsa_set_aln_mode (:1342) and lamsa_fill_mat (:1331). */
typedef struct lamsa_hp_para {
    int32_t seed_len, seed_step, seed_inv;
    int32_t per_aln_m, first_loci_thd;
    int32_t SV_len_thd, ske_max;
    float   ovlp_rat;
    int32_t bwt_seed_len, bwt_max_len, bwt_min_len;
    int32_t split_len, split_pen, res_mul_max;
    int32_t hash_len, hash_key_len, hash_step, hash_size;
    int32_t match_dis, mismatch_thd;
    int32_t ins_gapo, ins_gape, del_gapo, del_gape;      /* global DP   (ksw_global2)      */
    int32_t ins_ext_o, ins_ext_e, del_ext_o, del_ext_e;  /* extension DP (ksw_extend_core) */
    int32_t match, mis;
    int32_t band_w, end_bonus, zdrop;
    float   id_rate;
    int32_t read_type;   /* 0 default, 1 pacbio, 2 ont2d (-T) */
    int32_t aln_mode;    /* bit0 overlapping seeds, bit1 high indel error */
} lamsa_hp_para;

void lamsa_hp_para_init(lamsa_hp_para *p);
void lamsa_hp_para_finish(lamsa_hp_para *p);

/* Packed reference: the reference's .pac bytes (2 bit/base, base k at
 * pac[k>>2] >> ((~k&3)<<1) & 3, src/bntseq.c:242) plus the contig table of .ann
 * (bntann1_t.offset/.len, src/bntseq.h).  Replaces the (bntseq_t*, uint8_t *pac) pair
 * handed to every worker (src/lamsa_aln.c:1135). */
typedef struct lamsa_hp_ref {
    const uint8_t *pac;       /* l_pac/4+1 bytes */
    int64_t        l_pac;
    int32_t        n_seqs;
    const int64_t *seq_offset;/* [n_seqs] */
    const int32_t *seq_len;   /* [n_seqs] */
} lamsa_hp_ref;

typedef struct lamsa_hp_handle lamsa_hp_handle;

/* Replaces aux_dp_init + the index hand-over of lamsa_aln_core (src/lamsa_aln.c:969-984,
 * 1130-1137): uploads parameters and the packed reference to HBM of `device_id`. */
int  lamsa_hp_create(lamsa_hp_handle **out, const lamsa_hp_para *para, const lamsa_hp_ref *ref, int device_id);
void lamsa_hp_destroy(lamsa_hp_handle *h);
const char *lamsa_hp_last_error(const lamsa_hp_handle *h);

/* ------------------------------------------------------------------------------------
 * Batched banded affine-gap DP primitives:
 *   kind 0: ksw_global2      src/ksw.c:543   (global gap penalties, band w)
 *   kind 1: ksw_extend_core  src/ksw.c:667   (extension gap penalties, band w, h0)
 *   kind 2: ksw_bi_extend    src/ksw.c:862   (lh0 = rh0 = h0; w ignored)
 *   kind 4, 5, 6: the same three by the one-job-per-lane routines the read path runs its small jobs on (queries up to 160, targets up
 *           to 256 bases without N).  When the handle's penalties do not keep 16-bit cells exact these kinds run on the routines of
 *           kinds 0-2, as the read path does.
 *   kind 8 .. 11: a job as the read path's wave-per-job launch runs it (targets without N): 8 = a junction's ksw_bi_extend (kind 2),
 *           9 = a seed gap's ksw_global2 (kind 0), 10 / 11 = a line's head / tail extension -- ksw_extend_r (src/ksw.c:820) /
 *           ksw_extend_c (:809) with (w, h0); unless the query was consumed the rest of it is appended as a soft clip, and the head's
 *           CIGAR is turned round (frag_head_bound_fix / frag_tail_bound_fix, src/frag_check.c:640-648, :699-703); score / qle / tle
 *           are the extension's.
 *   kind 12, 13: a job as the read path's lane launches run it, listed into their queues and run stage by stage (queries of 1 .. 64 and
 *           targets of up to 160 bases without N; the handle's penalties must fit the lane routines): 12 = a junction's
 *           ksw_bi_extend(100, 100), 13 = a seed gap's ksw_global2(band_w); w and h0 are not read.  status 0 = the CIGAR was left for the
 *           fill to pick up (1: the fill would run the job itself), qle = DP cells charged to the job, tle = 1 when the job went through
 *           a hard queue (the second stage), score 0.
 *   One class (0-2, 4-6, 8-11, 12-13) per call.
 * Sequences are 1 byte/base codes 0..4; job i uses query seq[q_off[i] .. q_off[i]+qlen[i])
 * and target seq[t_off[i] .. t_off[i]+tlen[i]).
 * ---------------------------------------------------------------------------------- */
typedef struct lamsa_hp_dp_jobs {
    int32_t        n_jobs;
    const uint8_t *seq;  int64_t seq_bytes;
    const int64_t *q_off; const int32_t *qlen;
    const int64_t *t_off; const int32_t *tlen;
    const int32_t *kind, *w, *h0;
} lamsa_hp_dp_jobs;

typedef struct lamsa_hp_dp_out {       /* callee-owned, valid until the next call */
    const int32_t *score;              /* kind 0/1 (4/5, 9-11): DP score; kind 2 (6, 8): return flag */
    const int32_t *qle, *tle;          /* kind 1 (5, 10, 11) only                 */
    const int32_t *status;             /* LAMSA_HP_ST_* bits                      */
    const int64_t *cig_off;            /* [n_jobs+1] into cigar[]                 */
    const int32_t *cigar;              /* len<<4|op words, ops MIDNSH as in SAM   */
} lamsa_hp_dp_out;

int lamsa_hp_dp_batch(lamsa_hp_handle *h, const lamsa_hp_dp_jobs *jobs, lamsa_hp_dp_out *out);


/* ------------------------------------------------------------------------------------
 * The hot path proper: stages (2) sparse-DP chaining (frag_line_BCC, src/lamsa_dp_con.c:1305),
 * (3) gap-fill / split extension (frag_check, src/frag_check.c:856), and the second round
 * (2')/(3') on the read regions left uncovered (frag_line_remain :1252), for a batch of reads.
 * Replaces the loop body of lamsa_main_aln (src/lamsa_aln.c:857-871) for every read of a
 * chunk; the inputs are what the reference keeps in lamsa_seq_t / map_msg / map_t
 * (src/lamsa_aln.c:782-795, src/lamsa_aln.h:230-245), laid out as struct-of-arrays.
 * ---------------------------------------------------------------------------------- */
typedef struct lamsa_hp_batch {
    int32_t        n_reads;
    const int64_t *read_off;   /* [n_reads+1] into read_seq                                  */
    const uint8_t *read_seq;   /* 1 byte/base codes 0..4 (nst_nt4_table, src/bntseq.c:20)    */
    const int32_t *seed_all;   /* [n_reads] number of seeds of the read (APP->seed_all)      */
    const int32_t *last_len;   /* [n_reads] APP->last_len                                    */
    const int64_t *seed_off;   /* [n_reads+1]: read r owns seed slots [seed_off[r], seed_off[r+1]) = m_msg[0..seed_out) */
    const int32_t *seed_id;    /* [n_slots] 1-based seed index (map_msg.seed_id)             */
    const int64_t *hit_off;    /* [n_slots+1]: slot s owns hits [hit_off[s], hit_off[s+1]) = map[0..map_n) */
    const int64_t *h_pos;      /* [n_hits] map_t.offset (1-based leftmost reference coord)   */
    const int32_t *h_chr;      /* map_t.nchr (1-based contig id)                             */
    const int8_t  *h_strand;   /* map_t.nstrand (+1 / -1)                                    */
    const int16_t *h_nm;       /* map_t.NM                                                   */
    const int16_t *h_len_dif;  /* map_t.len_dif                                              */
    const int32_t *h_cig_off;  /* start of the seed CIGAR in cig[] / cig8[]; NULL: the CIGARs lie back to back in hit order
                                  (offset = sum of h_cig_n of the hits before; no 2^31 limit on n_cig then)           */
    const uint8_t *h_cig_n;    /* its length in elements                                     */
    const int32_t *cig;        /* seed CIGAR words, len << 4 | op (already reversed for '-' hits, src/gem_parse.c:267) */
    int64_t        n_cig;      /* elements in cig[] / cig8[]                                 */
    const uint8_t *cig8;       /* optional, instead of cig[]: one BYTE per element, op << 6 | len, op 0 M / 1 I / 2 D, len <= 63
                                  (a seed is seed_len = 50 bases: src/lamsa_aln.h:44) -- a quarter of the bytes over PCIe */
} lamsa_hp_batch;

/* Results: one int32 stream per read (callee-owned, valid until the next call):
 *   [0] status bits (LAMSA_HP_ST_*)  [1] lines of round 1 (a_res[0].l_n)  [2] lines of round 2 (a_res[1].l_n)
 *   per line : line_score, tol_score, tol_NM, n_res (= cur_res_n+1, 0 when every record was dropped)
 *   per res  : offset_lo, offset_hi, chr, nstrand (1 '+', 0 '-'), score (AS), NM, cigar_n, cigar words...
 *              and, only with LAMSA_HP_TAG_MISMATCHES set (lamsa_hp_set_result_tags), after the CIGAR words:
 *              n_mm, then n_mm words ref_off << 2 | base, ref_off ascending
 *              With LAMSA_HP_TAG_EQX set, cigar_n and the CIGAR words are the =/X form (below); no other word changes.
 * i.e. the fields of line_aln_res / res_t (src/frag_check.h:46-73) that aln_res_output and
 * rearr_aln_res consume.  A mismatch word names one aligned base that differs from the reference: ref_off is its
 * 0-based offset from the record's offset (POS) on the forward reference, base the .pac code (0-3) of the reference
 * base there.  A read N (code 4) is a mismatch, as it is for NM; so NM = n_mm + inserted + deleted bases.
 * The =/X form of a CIGAR (ops numbered as in SAM: '=' is 7, 'X' is 8): every M element is replaced, on its own, by its
 * pieces -- the maximal runs of aligned bases that equal the reference ('=') or differ from it ('X'; a read N differs).
 * The pieces are in order, none is empty, neighbours alternate; every other element is copied as it is, and pieces never
 * merge across elements ("..1X 2I 1X.." stays three elements).  So the X lengths of a record sum to its n_mm, the pieces
 * of one element with 7/8 read as 0 add up to the original word, and a record has at most cigar_n + 2 n_mm words.
 * With LAMSA_HP_TAG_LEFT_ALIGN set, the gaps of every record are left-aligned before anything is counted.  The definition
 * is this procedure on one record: op[0..n), len[0..n) its CIGAR in M form; R the read on the record's strand (as SEQ is
 * printed, soft clips included), compared by base code 0-4, so N equals N; T the forward reference from the record's
 * offset, compared by .pac code:
 *     for i = 0 .. n-1, ascending:
 *         if op[i] in {I, D} and 0 < i < n-1 and op[i-1] == M and op[i+1] == M:
 *             k = len[i]; q = read position of element i; p = reference position of element i
 *             while len[i-1] > 1 and ( op[i] == D ? T[p-1] == T[p+k-1] : R[q-1] == R[q+k-1] ):
 *                 len[i-1] -= 1; len[i+1] += 1; p -= 1; q -= 1
 * Only M lengths change: the element count, the order of the ops, the clips, the offset, the read and reference spans,
 * NM, AS, the line totals and the number of mismatches are what they were, and a second application changes nothing.
 * A gap never consumes the M before it, so it never merges with or crosses another gap or a clip and never reaches the
 * record's start; a gap that touches another gap or a clip stays and stops its neighbours.  A mismatch inside a stretch
 * that a deletion of k bases moved across keeps its base and gets ref_off + k.  Gaps are not right-aligned or merged, and
 * where the records of a line meet is not touched.  The mismatch lists and the =/X form describe the shifted alignment.
 * With LAMSA_HP_TAG_SUMMARY set, a record is exactly 15 words and no CIGAR word follows cigar_n:
 *     offset_lo, offset_hi, chr, nstrand, score, NM, cigar_n,
 *     q_beg, q_end, ref_span, m_bases, ins_bases, del_bases, ins_runs, del_runs
 * cigar_n is the element count of the record's M-form CIGAR, the one the stream ships without the item, and the eight
 * words behind it are defined on that CIGAR: q_beg .. q_end the covered read interval, 1-based and inclusive, on the
 * read as given (a '+' record: leading S + 1 .. read length - trailing S; a '-' record: the two clips swapped; an
 * empty CIGAR: 1 .. read length); ref_span the sum of the M and D lengths; m_bases, ins_bases, del_bases the sums of
 * the M / I / D lengths; ins_runs, del_runs the numbers of I / D elements (an I next to a D is two runs).  For every
 * record the device makes, n_mm = NM - ins_bases - del_bases >= 0 is its number of mismatches and
 *     score = (m_bases - n_mm) * match - n_mm * mis - ins_runs * ins_gapo - ins_bases * ins_gape
 *             - del_runs * del_gapo - del_bases * del_gape.
 * Line headers, the per-read header and the status are what they are without the item.  It is what a PAF
 * line needs, without the CIGAR words. */
typedef struct lamsa_hp_result {
    const int32_t *stream; int64_t stream_words;
    const int64_t *read_off;      /* [n_reads] start of read r's stream */
    const int32_t *read_len;      /* [n_reads] its length in words      */
    const int32_t *read_status;   /* [n_reads] LAMSA_HP_ST_* bits       */
    const int32_t *read_tbases;   /* [n_reads] reference bases the read's DP jobs fetched from the packed reference (accounting) */
    const int32_t *read_work;     /* [4*n_reads] per read: DP cells updated, chaining edge classes evaluated, seed-CIGAR words read by the gap fill, 0
                                     (accounting: GCUPS, pair evaluations/s, the algorithmic bytes of the fill launches) */
} lamsa_hp_result;

int lamsa_hp_align_batch(lamsa_hp_handle *h, const lamsa_hp_batch *batch, lamsa_hp_result *res);

/* Optional items of the result stream (lamsa_hp_result), for the batches aligned after the call; 0 (the default) is the
 * stream as documented without them.  LAMSA_HP_TAG_MISMATCHES: every record also lists its mismatches (what a SAM
 * writer needs for MD:Z without reading the reference again).  LAMSA_HP_TAG_EQX: the CIGARs are in =/X form (the
 * device splits the M elements by the same lists, which are in the stream only if LAMSA_HP_TAG_MISMATCHES is set too).
 * LAMSA_HP_TAG_LEFT_ALIGN: the gaps of every CIGAR are left-aligned (the device shifts them before it counts; no word
 * is added).  These three combine freely.  LAMSA_HP_TAG_SUMMARY: every record is its fixed 15-word summary in place
 * of its CIGAR (above).  With LAMSA_HP_TAG_MISMATCHES or LAMSA_HP_TAG_EQX it is LAMSA_HP_EINVAL (there is nothing to
 * list or split); with LAMSA_HP_TAG_LEFT_ALIGN it is accepted and the stream is word for word that of
 * LAMSA_HP_TAG_SUMMARY alone, since left alignment changes M lengths only (the device skips the shift).  Flags outside
 * the four (4, 16 and 64 among them): LAMSA_HP_EINVAL; so while a batch or run is in flight. */
#define LAMSA_HP_TAG_MISMATCHES 1
#define LAMSA_HP_TAG_EQX 2
#define LAMSA_HP_TAG_LEFT_ALIGN 8
#define LAMSA_HP_TAG_SUMMARY 32
int lamsa_hp_set_result_tags(lamsa_hp_handle *h, int flags);

/* The same in two steps, so that a caller can keep a batch resident in HBM and overlap or
 * repeat the compute: upload copies the batch to the device, run aligns the resident batch
 * (res may be NULL: results stay on the device and are not fetched). */
int lamsa_hp_upload_batch(lamsa_hp_handle *h, const lamsa_hp_batch *batch);
int lamsa_hp_run_uploaded(lamsa_hp_handle *h, lamsa_hp_result *res);
/* run_uploaded in two halves, two runs deep: start queues a run of the resident batch and returns; finish waits for
 * the oldest run and fetches its results (res may be NULL).  The second run's waves start as the first one's drain. */
int lamsa_hp_start_uploaded(lamsa_hp_handle *h);
int lamsa_hp_finish_uploaded(lamsa_hp_handle *h, lamsa_hp_result *res);

/* The streaming form, for the chunk loop of lamsa_aln_core (src/lamsa_aln.c:1140-1170): the reference overlaps nothing
 * (read chunk -> threads -> join -> print); here up to two chunks are in flight per handle.
 *   submit   validates the batch, copies it to the device on the copy stream -- while the kernel of the previously
 *            submitted batch is still running -- and queues its kernel behind that one.  It returns when the copy is
 *            done (the caller's arrays may be reused) without waiting for any kernel.  LAMSA_HP_EINVAL when two
 *            batches are already in flight.
 *   collect  waits for the OLDEST submitted batch, runs its second pass if a read needs one and fetches the results
 *            (callee-owned, valid until the next collect / run on this handle).  lamsa_hp_last_kernel_ms() then
 *            refers to that batch.  LAMSA_HP_EINVAL when nothing is in flight.
 * Loop of a streaming caller:  submit(B0); for i = 1..: prepare B_i; submit(B_i); collect(R_{i-1}); write R_{i-1}.
 * lamsa_hp_upload_batch / run_uploaded / align_batch must not be called while a submitted batch is in flight. */
int lamsa_hp_submit_batch(lamsa_hp_handle *h, const lamsa_hp_batch *batch);
int lamsa_hp_collect_batch(lamsa_hp_handle *h, lamsa_hp_result *res);

/* Optional: allocate now, for both batches that can be in flight, what batches within the given bounds will need on the device
 * (scratch, inter-launch state, input and output buffers) instead of inside the first submit / align call, where allocations of
 * tens of GB cost seconds.  A caller that knows its chunk size calls it once after lamsa_hp_create -- from a thread of its own if it
 * has input to read meanwhile (the handle must not be used concurrently).  Batches beyond the bounds still work; they allocate. */
int lamsa_hp_reserve(lamsa_hp_handle *h, int32_t n_reads, int64_t n_bases, int64_t n_hits, int64_t n_cig, int32_t max_read_len, int32_t max_hits_per_read);

/* Page-locked host memory for the arrays of a lamsa_hp_batch: copies from it run at the full PCIe rate and need no
 * staging pass through the runtime's bounce buffers.  Optional -- ordinary memory works everywhere. */
void *lamsa_hp_host_alloc(size_t bytes);
void  lamsa_hp_host_free(void *p);

/* Wall time in milliseconds of the kernel(s) of the most recent call on this handle (for the streaming form: of the
 * batch just collected), measured with HIP events on the stream the kernels ran on; which = 0: the main pass,
 * 1: the second pass over the reads that overflowed their scratch (0 when none did); 2..6: the five launches the main
 * pass consists of (chaining round 1, gap fill of its lines, chaining round 2, gap fill of its lines, result assembly); 7..10: how long each of the first four spent draining (first wave
 * that found the queue empty -> last wave done, i.e. time with idle wave slots); 11, 12: lines filled in round 1 / round 2; 13: of "gap fill, round 1"
 * the part before the fill launch proper (job listing + the two DP launches), 14: the listing, 15: the wave-per-job DP launch; 16: wave jobs listed,
 * 17: their algorithmic bytes (MB: sequences read, CIGARs written), 18: lane jobs listed, 19: MB of CIGARs computed ahead of the fill, 20: DP cells the wave jobs
 * updated (millions). */
float lamsa_hp_last_kernel_ms(const lamsa_hp_handle *h, int which);

/* Cap the per-wave scratch slab of the first pass at `bytes` (0 = size it from the batch, the default).  The slab
 * replaces the reference's per-thread malloc/realloc arenas (src/lamsa_aln.c:960-990, src/frag_check.h:142-146);
 * a read that does not fit is not truncated: it is flagged and re-run by the second pass with 8x capacities, as
 * always.  For memory-constrained devices and for testing that second pass. */
int lamsa_hp_set_scratch_limit(lamsa_hp_handle *h, size_t bytes);

/* ------------------------------------------------------------------------------------
 * The FM index of the reference's <ref>.bwt / <ref>.sa resident in HBM, and the batched exact search of k-mers in it: what
 * bwt_match_exact_alt (src/bwt.c:241) and bwt_sa (:86) answer one call at a time, for a caller that has its seeds in a batch
 * (stage 4, src/bwt_aln.c:316-363, is one).  The index is the text "forward reference + its reverse complement" of seq_len
 * symbols; row 0 is the sentinel suffix, row r >= 1 the r-th smallest suffix, primary the row of suffix 0.
 *   bwt, bwt_words   the words of <ref>.bwt behind its 40-byte header (blocks of 16: four 64-bit counts, 128 two-bit symbols);
 *                    at least (seq_len + 15) / 16 + (seq_len + 127) / 128 * 8 of them
 *   L2               L2[0] = 0 and the four cumulative counts of the header; L2[4] = seq_len
 *   sa, n_sa         n_sa = (seq_len + sa_intv) / sa_intv samples, sa[j] the text position of row j * sa_intv: sa[0] = (uint64_t)-1
 *                    (bwt_restore_sa, :440), then the values of <ref>.sa behind its 56-byte header; sa_intv a power of two
 * lamsa_hp_fm_load copies the index to the device; it replaces an index loaded earlier and lamsa_hp_destroy frees it.  After a
 * failed load the handle holds no index.  A handle created without a reference takes both calls.
 * ---------------------------------------------------------------------------------- */
typedef struct lamsa_hp_fm_index { uint64_t seq_len, primary, L2[5]; const uint32_t *bwt; uint64_t bwt_words;
                                   const uint64_t *sa; uint64_t n_sa, sa_intv; } lamsa_hp_fm_index;
int lamsa_hp_fm_load(lamsa_hp_handle *h, const lamsa_hp_fm_index *ix);
/* Queries: window w holds base codes 0..4 at seq[win_off[w] .. win_off[w+1]); its k-mers are all len - k + 1 overlapping ones in
 * order (none when the window is shorter than k), so k-mer j of the call is the (j - kmer_off[w])-th of its window.
 * Results (callee-owned, valid until the next lamsa_hp_fm_search on the handle): lo[j] .. hi[j] the inclusive row interval of
 * k-mer j, lo = 1, hi = 0 when it does not occur or holds a code above 3; for a k-mer with 1 <= hi - lo + 1 <= max_occ,
 * pos[pos_off[j] + i] is the suffix-array value of row lo + i (a coordinate in the doubled text; strand, contig and bounds are the
 * caller's), every other k-mer has none (pos_off[j + 1] == pos_off[j]).  max_occ = 0: intervals only.
 * LAMSA_HP_EINVAL: no index loaded, k outside 1..255, max_occ outside 0..2^20, offsets that decrease or leave seq_bytes.
 * The call blocks.  The device buffer for the positions is bounded: they are located and fetched in slices.
 * lamsa_hp_last_kernel_ms 21 / 22 / 23: the search kernel, the locate kernel (all slices), the scan between them. */
typedef struct lamsa_hp_fm_queries { int32_t n_win; const uint8_t *seq; int64_t seq_bytes; const int64_t *win_off; /* [n_win+1] */
                                     int32_t k, max_occ; } lamsa_hp_fm_queries;
typedef struct lamsa_hp_fm_out { int64_t n_kmers; const int64_t *kmer_off; /* [n_win+1] */ const uint64_t *lo, *hi; /* [n_kmers] */
                                 const int64_t *pos_off; /* [n_kmers+1] */ const uint64_t *pos; } lamsa_hp_fm_out;
int lamsa_hp_fm_search(lamsa_hp_handle *h, const lamsa_hp_fm_queries *q, lamsa_hp_fm_out *out);

/* ------------------------------------------------------------------------------------
 * Seeding in the resident index: the seeds of a batch of reads are cut, searched exactly and located on the device, and come back as
 * the hit records of a lamsa_hp_batch -- what split_seed (src/lamsa_aln.c:252), the GEM mapper and gem_map_msg (src/gem_parse.c) make
 * together, for exact hits only.  No mapper, no seed file, no map text.  The definition:
 *   Inputs: the reads (read_off / read_seq as in lamsa_hp_batch, codes 0..4); seed_len (1..63), seed_step (>= 1), max_hits (1..16383);
 *   the contig table (n_seqs, seq_offset, seq_len as in lamsa_hp_ref); the index loaded on the handle, whose text is the forward
 *   reference followed by its reverse complement, seq_len = 2 * l_pac.
 *   Per read of length L:  seed_all = L < seed_len ? 0 : 1 + (L - seed_len) / seed_step;
 *                          last_len = L - seed_len - (seed_all - 1) * seed_step  (what lamsa_hp_align_batch checks);
 *   seed i (1-based) is read[(i-1) * seed_step .. + seed_len).  Let n be the number of rows of the seed's interval
 *   (bwt_match_exact_alt from the whole index); n = 0 when a base code is above 3.
 *     n = 0:          the seed gets no slot.
 *     n > max_hits:   the seed keeps its slot (seed_id = i) with no hits, as gem_map_msg does for a line with more than per_aln_m hits
 *                     (src/gem_parse.c:243-246).
 *     otherwise, for the rows in ascending row order: p = the row's text position (bwt_sa); is_rev = p >= l_pac;
 *                     f = is_rev ? 2 * l_pac - 1 - p : p;  c = the contig that holds f (bns_pos2rid);
 *                     pos = f - seq_offset[c] + 1 - (is_rev ? seed_len - 1 : 0);
 *                     the row is kept iff pos >= 1 and pos + seed_len - 1 <= seq_len[c]  (an occurrence across a contig boundary, across
 *                     the middle of the doubled text, or -- on '-' -- beginning in the contig before, is none);
 *                     a kept row is the hit h_pos = pos, h_chr = c + 1, h_strand = is_rev ? -1 : +1, h_nm = 0, h_len_dif = 0,
 *                     CIGAR "seed_len M".  If no row is kept, the seed gets no slot.
 *   Hits of a slot stay in row order, slots in seed order, reads in input order.
 * Where the FASTA had N the .pac holds substituted bases, and a seed may hit there; filtering by <ref>.amb is the caller's.
 * `out` is a complete lamsa_hp_batch in the compact form: h_cig_off = NULL, cig = NULL, cig8 one byte per hit, n_cig = the number of
 * hits.  read_off / read_seq are the caller's arrays; everything else is callee-owned and valid until the next lamsa_hp_fm_seed on the
 * handle.  Every pointer is non-null, also for zero reads or zero hits.  It can be handed to lamsa_hp_align_batch /
 * lamsa_hp_submit_batch of any handle created with seed_len, seed_step and that reference.
 * LAMSA_HP_EINVAL: no index loaded; seed_len outside 1..63, seed_step < 1, max_hits outside 1..16383; offsets that do not start at 0 or
 * that decrease; a read longer than 2^24; a base code above 4; a contig table that is empty, not contiguous, or whose end is not the
 * index's seq_len / 2 (the index of another genome).  LAMSA_HP_ENOMEM as elsewhere; the handle stays usable after every error.
 * The call blocks and shares its device buffers with lamsa_hp_fm_search.  Rows are located LAMSA_HP_FM_SLICE (default 2^22) at a time
 * and a slice's hits fetched before the next is located, so the device buffers are bounded by the slice and by the number of seeds; the
 * hits travel once, 13 bytes each (position, contig, strand); what is the same for every exact hit is filled in on the host.
 * Exact seeds suit accurate reads: a 50-mer survives 1 % error with probability 0.61, 5 % with 0.08.
 * lamsa_hp_last_kernel_ms 21 / 22 / 23 after this call: search + scan of the row counts, locate + compaction of all slices, slots + emit.
 * ---------------------------------------------------------------------------------- */
typedef struct lamsa_hp_seed_queries {
    int32_t n_reads; const int64_t *read_off; const uint8_t *read_seq;
    int32_t seed_len, seed_step, max_hits;
    int32_t n_seqs; const int64_t *seq_offset; const int32_t *seq_len;
} lamsa_hp_seed_queries;
int lamsa_hp_fm_seed(lamsa_hp_handle *h, const lamsa_hp_seed_queries *q, lamsa_hp_batch *out);

#ifdef __cplusplus
}
#endif
#endif
