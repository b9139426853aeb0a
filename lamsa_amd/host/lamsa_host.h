// lamsa_host.h -- host side of `lamsa aln` (see lamsa_host.cpp).  Plain C++17; talks to the GPU only through
// the C-ABI of include/lamsa_hp.h.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../include/lamsa_hp.h"

namespace lamsa {

struct Index {                       // .ann contig table + .pac (src/bntseq.h bntseq_t, the parts the path reads)
    std::vector<std::string> name; std::vector<int64_t> off; std::vector<int32_t> len;
    std::vector<uint8_t> pac; int64_t l_pac = 0;
    std::map<std::string, int> name_to_id;
};
bool load_index(const std::string &prefix, Index &ix, std::string &err);

struct Read { std::string name, seq, qual; bool has_qual = false; };

class FastxReader {
  public:
    struct Impl;
    FastxReader(); ~FastxReader();
    bool open(const std::string &path);
    bool next(Read &r);
    // Sharding (--shard i/N).  A mapped (uncompressed, regular) file is cut by bytes: restrict(lo, hi) makes next() deliver the records
    // that START in [lo, hi) of the file; other inputs are cut by record count (count the records with next(), re-open, skip).
    bool mapped() const; size_t size() const;
    void restrict(size_t lo, size_t hi);
    // A mapped FASTA file (first byte '>') can hand out its records as byte spans -- two line searches per single-line record -- and
    // have them parsed later, on any thread: next_span() delivers the next record's [beg, end) (false at the end, or when the file
    // is not a mapped FASTA file), parse_span() is next() on that span.
    bool spans() const;
    bool next_span(size_t &beg, size_t &end);
    bool parse_span(size_t beg, size_t end, Read &r) const;
  private:
    Impl *p;
};

// vector whose resize() leaves new elements uninitialised: the batch arrays are sized once per chunk and then filled
// by all host threads, and a chunk's buffers are recycled, so nothing is ever zero-filled or page-faulted twice
template <class T> struct NoInitAlloc : std::allocator<T> {
    template <class U> struct rebind { typedef NoInitAlloc<U> other; };
    template <class U> void construct(U *p) noexcept { ::new ((void *)p) U; }
    template <class U, class... A> void construct(U *p, A &&... a) { ::new ((void *)p) U(std::forward<A>(a)...); }
};
template <class T> using RawVec = std::vector<T, NoInitAlloc<T>>;

struct Batch {                       // the arrays of lamsa_hp_batch, host side
    std::vector<Read> reads;
    RawVec<int64_t> read_off, seed_off, hit_off, h_pos;
    RawVec<uint8_t> read_seq, h_cig_n, cig8;      // cig8: the seed CIGARs as the GPU boundary's compact form takes them (op << 6 | len)
    bool cig_wide = false;                        // some element is longer than 63: the chunk goes in the word form (cig + h_cig_off)
    bool parse_compact = false, saw_wide = false; // a per-thread part of the parse: the seed CIGARs written as bytes (cig8) straight away; an element that does not fit was met
    RawVec<int32_t> seed_all, last_len, seed_id, h_chr, h_cig_off, cig;
    RawVec<int16_t> h_nm, h_len_dif;
    RawVec<int8_t> h_strand;
    void clear();
};

// cigar: M form, or with --eqx the =/X form (ops 7 / 8): every routine that walks it takes 0, 7 and 8 alike, as read and reference bases
inline bool cig_aligned(int op) { return op == 0 || op == 7 || op == 8; }      // M, =, X: read and reference bases facing each other
struct Rec { int64_t offset = 0; int chr = 0, nstrand = 0, score = 0, NM = 0, reg_beg = 0, reg_end = 0; std::vector<int32_t> cigar;   // res_t
             std::vector<int32_t> mm;        // --MD, --cs: the mismatches, ref_off << 2 | base (include/lamsa_hp.h, LAMSA_HP_TAG_MISMATCHES)
             // --paf, --paf-cg: the record's summary (LAMSA_HP_TAG_SUMMARY, include/lamsa_hp.h; q_beg / q_end are reg_beg / reg_end), from the
             // stream's 15-word record -- the CIGAR is empty then -- or from the CIGAR (rec_summary); summed: the six are set
             bool summed = false; int ref_span = 0, m_bases = 0, ins_bases = 0, del_bases = 0, ins_runs = 0, del_runs = 0; };
struct XaRef { int st, li, ri; };
struct Line { int line_score = 0, tol_score = 0, tol_NM = 0, merg_x = 0, merg_y = 0; uint8_t mapQ = 0; std::vector<Rec> rec; std::vector<XaRef> xa; };   // line_aln_res
struct ReadResult { int status = 0; std::vector<Line> stage[3]; };   // aln_res[3]: first round, remain round, BWT rescue (empty)

// tags: what lamsa_hp_set_result_tags was given.  LAMSA_HP_TAG_MISMATCHES: the stream carries the records' mismatch lists;
// LAMSA_HP_TAG_SUMMARY: the records are the 15 words of the item (no CIGAR, no list)
void parse_stream(const int32_t *s, int n_words, int read_len, ReadResult &R, int tags = 0);
// a record's covered read interval (1-based, forward strand) from its CIGAR, strand and the read's length
void cigar_read_interval(const std::vector<int32_t> &cigar, int nstrand, int read_len, int &beg, int &end);
// the eight summary words of include/lamsa_hp.h (LAMSA_HP_TAG_SUMMARY) from the record's CIGAR, ops 0, 7 and 8 alike: reg_beg, reg_end and the
// six fields behind `summed`.  For --paf-cg, for a library without lamsa_hp_set_result_tags, and for the records stage 4 makes on the host
void rec_summary(Rec &r, int read_len);
void rank_results(ReadResult &R, int read_len, const lamsa_hp_para &P);
// the record's CIGAR into =/X form from its mismatch list, to the definition of include/lamsa_hp.h (what the device does under
// LAMSA_HP_TAG_EQX): for a library without lamsa_hp_set_result_tags, and for the records stage 4 makes on the host
void rec_to_eqx(Rec &r);
// the gaps of the record's CIGAR (M form) left-aligned, by the procedure of include/lamsa_hp.h (what the device does under
// LAMSA_HP_TAG_LEFT_ALIGN): for a library without lamsa_hp_set_result_tags, and for the records stage 4 makes on the host.
// oriented_read: the read's base codes on the record's strand (reverse complement for '-'), read_len of them
void rec_left_align(Rec &r, const uint8_t *oriented_read, int read_len, const Index &ix);

// a path as one word of a POSIX shell command line: wrapped in single quotes, embedded ones spelled '\''
inline std::string shell_quote(const std::string &p) { std::string o = "'"; for (char c : p) { if (c == '\'') o += "'\\''"; else o += c; } return o + "'"; }

struct Options {
    std::string ref_prefix, reads, seed_result;
    int supp_soft = 0, comm = 0, device = 0, n_thread = 1;
    std::vector<int> devices;                             // --devices 0,1,...: chunks go round-robin over these GPUs (default: --device)
    // seeding front end (lamsa_aln_c, src/lamsa_aln.c:1224-1275): -N reuses <reads>.seed.gem.map, otherwise the read file is
    // cut into seeds and the GEM mapper of the reference's bundle is run on them
    int no_seed_aln = 0, fastest = 0;
    int seed_first = 0;                                   // --seed-first: wait for the mapper before aligning, as the reference does; default: read its map while it is being written
    long mapper_pid = 0;                                  // set by main(): the mapper started by run_seeding and still running
    std::string save_hits, hits;                          // --save-hits FILE: also write the parsed chunks as a binary hit stream; --hits FILE: read that instead of the GEM map text
    int shard_i = 0, shard_n = 1;                         // --shard i/N: this process aligns the i-th of N contiguous parts of the read stream (one process per GPU);
                                                          // the outputs of shards 0 .. N-1 concatenated are the unsharded output (only shard 0 writes the header)
    int parse_only = 0;                                   // --parse-only: read and parse the inputs, no GPU work, no output (ingest timing)
    int tag_md = 0, tag_sa = 0;                           // --MD, --SA: MD:Z / SA:Z at the end of every mapped record (not in the reference's output)
    int tag_eqx = 0, tag_cs = 0;                          // --eqx: every printed CIGAR in =/X form (LAMSA_HP_TAG_EQX, include/lamsa_hp.h); --cs: cs:Z (short form) on every mapped record
    int paf = 0, paf_cg = 0;                              // --paf: PAF lines from the per-record summaries of the GPU (LAMSA_HP_TAG_SUMMARY); --paf-cg: PAF with cg:Z from the ordinary stream
    int rescue_gpu = 0;                                   // --rescue-gpu: the exact search of stage 4 on the GPU, one lamsa_hp_fm_search per chunk (include/lamsa_hp.h)
    int seed_fm = 0;                                      // --seed-fm: the seeds of every chunk searched exactly in the FM index on the GPU, one lamsa_hp_fm_seed per chunk: no GEM mapper, no map text
    int left_align = 0;                                   // --left-align: the gaps of every printed CIGAR shifted as far left as they go (LAMSA_HP_TAG_LEFT_ALIGN, include/lamsa_hp.h)
    float ed_rate = -1, mis_rate = -1, mat_rate = -1;     // -e, -x; defaults per read type (src/lamsa_aln.h:26-70)
    std::string gem_dir;                                  // directory holding gem-mapper (default: <directory of this binary>/gem)
    int chunk_reads = 16384; int64_t chunk_bases = 256ll << 20;     // reads per GPU batch (the reference's CHUNK_READ_N is 128 per thread pool)
};
struct Stats { long n_reads = 0, n_bases = 0, n_bad = 0; double kernel_ms = 0;
               double wall_s = 0, load_s = 0, parse_s = 0, submit_s = 0, wait_s = 0, sam_s = 0, reserve_s = 0; };   // where the chunk loop's time went

void sam_header(std::string &o, const Index &ix, const std::string &pg);
void write_sam(std::string &o, const ReadResult &R, const Read &rd, const Index &ix, const Options &opt);
// PAF lines of the records write_sam would print, in its order, every XA:Z alternative as a line of its own behind its record; every record summed
void write_paf(std::string &o, const ReadResult &R, const Read &rd, const Index &ix, const Options &opt);
int run_seeding(const Options &opt, const lamsa_hp_para &P, long *pid = nullptr);   // pid: leave the mapper running and return its process id
int run_index(const std::string &fasta, const std::string &gem_dir, bool with_gem, bool from_pac = false);      // index.cpp
int run_aln(const Options &opt, const lamsa_hp_para &P, FILE *out, const std::string &pg_line, Stats *stats);

}  // namespace lamsa
