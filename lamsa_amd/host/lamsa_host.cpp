// lamsa_host.cpp -- host side of `lamsa aln`: everything around the MI355X hot path.
//
// Mirrors the reference's driver for the path (same files, same option letters, same SAM):
//   load_index      <- bns_restore_core + .pac read            src/bntseq.c:114-166, src/lamsa_aln.c:1237-1239
//   FastxReader     <- kseq_read with KS_SEP_REF names          src/kseq.h:179-225 (name ends at '\n', ':' or ',')
//   parse_gem_hits  <- gem_map_read / gem_map_msg / md2cigar    src/gem_parse.c:74-286, map_cal_msg src/lamsa_aln.c:767
//   cov_fraction    <- get_reg + get_cov_f                      src/lamsa_aln.c:571-651
//   rank_results    <- rearr_aln_res                            src/lamsa_aln.c:654-724
//   write_sam       <- aln_res_output / print_sam_header        src/lamsa_aln.c:1001-1100,1215
//   run_aln         <- lamsa_aln_core chunk loop                src/lamsa_aln.c:1116-1177
// The per-read stages (2),(3),(2'),(3') are NOT here: they run on the GPU behind lamsa_hp_align_batch()
// (include/lamsa_hp.h).  Stage (4), the BWT rescue of short uncovered regions (src/bwt_aln.c), is in rescue.cpp.
#include "lamsa_host.h"
#include "rescue.h"
// referenced weakly: a C-ABI without it (the tests' CPU emulation of the library) leaves it null, and --MD then derives the mismatch
// lists on the host with the walk of the stage-4 records (rec_aux); the product's library always has it and the device lists them
#pragma weak lamsa_hp_set_result_tags
// likewise the resident FM index: without the two calls --rescue-gpu says so and stage 4 searches on the host as it does by default
#pragma weak lamsa_hp_fm_load
#pragma weak lamsa_hp_fm_search
// and seeding in that index: without lamsa_hp_fm_seed --seed-fm is an error (there is no host seeding path)
#pragma weak lamsa_hp_fm_seed
#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <condition_variable>
#include <functional>
#include <future>
#include <mutex>
#include <memory>
#include <thread>
#include <time.h>
#include <zlib.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include <fcntl.h>
#include <signal.h>
#include <sstream>
#include <sys/wait.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

namespace lamsa {

// ------------------------------------------------------------------ index
bool load_index(const std::string &prefix, Index &ix, std::string &err)
{
    FILE *fp = fopen((prefix + ".ann").c_str(), "r");
    if (!fp) { err = "cannot open " + prefix + ".ann"; return false; }
    long long l_pac; int n_seqs; unsigned seed;
    if (fscanf(fp, "%lld%d%u", &l_pac, &n_seqs, &seed) != 3) { fclose(fp); err = "bad .ann header"; return false; }
    ix.name.resize(n_seqs); ix.off.resize(n_seqs); ix.len.resize(n_seqs);
    for (int i = 0; i < n_seqs; ++i) {
        unsigned gi; int c, n_ambs; long long off; std::string line;
        if (fscanf(fp, "%u", &gi) != 1) { fclose(fp); err = "bad .ann record"; return false; }
        while ((c = fgetc(fp)) != '\n' && c != EOF) line.push_back((char)c);
        {   // bns_restore_core reads the name with %s: the first blank-delimited word; the rest of the line is the comment
            size_t a = 0; while (a < line.size() && isspace((unsigned char)line[a])) ++a;
            size_t b = a; while (b < line.size() && !isspace((unsigned char)line[b])) ++b;
            ix.name[i] = line.substr(a, b - a);
        }
        if (fscanf(fp, "%lld%d%d", &off, &ix.len[i], &n_ambs) != 3) { fclose(fp); err = "bad .ann record"; return false; }
        ix.off[i] = off;
    }
    fclose(fp);
    fp = fopen((prefix + ".pac").c_str(), "rb");
    if (!fp) { err = "cannot open " + prefix + ".pac"; return false; }
    ix.l_pac = l_pac;
    ix.pac.assign((size_t)(l_pac / 4 + 1) + 16, 0);
    size_t got = fread(ix.pac.data(), 1, (size_t)(l_pac / 4 + 1), fp);
    fclose(fp);
    if (got == 0 && l_pac > 4) { err = "empty .pac"; return false; }
    for (int i = 0; i < n_seqs; ++i) ix.name_to_id[ix.name[i]] = i + 1;
    return true;
}

// A mapped input file is touched page by page by a helper thread that runs ahead of the reader, so that the reader
// itself does not take the page faults (they cost more than finding the line ends).
struct Prefault {
    std::thread th; std::atomic<bool> stop{false};
    void start(const char *p, size_t n) {
        th = std::thread([this, p, n]() { unsigned sink = 0; for (size_t i = 0; i < n && !stop.load(std::memory_order_relaxed); i += 4096) sink += (unsigned char)((const volatile char *)p)[i]; (void)sink; });
    }
    void finish() { stop = true; if (th.joinable()) th.join(); }
};

// ------------------------------------------------------------------ FASTA / FASTQ (+gz)
struct FastxReader::Impl {
    gzFile f = nullptr; std::string line; bool have = false;
    const char *m = nullptr; size_t mn = 0, mpos = 0;       // an uncompressed regular file is mapped instead of read through zlib
    size_t limit = (size_t)-1; size_t line_at = 0;           // restrict(): records that start at or beyond `limit` are not delivered; line_at: where the current line began
    Prefault pf;
};
bool FastxReader::mapped() const { return p->m != nullptr; }
size_t FastxReader::size() const { return p->mn; }
// is there a record header at offset `at` (which is the beginning of a line)?  The file's first byte says which kind it is.  FASTA: a line
// that begins with '>'.  FASTQ (four lines per record here, as every shardable file has): a line that begins with '@' and whose line after
// next begins with '+' -- a quality line may begin with '@' or '>' (Phred 31 / 29) too, but the line two below such a one is a sequence line.
static bool record_starts_at(const char *m, size_t n, size_t at)
{
    if (at >= n || n == 0) return false;
    if (m[0] != '@') return m[at] == '>';
    if (m[at] != '@') return false;
    const char *l1 = (const char *)memchr(m + at, '\n', n - at);
    if (!l1) return false;
    const char *l2 = (const char *)memchr(l1 + 1, '\n', (size_t)(m + n - (l1 + 1)));
    return l2 && l2 + 1 < m + n && l2[1] == '+';
}
void FastxReader::restrict(size_t lo, size_t hi)
{
    if (!p->m) return;
    size_t at = lo;
    if (at > 0) {                                             // the first beginning of a line at or after lo ...
        const char *nl = (const char *)memchr(p->m + at - 1, '\n', p->mn - (at - 1));
        at = nl ? (size_t)(nl - p->m) + 1 : p->mn;
    }
    while (at < p->mn && !record_starts_at(p->m, p->mn, at)) {    // ... that begins a record
        const char *nl = (const char *)memchr(p->m + at, '\n', p->mn - at);
        at = nl ? (size_t)(nl - p->m) + 1 : p->mn;
    }
    p->mpos = at; p->have = false; p->limit = hi;
}
FastxReader::FastxReader() : p(new Impl) {}
FastxReader::~FastxReader() { p->pf.finish(); if (p->f) gzclose(p->f); if (p->m) munmap((void *)p->m, p->mn); delete p; }
bool FastxReader::open(const std::string &path)
{
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd >= 0) {
        struct stat st; unsigned char magic[2] = {0, 0};
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0 && pread(fd, magic, 2, 0) == 2 && !(magic[0] == 0x1f && magic[1] == 0x8b)) {
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) { madvise(m, (size_t)st.st_size, MADV_SEQUENTIAL); p->m = (const char *)m; p->mn = (size_t)st.st_size; ::close(fd); p->pf.start(p->m, p->mn); return true; }
        }
        ::close(fd);
    }
    p->f = gzopen(path.c_str(), "r");
    return p->f != nullptr;
}
static bool next_line(FastxReader::Impl *p)
{
    if (p->have) { p->have = false; return true; }
    if (p->m) {
        if (p->mpos >= p->mn) return false;
        p->line_at = p->mpos;
        const char *a = p->m + p->mpos, *nl = (const char *)memchr(a, '\n', p->mn - p->mpos);
        const char *e = nl ? nl : p->m + p->mn;
        p->mpos = (size_t)(e - p->m) + (nl ? 1 : 0);
        while (e > a && (e[-1] == '\r' || e[-1] == '\n')) --e;
        p->line.assign(a, (size_t)(e - a));
        return true;
    }
    p->line.clear();
    char buf[1 << 16];
    bool any = false;
    while (gzgets(p->f, buf, sizeof buf)) {
        any = true;
        size_t n = strlen(buf);
        p->line.append(buf, n);
        if (n && buf[n - 1] == '\n') break;
    }
    if (!any) return false;
    while (!p->line.empty() && (p->line.back() == '\n' || p->line.back() == '\r')) p->line.pop_back();
    return true;
}
// A record of a mapped file, read straight out of the mapping: one copy of the sequence (into r.seq), none of the lines -- the sequential
// pass over the read file is what bounds the host side once the hits come from a binary stream (tools/cli_bench.py).
static bool next_mapped(FastxReader::Impl *p, Read &r)
{
    const char *m = p->m; const size_t n = p->mn;
    size_t at = p->mpos;
    auto line_end = [&](size_t from, size_t &next) { const char *nl = (const char *)memchr(m + from, '\n', n - from); size_t e = nl ? (size_t)(nl - m) : n; next = nl ? e + 1 : n; while (e > from && m[e - 1] == '\r') --e; return e; };
    // the next header line
    for (;;) {
        if (at >= n) { p->mpos = n; return false; }
        if (m[at] == '>' || m[at] == '@') break;
        size_t nx; line_end(at, nx); at = nx;
    }
    if (at >= p->limit) { p->mpos = at; return false; }                        // the record belongs to the next shard
    const bool fastq = m[at] == '@';
    size_t nx; size_t e = line_end(at, nx);
    { const char *h = m + at + 1; size_t k = 0, hl = e - (at + 1); while (k < hl && h[k] != ':' && h[k] != ',') ++k; r.name.assign(h, k); }
    at = nx;
    bool plus = false;
    while (at < n) {                                                            // sequence lines, up to the next header or the '+' of a FASTQ record
        const char c0 = m[at];
        if (c0 == '>' || c0 == '@') break;
        if (c0 == '+') { plus = true; line_end(at, nx); at = nx; break; }
        e = line_end(at, nx);
        const size_t k0 = r.seq.size();
        r.seq.append(m + at, e - at);
        unsigned dirty = 0;                                                     // kseq keeps the isgraph() characters of a sequence line (33..126 in the C locale)
        { const char *d = r.seq.data(); const size_t k1 = r.seq.size(); for (size_t k = k0; k < k1; ++k) dirty |= (unsigned)((unsigned char)(d[k] - 33) >= 94); }
        if (dirty) r.seq.erase(std::remove_if(r.seq.begin() + (long)k0, r.seq.end(), [](char c) { return (unsigned char)(c - 33) >= 94; }), r.seq.end());
        at = nx;
    }
    if (fastq && plus) {
        while (r.qual.size() < r.seq.size() && at < n) { e = line_end(at, nx); r.qual.append(m + at, e - at); at = nx; }
        if (r.qual.size() > r.seq.size()) r.qual.resize(r.seq.size());
        r.has_qual = true;
    }
    p->mpos = at;
    return true;
}

bool FastxReader::spans() const { return p->m != nullptr && p->mn > 0 && p->m[0] == '>'; }
bool FastxReader::next_span(size_t &beg, size_t &end)
{
    if (!spans() || p->have) return false;
    const char *m = p->m; const size_t n = p->mn;
    size_t at = p->mpos;
    while (at < n && m[at] != '>') { const char *nl = (const char *)memchr(m + at, '\n', n - at); at = nl ? (size_t)(nl - m) + 1 : n; }      // the next header line
    if (at >= n) { p->mpos = n; return false; }
    if (at >= p->limit) { p->mpos = at; return false; }                        // the record belongs to the next shard
    beg = at;
    do { const char *nl = (const char *)memchr(m + at, '\n', n - at); at = nl ? (size_t)(nl - m) + 1 : n; } while (at < n && m[at] != '>');
    end = at; p->mpos = at;
    return true;
}
bool FastxReader::parse_span(size_t beg, size_t end, Read &r) const
{
    Impl q; q.m = p->m; q.mn = end; q.mpos = beg;                              // a view of the mapping that ends with the record (it owns nothing)
    r.seq.clear(); r.qual.clear(); r.has_qual = false;
    const bool ok = next_mapped(&q, r);
    q.m = nullptr;
    return ok;
}

bool FastxReader::next(Read &r)
{
    r.seq.clear(); r.qual.clear(); r.has_qual = false;
    if (p->m && !p->have) return next_mapped(p, r);
    do { if (!next_line(p)) return false; } while (p->line.empty() || (p->line[0] != '>' && p->line[0] != '@'));
    if (p->m && p->line_at >= p->limit) { p->have = true; return false; }     // the record belongs to the next shard
    const bool fastq = p->line[0] == '@';
    size_t nl = strcspn(p->line.c_str() + 1, ":,");
    r.name.assign(p->line, 1, nl);
    while (next_line(p)) {
        const char c0 = p->line.empty() ? 0 : p->line[0];
        if (c0 == '>' || c0 == '+' || c0 == '@') { if (c0 != '+') p->have = true; break; }
        const size_t k0 = r.seq.size();                                   // kseq keeps the isgraph() characters of a sequence line
        r.seq.append(p->line);
        unsigned dirty = 0;                                               // isgraph() in the C locale: 33..126
        { const char *d = r.seq.data(); const size_t k1 = r.seq.size(); for (size_t k = k0; k < k1; ++k) dirty |= (unsigned)((unsigned char)(d[k] - 33) >= 94); }
        if (dirty) r.seq.erase(std::remove_if(r.seq.begin() + (long)k0, r.seq.end(), [](char c) { return (unsigned char)(c - 33) >= 94; }), r.seq.end());
    }
    if (fastq && !p->have) {
        while (r.qual.size() < r.seq.size() && next_line(p)) r.qual += p->line;
        if (r.qual.size() > r.seq.size()) r.qual.resize(r.seq.size());
        r.has_qual = true;
    }
    return true;
}

// ------------------------------------------------------------------ GEM map line -> hits
template <class V> static inline void cig_push1(V &c, size_t base, int32_t w)
{   // _push_cigar1, src/frag_check.h:153 (restricted to the CIGAR that starts at `base`)
    if ((w >> 4) == 0) return;
    if (c.size() > base && (c.back() & 0xf) == (w & 0xf)) { c.back() += (w >> 4) << 4; return; }
    c.push_back(w);
}

// the same on the compact form (op << 6 | len, len <= 63, ops M / I / D); false: the element does not fit
static inline bool cig8_push1(RawVec<uint8_t> &c, size_t base, int32_t w)
{
    const int len = w >> 4, op = w & 0xf;
    if (len == 0) return true;
    if (c.size() > base && (c.back() >> 6) == op) { const int nl = (c.back() & 63) + len; c.back() = (uint8_t)((op << 6) | (nl & 63)); return nl <= 63 && op <= 2; }
    c.push_back((uint8_t)((op << 6) | (len & 63)));
    return len <= 63 && op <= 2;
}

// one hit "chr:strand:pos:gigar" appended to the batch; md2cigar, src/gem_parse.c:74-112.  The text is a view into the
// mapped file: every scan is bounded by the token's end.
static void add_hit(Batch &B, const Index &ix, const char *tok, size_t len)
{
    const char *e = tok + len, *c1 = tok;
    while (c1 < e && *c1 != ':') ++c1;
    if (c1 >= e) return;
    const char strand = c1 + 1 < e ? c1[1] : '+';
    const char *c2 = c1 + 2;
    while (c2 < e && *c2 != ':') ++c2;
    if (c2 >= e) return;
    long long pos = 0;                                                     // atoll on the field
    const char *c3 = c2 + 1;
    { bool neg = false; if (c3 < e && (*c3 == '-' || *c3 == '+')) { neg = *c3 == '-'; ++c3; } for (; c3 < e && *c3 >= '0' && *c3 <= '9'; ++c3) pos = pos * 10 + (*c3 - '0'); if (neg) pos = -pos; }
    while (c3 < e && *c3 != ':') ++c3;
    const char *md = c3 < e ? c3 + 1 : e, *mdend = md;
    while (mdend < e && *mdend != ':') ++mdend;
    const bool compact = B.parse_compact;
    const size_t base = compact ? B.cig8.size() : B.cig.size();
    bool fits = true;
#define HP_HIT_PUSH(w_) do { if (compact) fits &= cig8_push1(B.cig8, base, (w_)); else cig_push1(B.cig, base, (w_)); } while (0)
    int nm = 0, bd = 0, bi = 0;
    for (const char *q = md; q < mdend;) {
        if (*q == '>') {
            int n = 0;                                                     // atoi(q + 1)
            const char *s = q + 1;
            bool neg = false; if (s < mdend && (*s == '-' || *s == '+')) { neg = *s == '-'; ++s; }
            const char *d0 = s;
            for (; s < mdend && *s >= '0' && *s <= '9'; ++s) n = n * 10 + (*s - '0');
            if (neg) { n = -n; s = d0 - 1; }                               // ">-3": atoi takes the sign, the scan below stops at it
            while (s < mdend && *s != '+' && *s != '-') ++s;
            if (s < mdend && *s == '+') { bd += n; HP_HIT_PUSH((n << 4) | 2); } else { bi += n; HP_HIT_PUSH((n << 4) | 1); }
            nm += n;
            int d = 1; for (int t = n; t >= 10; t /= 10) ++d;
            q += d + 2;
        } else {
            int m = 0, mm = 0, run = 0; bool in_run = false;
            for (; q < mdend && *q != '>'; ++q) {
                const char ch = *q;
                if (ch >= 'A' && ch <= 'T') { ++mm; if (in_run) { m += run; run = 0; in_run = false; } }
                else if (ch >= '0' && ch <= '9') { run = in_run ? run * 10 + (ch - '0') : (ch - '0'); in_run = true; }
                else if (in_run) { m += run; run = 0; in_run = false; }
            }
            if (in_run) m += run;
            HP_HIT_PUSH(((m + mm) << 4) | 0);
            nm += mm;
        }
    }
#undef HP_HIT_PUSH
    if (!fits) B.saw_wide = true;
    if (strand == '-') { if (compact) std::reverse(B.cig8.begin() + (long)base, B.cig8.end()); else std::reverse(B.cig.begin() + (long)base, B.cig.end()); }      // _invert_cigar, src/gem_parse.c:267
    // contig name -> id (map_cal_msg's strcmp scan, src/lamsa_aln.c:767); consecutive hits mostly share the contig
    // (the hits of a repeat seed go from contig to contig: a small cache per thread, keyed by a hash of the name, in front of the map)
    struct NameSlot { std::string name; int id = 0; const Index *ix = nullptr; };
    static thread_local NameSlot cache[256];
    const size_t nl = (size_t)(c1 - tok);
    unsigned hsh = 2166136261u;
    for (size_t k = 0; k < nl; ++k) hsh = (hsh ^ (unsigned char)tok[k]) * 16777619u;
    NameSlot &slot = cache[(hsh ^ (hsh >> 8) ^ (hsh >> 16)) & 255];
    if (slot.ix != &ix || slot.name.size() != nl || memcmp(slot.name.data(), tok, nl) != 0) {
        slot.name.assign(tok, nl); slot.ix = &ix;
        auto it = ix.name_to_id.find(slot.name);
        slot.id = it == ix.name_to_id.end() ? -1 : it->second;
    }
    const int last_id = slot.id;
    B.h_pos.push_back(pos); B.h_chr.push_back(last_id); B.h_strand.push_back(strand == '+' ? 1 : -1);
    B.h_nm.push_back((int16_t)nm); B.h_len_dif.push_back((int16_t)(bd - bi));
    if (compact) {
        if (B.cig8.size() - base > 255) B.cig8.resize(base + 255);         // the boundary counts a seed's CIGAR in 8 bits: the surplus goes, so that the counts add up to the arena
        B.h_cig_n.push_back((uint8_t)(B.cig8.size() - base));
    } else {
        B.h_cig_off.push_back((int32_t)base);
        if (B.cig.size() - base > 255) B.cig.resize(base + 255);
        B.h_cig_n.push_back((uint8_t)(B.cig.size() - base));
    }
}

// all hits of one seed; more than max_n hits: the seed keeps its slot but loses all hits (src/gem_parse.c:243-246)
static void parse_gem_hits(Batch &B, const Index &ix, const char *s, const char *end, int max_n)
{
    const size_t h0 = B.h_pos.size(), c0 = B.parse_compact ? B.cig8.size() : B.cig.size();
    int n = 0;
    for (const char *p = s; p < end;) {
        while (p < end && *p == ',') ++p;
        if (p >= end) break;
        const char *e = (const char *)memchr(p, ',', (size_t)(end - p)); if (!e) e = end;
        if (n >= max_n) {
            B.h_pos.resize(h0); B.h_chr.resize(h0); B.h_strand.resize(h0); B.h_nm.resize(h0); B.h_len_dif.resize(h0); B.h_cig_n.resize(h0);
            if (B.parse_compact) B.cig8.resize(c0); else { B.h_cig_off.resize(h0); B.cig.resize(c0); }
            return;
        }
        add_hit(B, ix, p, (size_t)(e - p));
        ++n; p = e;
    }
}

void Batch::clear()
{
    reads.clear(); read_off.assign(1, 0); read_seq.clear(); seed_all.clear(); last_len.clear(); seed_off.assign(1, 0); seed_id.clear(); hit_off.assign(1, 0);
    h_pos.clear(); h_chr.clear(); h_strand.clear(); h_nm.clear(); h_len_dif.clear(); h_cig_off.clear(); h_cig_n.clear(); cig.clear(); cig8.clear(); cig_wide = false; saw_wide = false;
}

static const uint8_t *nt4_table()
{   // nst_nt4_table, src/bntseq.c:20 ('-' maps to 5 there; the hot path accepts 0..4, so it is treated as N)
    static uint8_t t[256]; static bool init = false;
    if (!init) { memset(t, 4, 256); t['A'] = t['a'] = 0; t['C'] = t['c'] = 1; t['G'] = t['g'] = 2; t['T'] = t['t'] = 3; init = true; }
    return t;
}

// one read + its seed_all GEM map lines -> batch (lamsa_read_seq, src/lamsa_aln.c:927-956; split_seed :252-253,281).
// [lines, lines_end): the read's seed_all map lines as they are in the file, each ending in '\n'.
static void append_read_lines(Batch &B, const Index &ix, const lamsa_hp_para &P, const Read &rd, const char *lines, const char *lines_end, int seed_all)
{
    const int L = (int)rd.seq.size();
    const uint8_t *t4 = nt4_table();
    const size_t b0 = B.read_seq.size();
    B.read_seq.resize(b0 + (size_t)L);
    for (int i = 0; i < L; ++i) B.read_seq[b0 + (size_t)i] = t4[(unsigned char)rd.seq[(size_t)i]];
    B.read_off.push_back((int64_t)B.read_seq.size());
    B.seed_all.push_back(seed_all); B.last_len.push_back(L - P.seed_len - (seed_all - 1) * P.seed_step);
    const char *line = lines;
    for (int sd = 0; sd < seed_all && line < lines_end; ++sd) {
        const char *eol = (const char *)memchr(line, '\n', (size_t)(lines_end - line));
        if (!eol) eol = lines_end;
        const char *q = line; int ct = 0;
        for (; q < eol; ++q) if (*q == '\t') { if (ct == 3) break; ct++; }
        if (q < eol && q + 1 < eol && q[1] != '-') {                    // otherwise no map content: the seed gets no slot
            const char *he = eol; if (he > q + 1 && he[-1] == '\r') --he;
            B.seed_id.push_back(sd + 1);
            parse_gem_hits(B, ix, q + 1, he, P.per_aln_m);
            B.hit_off.push_back((int64_t)B.h_pos.size());
        }
        line = eol + 1;
    }
    B.seed_off.push_back((int64_t)B.seed_id.size());
}

static int seeds_of(const lamsa_hp_para &P, int L) { return L < P.seed_len ? 0 : 1 + (L - P.seed_len) / P.seed_step; }

// the seed-result file, mapped (or, where that fails, read) into memory: lines are handed out as spans, never copied
struct MapText {
    const char *p = nullptr; size_t n = 0, pos = 0; bool mapped = false; std::vector<char> owned; Prefault pf;
    // Follow mode (the reference runs the mapper to completion first, src/lamsa_aln.c:1179-1193): the map
    // is still being written by the mapper started by run_seeding; lines are read as they appear, the end of the file counts only once
    // the mapper has exited.  The text of a read is handed out as a string of its own (the chunk keeps it until it is parsed).
    int follow_fd = -1; long follow_pid = 0; int follow_status = 0; bool follow_done = false; std::string fbuf; size_t fpos = 0; std::string follow_path;
    bool following() const { return follow_pid != 0; }
    bool open_follow(const std::string &path, long pid) { follow_path = path; follow_pid = pid; p = ""; return true; }
    // more bytes of the growing file into fbuf; false: the mapper is gone and everything it wrote has been read
    bool follow_more() {
        for (;;) {
            if (follow_fd < 0) follow_fd = ::open(follow_path.c_str(), O_RDONLY);
            if (follow_fd >= 0) {
                if (fpos > (1u << 20)) { fbuf.erase(0, fpos); fpos = 0; }
                const size_t at = fbuf.size();
                fbuf.resize(at + (1u << 20));
                const ssize_t got = ::read(follow_fd, &fbuf[at], 1u << 20);
                fbuf.resize(at + (got > 0 ? (size_t)got : 0));
                if (got > 0) return true;
            }
            if (follow_done) return false;                                    // the mapper had exited before this (empty) read
            int st = 0;
            const pid_t w = waitpid((pid_t)follow_pid, &st, WNOHANG);
            if (w == (pid_t)follow_pid || w < 0) { follow_done = true; follow_status = w < 0 ? -1 : st; continue; }   // one more read picks up what it wrote last
            usleep(2000);
        }
    }
    // the next `lines` lines of the growing map as one string; false when the mapper's output ends first
    bool take_follow(int lines, std::string &out) {
        out.clear();
        size_t scan = fpos;
        for (int left = lines; left > 0; ) {
            const void *nl = scan < fbuf.size() ? memchr(fbuf.data() + scan, '\n', fbuf.size() - scan) : nullptr;
            if (nl) { scan = (size_t)((const char *)nl - fbuf.data()) + 1; --left; continue; }
            const size_t keep = scan - fpos;
            if (!follow_more()) return false;
            scan = fpos + keep;                                                // fbuf may have been compacted: fpos moved with it
        }
        out.assign(fbuf.data() + fpos, scan - fpos);
        fpos = scan;
        return true;
    }
    // after the last read: has the mapper ended well?  (waits for it)
    bool follow_finish() {
        if (!follow_pid) return true;
        if (!follow_done) { int st = 0; follow_status = waitpid((pid_t)follow_pid, &st, 0) < 0 ? -1 : st; follow_done = true; }
        if (follow_fd >= 0) { ::close(follow_fd); follow_fd = -1; }
        return follow_status != -1 && WIFEXITED(follow_status) && WEXITSTATUS(follow_status) == 0;
    }
    bool open(const std::string &path) {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
            n = (size_t)st.st_size;
            if (n == 0) { ::close(fd); p = ""; return true; }
            void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) { madvise(m, n, MADV_SEQUENTIAL); p = (const char *)m; mapped = true; ::close(fd); pf.start(p, n); return true; }
        }
        char buf[1 << 16]; ssize_t got;                                    // a pipe or a file system without mmap
        while ((got = ::read(fd, buf, sizeof buf)) > 0) owned.insert(owned.end(), buf, buf + got);
        ::close(fd);
        p = owned.data(); n = owned.size();
        return true;
    }
    ~MapText() { pf.finish(); if (mapped) munmap((void *)p, n); if (follow_fd >= 0) ::close(follow_fd); }
    // the next `lines` lines as [a, b); false when the file ends first
    bool take(int lines, const char *&a, const char *&b) {
        a = p + pos;
        int left = lines;
#if defined(__x86_64__)
        static const bool avx2 = __builtin_cpu_supports("avx2");
        if (avx2) pos = skip_lines_avx2(p, pos, n, left);
#endif
        for (; left > 0; --left) {
            if (pos >= n) return false;
            const char *nl = (const char *)memchr(p + pos, '\n', n - pos);
            pos = nl ? (size_t)(nl - p) + 1 : n;
        }
        b = p + pos;
        return true;
    }
#if defined(__x86_64__)
    // advance over whole 32-byte blocks while they hold fewer newlines than are still wanted; `left` is updated.  The
    // lines are ~200 bytes, so counting newlines a block at a time beats one memchr call per line.
    __attribute__((target("avx2"))) static size_t skip_lines_avx2(const char *p, size_t pos, size_t n, int &left) {
        const __m256i nl = _mm256_set1_epi8('\n');
        while (left > 0 && pos + 32 <= n) {
            const unsigned m = (unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i *)(p + pos)), nl));
            const int c = __builtin_popcount(m);
            if (c < left) { left -= c; pos += 32; continue; }
            unsigned mm = m;                                               // the left-th newline is inside this block
            for (int i = 1; i < left; ++i) mm &= mm - 1;
            pos += (size_t)__builtin_ctz(mm) + 1; left = 0;
        }
        return pos;
    }
#endif
};

template <class F> static void parallel_blocks(int n, int threads, F fn)
{
    if (threads < 2 || n < 2 * threads) { fn(0, 0, n); return; }
    std::vector<std::thread> th;
    const int per = (n + threads - 1) / threads;
    for (int t = 0; t < threads; ++t) { const int a = t * per, b = std::min(n, a + per); if (a < b) th.emplace_back([=]() { fn(t, a, b); }); }
    for (auto &x : th) x.join();
}

// concatenate per-thread partial batches (offsets become absolute); every thread copies its own part
static void merge_batches(Batch &B, std::vector<Batch> &parts, int threads)
{
    const size_t np = parts.size();
    std::vector<size_t> r0(np + 1, 0), b0(np + 1, 0), s0(np + 1, 0), h0(np + 1, 0), c0(np + 1, 0);
    for (size_t i = 0; i < np; ++i) {
        const Batch &p = parts[i];
        r0[i + 1] = r0[i] + p.seed_all.size(); b0[i + 1] = b0[i] + p.read_seq.size(); s0[i + 1] = s0[i] + p.seed_id.size();
        h0[i + 1] = h0[i] + p.h_pos.size(); c0[i + 1] = c0[i] + (p.parse_compact ? p.cig8.size() : p.cig.size());
    }
    const bool compact_parts = np > 0 && parts[0].parse_compact;      // the parts hold the seed CIGARs as bytes already (none of them met an element that does not fit)
    B.read_off.resize(r0[np] + 1); B.seed_off.resize(r0[np] + 1); B.seed_all.resize(r0[np]); B.last_len.resize(r0[np]); B.read_seq.resize(b0[np]);
    B.seed_id.resize(s0[np]); B.hit_off.resize(s0[np] + 1);
    B.h_pos.resize(h0[np]); B.h_chr.resize(h0[np]); B.h_strand.resize(h0[np]); B.h_nm.resize(h0[np]); B.h_len_dif.resize(h0[np]); B.h_cig_n.resize(h0[np]);
    B.cig8.resize(c0[np]); B.cig.clear(); B.h_cig_off.clear();      // the word form of the CIGARs (4 B per element + 4 B per hit) is only made when an element does not fit a byte
    std::atomic<int> wide(0);
    B.read_off[0] = 0; B.seed_off[0] = 0; B.hit_off[0] = 0;
    auto copy_parts = [&](int i0, int i1) {
        for (int i = i0; i < i1; ++i) {
            Batch &p = parts[(size_t)i];
            for (size_t k = 1; k < p.read_off.size(); ++k) B.read_off[r0[i] + k] = p.read_off[k] + (int64_t)b0[i];
            for (size_t k = 1; k < p.seed_off.size(); ++k) B.seed_off[r0[i] + k] = p.seed_off[k] + (int64_t)s0[i];
            for (size_t k = 1; k < p.hit_off.size(); ++k) B.hit_off[s0[i] + k] = p.hit_off[k] + (int64_t)h0[i];
            std::copy(p.read_seq.begin(), p.read_seq.end(), B.read_seq.begin() + (long)b0[i]);
            std::copy(p.seed_all.begin(), p.seed_all.end(), B.seed_all.begin() + (long)r0[i]);
            std::copy(p.last_len.begin(), p.last_len.end(), B.last_len.begin() + (long)r0[i]);
            std::copy(p.seed_id.begin(), p.seed_id.end(), B.seed_id.begin() + (long)s0[i]);
            std::copy(p.h_pos.begin(), p.h_pos.end(), B.h_pos.begin() + (long)h0[i]);
            std::copy(p.h_chr.begin(), p.h_chr.end(), B.h_chr.begin() + (long)h0[i]);
            std::copy(p.h_strand.begin(), p.h_strand.end(), B.h_strand.begin() + (long)h0[i]);
            std::copy(p.h_nm.begin(), p.h_nm.end(), B.h_nm.begin() + (long)h0[i]);
            std::copy(p.h_len_dif.begin(), p.h_len_dif.end(), B.h_len_dif.begin() + (long)h0[i]);
            std::copy(p.h_cig_n.begin(), p.h_cig_n.end(), B.h_cig_n.begin() + (long)h0[i]);
            {   // the same CIGARs one byte per element (they lie back to back in hit order: no offsets needed on the way to the GPU)
                int w = 0;
                uint8_t *o8 = B.cig8.data() + c0[i];
                if (compact_parts) std::copy(p.cig8.begin(), p.cig8.end(), o8);
                else for (size_t k = 0; k < p.cig.size(); ++k) { const int32_t x = p.cig[k]; w |= (x >> 4) > 63 || (x & 0xf) > 2; o8[k] = (uint8_t)(((x & 3) << 6) | ((x >> 4) & 63)); }
                if (w) wide = 1;
            }
        }
    };
    auto copy_words = [&](int i0, int i1) {                   // second pass, rare: some element is longer than 63
        for (int i = i0; i < i1; ++i) {
            const Batch &p = parts[(size_t)i];
            for (size_t k = 0; k < p.h_cig_off.size(); ++k) B.h_cig_off[h0[i] + k] = (int32_t)(p.h_cig_off[k] + (int64_t)c0[i]);
            std::copy(p.cig.begin(), p.cig.end(), B.cig.begin() + (long)c0[i]);
        }
    };
    auto on_parts = [&](const std::function<void(int, int)> &fn) {
        if (threads < 2 || h0[np] < 4096) { fn(0, (int)np); return; }
        std::vector<std::thread> th;                         // one thread per part
        for (size_t i = 0; i < np; ++i) if (!parts[i].seed_all.empty()) th.emplace_back(fn, (int)i, (int)i + 1);
        for (auto &x : th) x.join();
    };
    on_parts(copy_parts);
    B.cig_wide = wide.load() != 0 || !compact_parts;          // (parts in words: the parse has met an element that does not fit a byte)
    if (B.cig_wide) { B.cig.resize(c0[np]); B.h_cig_off.resize(h0[np]); on_parts(copy_words); }
    for (Batch &p : parts) p.clear();
}

// ------------------------------------------------------------------ result stream -> records
// covered read interval of a record, push_reg_res src/lamsa_aln.c:571-595: the read without the record's soft clips, on the forward strand
void cigar_read_interval(const std::vector<int32_t> &cigar, int nstrand, int read_len, int &beg, int &end)
{
    beg = 1; end = read_len;
    if (cigar.empty()) return;
    const int32_t c0 = cigar.front(), c1 = cigar.back();
    const int32_t head = nstrand == 1 ? c0 : c1, tail = nstrand == 1 ? c1 : c0;
    if ((head & 0xf) == 4) beg = (head >> 4) + 1;
    if ((tail & 0xf) == 4) end = read_len - (tail >> 4);
}

void rec_summary(Rec &r, int read_len)
{
    r.ref_span = r.m_bases = r.ins_bases = r.del_bases = r.ins_runs = r.del_runs = 0;
    for (int32_t w : r.cigar) {
        const int op = w & 0xf, len = w >> 4;
        if (cig_aligned(op)) r.m_bases += len;
        else if (op == 1) { r.ins_bases += len; ++r.ins_runs; }
        else if (op == 2) { r.del_bases += len; ++r.del_runs; }
    }
    r.ref_span = r.m_bases + r.del_bases;
    r.summed = true;
    cigar_read_interval(r.cigar, r.nstrand, read_len, r.reg_beg, r.reg_end);
}

void parse_stream(const int32_t *s, int n_words, int read_len, ReadResult &R, int tags)
{
    const bool with_mm = (tags & LAMSA_HP_TAG_MISMATCHES) != 0, summary = (tags & LAMSA_HP_TAG_SUMMARY) != 0;
    // (R may hold an earlier read's result: its lines, records and CIGAR vectors are reused, not freed and allocated again)
    R.stage[2].clear();
    R.status = n_words > 0 ? s[0] : LAMSA_HP_ST_OVERFLOW;
    if (n_words < 3 || R.status != 0) { R.stage[0].clear(); R.stage[1].clear(); return; }
    int i = 3;
    for (int st = 0; st < 2; ++st) {
        R.stage[st].resize((size_t)s[1 + st]);
        for (Line &ln : R.stage[st]) {
            ln.line_score = s[i]; ln.tol_score = s[i + 1]; ln.tol_NM = s[i + 2]; ln.merg_x = ln.merg_y = 0; ln.mapQ = 0; ln.xa.clear();
            const int n_res = s[i + 3]; i += 4;
            ln.rec.resize((size_t)n_res);
            for (Rec &r : ln.rec) {
                r.offset = (int64_t)(((uint64_t)(uint32_t)s[i + 1] << 32) | (uint32_t)s[i]); r.chr = s[i + 2]; r.nstrand = s[i + 3]; r.score = s[i + 4]; r.NM = s[i + 5];
                r.summed = false;
                if (summary) {                                   // LAMSA_HP_TAG_SUMMARY: cigar_n (not kept) and the eight words that stand for the CIGAR
                    r.reg_beg = s[i + 7]; r.reg_end = s[i + 8]; r.ref_span = s[i + 9]; r.m_bases = s[i + 10]; r.ins_bases = s[i + 11]; r.del_bases = s[i + 12];
                    r.ins_runs = s[i + 13]; r.del_runs = s[i + 14]; r.summed = true; r.cigar.clear(); r.mm.clear(); i += 15;
                    continue;
                }
                const int cn = s[i + 6]; i += 7;
                r.cigar.assign(s + i, s + i + cn); i += cn;
                if (with_mm) { const int nm = s[i]; r.mm.assign(s + i + 1, s + i + 1 + nm); i += 1 + nm; }
                else r.mm.clear();
                cigar_read_interval(r.cigar, r.nstrand, read_len, r.reg_beg, r.reg_end);
            }
        }
    }
}

void rec_left_align(Rec &r, const uint8_t *rd, int read_len, const Index &ix)
{
    // the procedure of include/lamsa_hp.h (LAMSA_HP_TAG_LEFT_ALIGN) as it is written there, on the M form
    std::vector<int32_t> &c = r.cigar;
    const int n = (int)c.size();
    if (n < 3 || r.chr < 1 || (size_t)r.chr > ix.len.size() || r.offset < 1) return;
    int64_t read_tot = 0, ref_tot = 0;
    for (int32_t w : c) { const int op = w & 0xf, len = w >> 4; if (len < 0) return; if (op == 0 || op == 1 || op == 4) read_tot += len; if (op == 0 || op == 2) ref_tot += len; }
    if (read_tot > read_len || r.offset - 1 + ref_tot > ix.len[(size_t)r.chr - 1]) return;       // (a record that fits neither the read nor the contig is flagged elsewhere)
    const int64_t k0 = ix.off[(size_t)r.chr - 1] + r.offset - 1;
    auto T = [&](int64_t p) { const int64_t k = k0 + p; return (int)(ix.pac[(size_t)(k >> 2)] >> ((~k & 3) << 1) & 3); };
    int64_t q = 0, p = 0;
    for (int i = 0; i < n; ++i) {
        const int op = c[(size_t)i] & 0xf, k = c[(size_t)i] >> 4;
        if ((op == 1 || op == 2) && i > 0 && i < n - 1 && (c[(size_t)i - 1] & 0xf) == 0 && (c[(size_t)i + 1] & 0xf) == 0) {
            while ((c[(size_t)i - 1] >> 4) > 1 && (op == 2 ? T(p - 1) == T(p + k - 1) : rd[q - 1] == rd[q + k - 1])) {
                c[(size_t)i - 1] -= 1 << 4; c[(size_t)i + 1] += 1 << 4; --p; --q;
            }
        }
        if (op == 0 || op == 1 || op == 4) q += k;
        if (op == 0 || op == 2) p += k;
    }
}

void rec_to_eqx(Rec &r)
{
    std::vector<int32_t> out;
    out.reserve(r.cigar.size() + 2 * r.mm.size());
    int64_t ref = 0; size_t e = 0;
    for (int32_t w : r.cigar) {
        const int op = w & 0xf, len = w >> 4;
        if (op == 0) {
            const int64_t end = ref + len;
            while (e < r.mm.size() && (r.mm[e] >> 2) < end) {
                const int64_t p = r.mm[e] >> 2;
                size_t j = e;                                    // the run of neighbouring mismatches that starts here (it ends with the element)
                while (j + 1 < r.mm.size() && (r.mm[j + 1] >> 2) == (r.mm[j] >> 2) + 1 && (r.mm[j + 1] >> 2) < end) ++j;
                if (p > ref) out.push_back((int32_t)((p - ref) << 4) | 7);
                out.push_back((int32_t)((j - e + 1) << 4) | 8);
                ref = p + (int64_t)(j - e + 1); e = j + 1;
            }
            if (end > ref) out.push_back((int32_t)((end - ref) << 4) | 7);
            ref = end;
        } else {
            out.push_back(w);
            if (op == 2) ref += len;
            else if (op == 7 || op == 8) { ref += len; while (e < r.mm.size() && (r.mm[e] >> 2) < ref) ++e; }      // in =/X form already
        }
    }
    r.cigar.swap(out);
}

bool rec_finish(Rec &r, const uint8_t *oriented_read, int read_len, const Index &ix, int what, AuxCounts *counts)
{
    if (what & FIN_LEFT_ALIGN) rec_left_align(r, oriented_read, read_len, ix);
    if (what & FIN_AUX) { AuxCounts k; if (!rec_aux(ix, oriented_read, read_len, r, k)) return false; if (counts) *counts = k; }
    if (what & FIN_EQX) rec_to_eqx(r);
    if (what & FIN_SUMMARY) rec_summary(r, read_len);
    return true;
}

const uint8_t *oriented_read(const uint8_t *bseq, int len, int nstrand, std::vector<uint8_t> &rc)
{
    if (nstrand == 1) return bseq;
    if (rc.empty()) { rc.resize((size_t)len); for (int i = 0; i < len; ++i) rc[(size_t)i] = bseq[len - 1 - i] < 4 ? 3 - bseq[len - 1 - i] : 4; }
    return rc.data();
}

void read_finish(ReadResult &R, const uint8_t *bseq, int read_len, const Index &ix, int what)
{
    if (!what || R.status != 0) return;
    std::vector<uint8_t> rc;
    for (int st = 0; st < 2; ++st)
        for (Line &ln : R.stage[st])
            for (Rec &r : ln.rec)
                if (!rec_finish(r, oriented_read(bseq, read_len, r.nstrand, rc), read_len, ix, what)) R.status |= LAMSA_HP_ST_REFEXIT;
}

// a stable sort that allocates nothing for the handful of elements a read has (std::stable_sort asks for a buffer every time)
template <class It, class Less> static inline void small_stable_sort(It b, It e, Less less)
{
    if (e - b > 24) { std::stable_sort(b, e, less); return; }
    for (It i = b + (b != e); i < e; ++i) { auto v = *i; It j = i; while (j > b && less(v, *(j - 1))) { *j = *(j - 1); --j; } *j = v; }
}

// get_cov_f, src/lamsa_aln.c:639-651
static float cov_fraction(const ReadResult &R, int read_len)
{
    std::vector<std::pair<int, int>> reg;
    for (int st = 0; st < 3; ++st) for (const Line &ln : R.stage[st]) { if (ln.tol_score < 0) continue; for (const Rec &r : ln.rec) reg.push_back({r.reg_beg, r.reg_end}); }
    if (reg.empty()) return (float)(0.0 / read_len);
    small_stable_sort(reg.begin(), reg.end(), [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first < b.first; });
    int cov = 0; size_t cur = 0;
    for (size_t i = 1; i < reg.size(); ++i) {                              // aln_merg_reg with thd 0, :499
        if (reg[i].first - reg[cur].second - 1 < 0) { if (reg[i].second > reg[cur].second) reg[cur].second = reg[i].second; }
        else { ++cur; reg[cur] = reg[i]; }
    }
    for (size_t i = 0; i <= cur; ++i) cov += reg[i].second - reg[i].first + 1;
    return (float)((cov + 0.0) / read_len);
}

static float cover_rate(int s1, int e1, int s2, int e2)
{   // src/lamsa_dp_con.c:61-67
    const int s = s2 > s1 ? s2 : s1, e = e2 < e1 ? e2 : e1;
    const float rat1 = (float)((e - s + 1 + 0.0) / (e1 - s1 + 1 + 0.0)), rat2 = (float)((e - s + 1 + 0.0) / (e2 - s2 + 1 + 0.0));
    return rat1 > rat2 ? rat1 : rat2;
}

// rearr_aln_res, src/lamsa_aln.c:654-724
void rank_results(ReadResult &R, int read_len, const lamsa_hp_para &P)
{
    struct Q { int st, li, a, b; };
    std::vector<Q> qua;
    for (int st = 0; st < 3; ++st)
        for (size_t i = 0; i < R.stage[st].size(); ++i) {
            Line &l = R.stage[st][i];
            l.xa.clear(); l.mapQ = 0;
            if (l.tol_score < 0) { l.merg_x = 0; l.merg_y = -1; continue; }
            qua.push_back({st, (int)i, l.tol_score, l.line_score});
        }
    if (qua.empty()) return;
    small_stable_sort(qua.begin(), qua.end(), [](const Q &x, const Q &y) { return x.a != y.a ? x.a > y.a : x.b > y.b; });   // res_comp :632 on glibc's stable qsort
    auto L = [&](int i) -> Line & { return R.stage[qua[i].st][qua[i].li]; };
    std::vector<int> head;
    std::vector<std::pair<int, int>> reg;                                     // intervals of the accepted heads, in acceptance order
    for (const Rec &r : L(0).rec) reg.push_back({r.reg_beg, r.reg_end});
    head.push_back(0);
    L(0).merg_x = 1; L(0).merg_y = 0;
    for (size_t i = 0; i < qua.size(); ++i) L((int)i).mapQ = 255;
    const float cov_f = cov_fraction(R, read_len);
    const int mapq_max = (int)(254 * cov_f);
    for (int i = 1; i < (int)qua.size(); ++i) {
        int cov_qi = -1;
        for (const Rec &nr : L(i).rec) {                                      // get_cover_res :607-629
            size_t reg_i = 0;
            for (int hi : head) {
                for (size_t j = 0; j < L(hi).rec.size(); ++j, ++reg_i)
                    if (cover_rate(reg[reg_i].first, reg[reg_i].second, nr.reg_beg, nr.reg_end) >= P.ovlp_rat) { cov_qi = hi; break; }
                if (cov_qi >= 0) break;
            }
            if (cov_qi >= 0) break;
        }
        if (cov_qi < 0) {
            for (const Rec &r : L(i).rec) reg.push_back({r.reg_beg, r.reg_end});
            head.push_back(i);
            L(i).merg_x = 1; L(i).merg_y = 0;
        } else if (qua[i].a > qua[cov_qi].a / 2 && (int)L(cov_qi).xa.size() + (int)L(i).rec.size() - 1 < P.res_mul_max) {
            for (size_t j = 0; j < L(i).rec.size(); ++j) L(cov_qi).xa.push_back({qua[i].st, qua[i].li, (int)j});
            L(cov_qi).merg_y = 1;
            const uint8_t tmpQ = (uint8_t)(mapq_max * (qua[cov_qi].a - qua[i].a) / qua[cov_qi].a);
            if (tmpQ < L(cov_qi).mapQ) L(cov_qi).mapQ = tmpQ;
            L(i).merg_x = 2; L(i).merg_y = 0;
        } else { L(i).merg_x = 0; L(i).merg_y = -1; }
    }
    for (size_t i = 0; i < qua.size(); ++i) {
        Line &l = L((int)i);
        if (l.merg_x != 1) continue;
        if (l.mapQ == 255) l.mapQ = (uint8_t)(mapq_max / (int)head.size()); else l.mapQ = (uint8_t)(l.mapQ / (int)head.size());
    }
}

// ------------------------------------------------------------------ SAM
static char comp_char(char c)
{
    switch (c) { case 'A': return 'T'; case 'a': return 't'; case 'C': return 'G'; case 'c': return 'g';
                 case 'G': return 'C'; case 'g': return 'c'; case 'T': return 'A'; case 't': return 'a'; default: return c; }
}
static void appendf(std::string &o, const char *fmt, ...)
{
    char tmp[256]; va_list ap; va_start(ap, fmt); int n = vsnprintf(tmp, sizeof tmp, fmt, ap); va_end(ap);
    if (n < (int)sizeof tmp) { o.append(tmp, (size_t)n); return; }
    std::vector<char> big((size_t)n + 1); va_start(ap, fmt); vsnprintf(big.data(), big.size(), fmt, ap); va_end(ap); o.append(big.data(), (size_t)n);
}

void sam_header(std::string &o, const Index &ix, const std::string &pg)
{   // print_sam_header, src/lamsa_aln.c:1215
    for (size_t i = 0; i < ix.name.size(); ++i) appendf(o, "@SQ\tSN:%s\tLN:%d\n", ix.name[i].c_str(), ix.len[i]);
    o += pg; o += "\n";
}

// aln_res_output, src/lamsa_aln.c:1001-1100.  (`-C` with a reverse-strand FASTQ read never terminates in the
// reference, :1043; here QUAL is printed reversed -- the evident intent, documented divergence.)
// decimal digits of v appended to o (the CIGAR of a 10 kbp noisy read has ~1 500 operations: no printf per operation)
static inline void append_int(std::string &o, long long v)
{
    char buf[24]; int n = 0;
    unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
    do { buf[n++] = (char)('0' + u % 10); u /= 10; } while (u);
    if (v < 0) buf[n++] = '-';
    while (n) o.push_back(buf[--n]);
}
// The CIGAR of a 10-kbp noisy read has ~1 500 operations, nearly all of one or two digits: they are formatted into a block of the string's
// own storage through a pointer (no per-character capacity check), lengths below 100 from a table of digit pairs.
static inline char *put_len(char *p, unsigned v)
{
    static const char D2[] = "00010203040506070809101112131415161718192021222324252627282930313233343536373839404142434445464748495051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";
    if (v < 10) { *p++ = (char)('0' + v); return p; }
    if (v < 100) { p[0] = D2[2 * v]; p[1] = D2[2 * v + 1]; return p + 2; }
    char buf[12]; int n = 0;
    while (v >= 100) { const unsigned q = v / 100, r = v - 100 * q; buf[n++] = D2[2 * r + 1]; buf[n++] = D2[2 * r]; v = q; }
    if (v >= 10) { buf[n++] = D2[2 * v + 1]; buf[n++] = D2[2 * v]; } else buf[n++] = (char)('0' + v);
    while (n) *p++ = buf[--n];
    return p;
}
static inline void append_cigar(std::string &o, const std::vector<int32_t> &cig, const char *ops)
{
    const size_t k0 = o.size();
    o.resize(k0 + 11 * cig.size());                          // at most ten digits and the operation
    char *p = &o[k0];
    for (int32_t w : cig) { p = put_len(p, (unsigned)(w >> 4)); *p++ = ops[w & 0xf]; }
    o.resize((size_t)(p - o.data()));
}

// MD:Z of a record (SAM spec form): its CIGAR walked against its mismatch list, the bases of deletions from the index's .pac.  Where the
// reference has N the .pac holds a substituted base (as the reference's index does); MD shows that base, the one NM was counted against.
static void append_md(std::string &o, const Rec &r, const Index &ix)
{
    static const char B[] = "ACGT";
    const int64_t k0 = ix.off[(size_t)r.chr - 1] + r.offset - 1;      // .pac coordinate of POS
    int64_t ref = 0; int run = 0; size_t e = 0;
    for (int32_t w : r.cigar) {
        const int op = w & 0xf, len = w >> 4;
        if (cig_aligned(op)) {                         // aligned bases, in M or in =/X form
            const int64_t end = ref + len;
            for (; e < r.mm.size() && (r.mm[e] >> 2) < end; ++e) {
                const int64_t p = r.mm[e] >> 2;
                run += (int)(p - ref); append_int(o, run); o.push_back(B[r.mm[e] & 3]);
                run = 0; ref = p + 1;
            }
            run += (int)(end - ref); ref = end;
        } else if (op == 2) {
            append_int(o, run); run = 0; o.push_back('^');
            for (int j = 0; j < len; ++j, ++ref) { const int64_t k = k0 + ref; o.push_back(B[ix.pac[(size_t)(k >> 2)] >> ((~k & 3) << 1) & 3]); }
        }                                                           // I, S, H: nothing of the reference
    }
    append_int(o, run);
}

// cs:Z of a record, minimap2's short form: ":n" identical bases, "*xy" a substitution (reference base, read base), "+seq" inserted read
// bases, "-seq" deleted reference bases; lowercase, a read N is 'n', everything on the forward reference strand (as SEQ is printed); clips
// contribute nothing.  The substituted reference bases come from the mismatch list, the deleted ones from the .pac (MD's caveat on N holds).
static void append_cs(std::string &o, const Rec &r, const Read &rd, const Index &ix)
{
    static const char B[] = "acgt";
    const int read_len = (int)rd.seq.size();
    auto base = [&](int i) {                                          // base i of the read as the record aligns it
        switch (r.nstrand == 1 ? rd.seq[(size_t)i] : comp_char(rd.seq[(size_t)(read_len - 1 - i)])) {
            case 'A': case 'a': return 'a'; case 'C': case 'c': return 'c'; case 'G': case 'g': return 'g'; case 'T': case 't': return 't'; default: return 'n'; }
    };
    const int64_t k0 = ix.off[(size_t)r.chr - 1] + r.offset - 1;
    int64_t ref = 0; int read_i = 0; size_t e = 0;
    for (int32_t w : r.cigar) {
        const int op = w & 0xf, len = w >> 4;
        if (cig_aligned(op)) {
            const int64_t beg = ref, end = ref + len;
            for (; e < r.mm.size() && (r.mm[e] >> 2) < end; ++e) {
                const int64_t p = r.mm[e] >> 2;
                if (p > ref) { o.push_back(':'); append_int(o, (long long)(p - ref)); }
                o.push_back('*'); o.push_back(B[r.mm[e] & 3]); o.push_back(base(read_i + (int)(p - beg)));
                ref = p + 1;
            }
            if (end > ref) { o.push_back(':'); append_int(o, (long long)(end - ref)); }
            ref = end; read_i += len;
        } else if (op == 1) {
            o.push_back('+');
            for (int j = 0; j < len; ++j) o.push_back(base(read_i + j));
            read_i += len;
        } else if (op == 2) {
            o.push_back('-');
            for (int j = 0; j < len; ++j, ++ref) { const int64_t k = k0 + ref; o.push_back(B[ix.pac[(size_t)(k >> 2)] >> ((~k & 3) << 1) & 3]); }
        } else if (op == 4) read_i += len;
    }
}

void write_sam(std::string &o, const ReadResult &R, const Read &rd, const Index &ix, const Options &opt)
{
    static const char OPS[] = "MIDNSHP=XB", OPS_HC[] = "MIDNHHP=XB";
    const int read_len = (int)rd.seq.size();
    const bool with_qual = rd.has_qual && opt.comm;
    int all = 0; bool prim = false;
    // --SA: the records printed for this read, in print order, and the SA:Z entry of each (rname,pos,strand,CIGAR,mapQ,NM; -- soft clips
    // even where the line itself is hard-clipped)
    std::vector<std::string> sa;
    if (opt.tag_sa) {
        for (int st = 0; st < 3; ++st)
            for (const Line &la : R.stage[st]) {
                if (la.merg_x != 1) continue;
                for (const Rec &r : la.rec) {
                    std::string x = ix.name[(size_t)r.chr - 1]; x.push_back(','); append_int(x, (long long)r.offset); x.push_back(','); x.push_back("-+"[r.nstrand]); x.push_back(',');
                    append_cigar(x, r.cigar, OPS); x.push_back(','); append_int(x, (int)la.mapQ); x.push_back(','); append_int(x, r.NM); x.push_back(';');
                    sa.push_back(std::move(x));
                }
            }
    }
    if (o.capacity() - o.size() < 4 * (size_t)read_len + 4096) o.reserve(o.size() + std::max<size_t>(o.size() / 2, 8 * (size_t)read_len + 65536));      // grown in large steps, not per append
    for (int st = 0; st < 3; ++st)
        for (const Line &la : R.stage[st]) {
            if (la.merg_x != 1) continue;
            for (size_t j = 0; j < la.rec.size(); ++j) {
                const Rec &r = la.rec[j];
                ++all;
                int flag = r.nstrand ? 0 : 0x10;
                const bool soft = !prim || opt.supp_soft;
                if (!soft) flag |= 0x800;
                o += rd.name; o.push_back('\t'); append_int(o, flag); o.push_back('\t'); o += ix.name[(size_t)r.chr - 1]; o.push_back('\t');
                append_int(o, (long long)r.offset); o.push_back('\t'); append_int(o, (int)la.mapQ); o.push_back('\t');
                append_cigar(o, r.cigar, soft ? OPS : OPS_HC);
                o += "\t*\t0\t0\t";
                const int b = soft ? 0 : r.reg_beg - 1, e = soft ? read_len : r.reg_end;
                if (r.nstrand == 1) o.append(rd.seq, (size_t)b, (size_t)(e - b));
                else { const size_t k0 = o.size(); o.resize(k0 + (size_t)(e - b)); char *d = &o[k0]; for (int si = e - 1; si >= b; --si) *d++ = comp_char(rd.seq[(size_t)si]); }
                o.push_back('\t');
                if (with_qual) { if (r.nstrand == 1) o.append(rd.qual, (size_t)b, (size_t)(e - b)); else for (int si = e - 1; si >= b; --si) o.push_back(rd.qual[(size_t)si]); }
                else o.push_back('*');
                if (soft) prim = true;
                o += "\tNM:i:"; append_int(o, r.NM); o += "\tAS:i:"; append_int(o, r.score);
                if (j == 0 && !la.xa.empty()) {
                    o += "\tXA:Z:";
                    for (const XaRef &x : la.xa) {
                        const Rec &xr = R.stage[x.st][(size_t)x.li].rec[(size_t)x.ri];
                        o += ix.name[(size_t)xr.chr - 1]; o.push_back(','); o.push_back("-+"[xr.nstrand]); append_int(o, (long long)xr.offset); o.push_back(',');
                        append_cigar(o, xr.cigar, OPS);
                        o.push_back(','); append_int(o, xr.NM); o.push_back(';');
                    }
                }
                if (opt.tag_md) { o += "\tMD:Z:"; append_md(o, r, ix); }
                if (opt.tag_cs) { o += "\tcs:Z:"; append_cs(o, r, rd, ix); }
                if (sa.size() > 1) { o += "\tSA:Z:"; for (size_t k = 0; k < sa.size(); ++k) if (k != (size_t)all - 1) o += sa[k]; }
                o.push_back('\n');
            }
        }
    if (all == 0) {
        appendf(o, "%s\t%d\t*\t%lld\t%d\t*\t*\t0\t0\t", rd.name.c_str(), 4, 0LL, 0);
        o += rd.seq; o.push_back('\t');
        if (rd.has_qual) o += rd.qual; else o.push_back('*');
        o.push_back('\n');
    }
}

// One PAF line from a summed record: the twelve columns, then tp, NM, (AS,) de.  n_mm = NM - inserted - deleted bases (include/lamsa_hp.h).
static void paf_line(std::string &o, const Rec &r, const Read &rd, const Index &ix, int mapq, bool primary)
{
    const int n_mm = r.NM - r.ins_bases - r.del_bases;
    o += rd.name; o.push_back('\t'); append_int(o, (long long)rd.seq.size()); o.push_back('\t'); append_int(o, r.reg_beg - 1); o.push_back('\t'); append_int(o, r.reg_end);
    o.push_back('\t'); o.push_back("-+"[r.nstrand]); o.push_back('\t'); o += ix.name[(size_t)r.chr - 1]; o.push_back('\t'); append_int(o, ix.len[(size_t)r.chr - 1]);
    o.push_back('\t'); append_int(o, (long long)r.offset - 1); o.push_back('\t'); append_int(o, (long long)r.offset - 1 + r.ref_span);
    o.push_back('\t'); append_int(o, r.m_bases - n_mm); o.push_back('\t'); append_int(o, r.m_bases + r.ins_bases + r.del_bases); o.push_back('\t'); append_int(o, mapq);
    o += primary ? "\ttp:A:P\tNM:i:" : "\ttp:A:S\tNM:i:"; append_int(o, r.NM);
    if (primary) { o += "\tAS:i:"; append_int(o, r.score); }
    const int den = r.m_bases + r.ins_runs + r.del_runs;
    appendf(o, "\tde:f:%.4f", den > 0 ? (double)(n_mm + r.ins_runs + r.del_runs) / (double)den : 0.0);
}
static void append_cg(std::string &o, const Rec &r)
{
    static const char OPS[] = "MIDNSHP=XB";
    o += "\tcg:Z:";
    const size_t k0 = o.size();
    o.resize(k0 + 11 * r.cigar.size());
    char *p = &o[k0];
    for (int32_t w : r.cigar) { if ((w & 0xf) == 4) continue; p = put_len(p, (unsigned)(w >> 4)); *p++ = OPS[w & 0xf]; }       // (the clips are columns 3 and 4)
    o.resize((size_t)(p - o.data()));
}

void write_paf(std::string &o, const ReadResult &R, const Read &rd, const Index &ix, const Options &opt)
{
    if (o.capacity() - o.size() < 4096) o.reserve(o.size() + std::max<size_t>(o.size() / 2, 65536));
    for (int st = 0; st < 3; ++st)
        for (const Line &la : R.stage[st]) {
            if (la.merg_x != 1) continue;                       // the lines write_sam prints, in its order
            for (size_t j = 0; j < la.rec.size(); ++j) {
                const Rec &r = la.rec[j];
                paf_line(o, r, rd, ix, (int)la.mapQ, true);
                if (opt.paf_cg) {
                    append_cg(o, r);
                    if (opt.tag_md) { o += "\tMD:Z:"; append_md(o, r, ix); }
                    if (opt.tag_cs) { o += "\tcs:Z:"; append_cs(o, r, rd, ix); }
                }
                o.push_back('\n');
                if (j == 0)
                    for (const XaRef &x : la.xa) {               // the alternatives SAM lists in XA:Z: NM and the CIGAR are all it gives them
                        const Rec &xr = R.stage[x.st][(size_t)x.li].rec[(size_t)x.ri];
                        paf_line(o, xr, rd, ix, 0, false);
                        if (opt.paf_cg) append_cg(o, xr);
                        o.push_back('\n');
                    }
            }
        }
}

// ------------------------------------------------------------------ seeding front end
// split_seed (src/lamsa_aln.c:223-303) + lamsa_gem (:1179-1193, gem/gem_map.sh): the read file is cut into overlapping
// seeds (<reads>.seed, names "<read>_<i>:<offset>"; <reads>.seed.info as the reference writes it) and the GEM mapper is
// run on them with the reference's arguments; its output <reads>.seed.gem.map is what run_aln reads.  The mapper and
// the <ref>.gem index belong to the reference's bundle (`lamsa index`); nothing of them is part of this repository.
// Cuts the seeds as split_seed does (src/lamsa_aln.c:225-303), then starts the bundle's gem-mapper with the arguments of gem/gem_map.sh.
// pid == nullptr: waits for it, as the reference does (lamsa_gem, :1179-1193).  Otherwise the mapper is left running and its process id
// returned: run_aln reads the map while it is being written, so seeding overlaps parsing and the GPU (it must be started before any GPU
// call of this process: a process that has initialised the GPU must not fork + exec on this pool).
int run_seeding(const Options &opt, const lamsa_hp_para &P, long *pid)
{
    FastxReader fx;
    if (!fx.open(opt.reads)) { fprintf(stderr, "[lamsa_aln] Can't open read file %s\n", opt.reads.c_str()); return 1; }
    const std::string seed_f = opt.reads + ".seed", info_f = opt.reads + ".seed.info";
    FILE *sf = fopen(seed_f.c_str(), "w"), *inf = fopen(info_f.c_str(), "w");
    if (!sf || !inf) { fprintf(stderr, "[lamsa_aln] Can't open seed file %s\n", sf ? info_f.c_str() : seed_f.c_str()); if (sf) fclose(sf); if (inf) fclose(inf); return 1; }
    fprintf(stderr, "[lamsa_aln] Generating seed ... ");
    Read rd; std::string o;
    while (fx.next(rd)) {
        const int L = (int)rd.seq.size(), seed_all = seeds_of(P, L);
        o.clear();
        for (int i = 0; i < seed_all; ++i) {
            o += ">"; o += rd.name; o += "_"; o += std::to_string(i); o += ":"; o += std::to_string(i * P.seed_step); o += "\n";
            o.append(rd.seq, (size_t)i * P.seed_step, (size_t)P.seed_len); o += "\n";
        }
        fwrite(o.data(), 1, o.size(), sf);
        fprintf(inf, "%s %d %d %d\n", rd.name.c_str(), seed_all, L - P.seed_len - (seed_all - 1) * P.seed_step, L);
    }
    fclose(sf); fclose(inf);
    fprintf(stderr, "done!\n");
    const int t = P.read_type;
    const float ed = opt.ed_rate >= 0 ? opt.ed_rate : (t == 1 ? 0.3f : (t == 2 ? 0.25f : 0.04f));
    const float mis = opt.mis_rate >= 0 ? opt.mis_rate : (t == 2 ? 0.06f : 0.04f);
    const float mat = opt.mat_rate >= 0 ? opt.mat_rate : (t == 1 ? 0.7f : (t == 2 ? 0.6f : 0.80f));
    const std::string mapper = opt.gem_dir + "/gem-mapper", idx = opt.ref_prefix + ".gem", outp = seed_f + ".gem";
    FILE *probe = fopen(mapper.c_str(), "r");
    if (!probe) { fprintf(stderr, "[lamsa_aln] GEM mapper not found at %s (it ships with the reference; give its directory with --gem-dir, or run with -N on an existing %s.gem.map)\n", mapper.c_str(), seed_f.c_str()); return 1; }
    fclose(probe);
    char num[256];
    snprintf(num, sizeof num, " -m %f -e %f --min-matched-bases %f --max-big-indel-length 3 -d %d -D 0 -T %d %s", mis, ed, mat, P.per_aln_m, opt.n_thread > 0 ? opt.n_thread : 1,
             opt.fastest ? "--fast-mapping=0" : "--fast-mapping");
    ::remove((outp + ".map").c_str());                   // a stale map of an earlier run must not be taken for this one's
    std::vector<std::string> av = {mapper, "-I", idx, "-i", seed_f, "-o", outp};
    { std::istringstream is(num); std::string w; while (is >> w) av.push_back(w); }
    fprintf(stderr, "[lamsa_aln] Executing gem-mapper ... \n");
    fflush(stderr);
    const pid_t child = fork();
    if (child < 0) { fprintf(stderr, "[lamsa_aln] Seeding undone, cannot start gem-mapper.\n"); return 1; }
    if (child == 0) {
        const int lf = ::open((outp + ".log").c_str(), O_WRONLY | O_CREAT | O_APPEND, 0644);
        if (lf >= 0) { dup2(lf, 2); ::close(lf); }
        std::vector<char *> argv;
        for (std::string &a : av) argv.push_back(&a[0]);
        argv.push_back(nullptr);
        execv(mapper.c_str(), argv.data());
        _exit(127);
    }
    if (pid) { *pid = (long)child; return 0; }
    int st = 0;
    if (waitpid(child, &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) { fprintf(stderr, "[lamsa_aln] Seeding undone, gem-mapper exit abnormally.\n"); return 1; }
    fprintf(stderr, "[lamsa_aln] gem-mapper done!\n");
    return 0;
}

// ------------------------------------------------------------------ binary hit stream
// The arrays of lamsa_hp_batch, chunk after chunk, as they go to the GPU: a re-run on the same reads (other scoring /
// filtering options) maps the file and uploads straight from the page cache -- no seeding, no text, no parse.  Native
// byte order; the header pins the options that shape the arrays (-T, -l, -i, -p).
namespace {
const char HITS_MAGIC[8] = {'L', 'A', 'M', 'S', 'A', 'H', 'P', '2'};
struct HitsHeader { char magic[8]; int32_t read_type, seed_len, seed_step, per_aln_m; int64_t reserved[2]; };
struct HitsChunkHeader { int64_t n_reads, n_bases, n_slots, n_hits, n_cig, bytes, cig_elem; };   // bytes: of the arrays that follow (each padded to 64);
                                                                                              // cig_elem 1: cig8, no offsets; 4: cig words + 32-bit offsets
inline size_t pad64(size_t x) { return (x + 63) & ~(size_t)63; }

struct HitsWriter {
    FILE *fp = nullptr;
    bool open(const std::string &path, const lamsa_hp_para &P) {
        fp = fopen(path.c_str(), "wb");
        if (!fp) return false;
        HitsHeader h; memset(&h, 0, sizeof h); memcpy(h.magic, HITS_MAGIC, 8);
        h.read_type = P.read_type; h.seed_len = P.seed_len; h.seed_step = P.seed_step; h.per_aln_m = P.per_aln_m;
        return fwrite(&h, sizeof h, 1, fp) == 1;
    }
    template <class V> bool put(const V &v, size_t n) {
        static const char zeros[64] = {0};
        const size_t bytes = n * sizeof(v[0]);
        if (bytes && fwrite(v.data(), 1, bytes, fp) != bytes) return false;
        const size_t padn = pad64(bytes) - bytes;
        return padn == 0 || fwrite(zeros, 1, padn, fp) == padn;
    }
    bool write(const lamsa::Batch &B) {
        const size_t n = B.reads.size(), nb = B.read_seq.size(), ns = B.seed_id.size(), nh = B.h_pos.size(), nc = B.cig8.size();
        HitsChunkHeader c; c.n_reads = (int64_t)n; c.n_bases = (int64_t)nb; c.n_slots = (int64_t)ns; c.n_hits = (int64_t)nh; c.n_cig = (int64_t)nc; c.cig_elem = B.cig_wide ? 4 : 1;
        c.bytes = (int64_t)(pad64(8 * (n + 1)) * 2 + pad64(nb) + pad64(4 * n) * 2 + pad64(4 * ns) + pad64(8 * (ns + 1)) + pad64(8 * nh) + pad64(4 * nh) + pad64(nh) * 2 + pad64(2 * nh) * 2 +
                            (B.cig_wide ? pad64(4 * nh) + pad64(4 * nc) : pad64(nc)));
        if (fwrite(&c, sizeof c, 1, fp) != 1) return false;
        return put(B.read_off, n + 1) && put(B.read_seq, nb) && put(B.seed_all, n) && put(B.last_len, n) && put(B.seed_off, n + 1) && put(B.seed_id, ns) && put(B.hit_off, ns + 1) &&
               put(B.h_pos, nh) && put(B.h_chr, nh) && put(B.h_strand, nh) && put(B.h_nm, nh) && put(B.h_len_dif, nh) && put(B.h_cig_n, nh) &&
               (B.cig_wide ? put(B.h_cig_off, nh) && put(B.cig, nc) : put(B.cig8, nc));
    }
    void close() { if (fp) fclose(fp); fp = nullptr; }
};
}  // namespace

// ------------------------------------------------------------------ chunk loop
static double now_s() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }

int run_aln(const Options &opt, const lamsa_hp_para &P, FILE *out, const std::string &pg_line, Stats *stats)
{
    const double t_begin = now_s();
    double parse_s = 0, submit_s = 0, wait_s = 0, sam_s = 0;
    long n_mapped_chunks = 0;                                // chunks whose SAM text the threads wrote side by side
    // Every way out of this function before the map has been read to its end -- an index that does not load, a map that does not match
    // the reads, a failed submit -- must not leave the mapper started by run_seeding running (and writing, on -t cores): it is told to
    // stop and waited for, and its exit status reported.
    struct MapperGuard { long pid = 0; MapText *m = nullptr; ~MapperGuard() {
        if (!pid || (m && m->follow_done)) return;
        kill((pid_t)pid, SIGTERM);
        int st = 0; const pid_t w = waitpid((pid_t)pid, &st, 0);
        if (m) m->follow_done = true;
        if (w > 0 && WIFEXITED(st)) fprintf(stderr, "[lamsa_aln] gem-mapper stopped (exit status %d)\n", WEXITSTATUS(st));
        else fprintf(stderr, "[lamsa_aln] gem-mapper stopped (signal %d)\n", w > 0 && WIFSIGNALED(st) ? WTERMSIG(st) : 0);
    } };
    MapText mapt, hitsf;                                // GEM map text, or (--hits) the binary hit stream written by --save-hits (declared before the guard that ends the mapper: destroyed after it)
    MapperGuard orphan; orphan.pid = opt.mapper_pid; orphan.m = &mapt;
    Index ix; std::string err;
    if (!load_index(opt.ref_prefix, ix, err)) { fprintf(stderr, "[lamsa_aln] %s\n", err.c_str()); return 1; }
    const std::string map_path = opt.seed_result.empty() ? opt.reads + ".seed.gem.map" : opt.seed_result;
    const bool from_hits = !opt.hits.empty();
    // --seed-fm: the hit records of every chunk come from lamsa_hp_fm_seed (include/lamsa_hp.h): no mapper, no .gem index, no seed files,
    // no map text.  It needs the reference's FM index files and a library that has the call; there is no host seeding path.
    const bool seed_fm = opt.seed_fm != 0;
    FmIndex fm; bool fm_loaded = false;
    if (seed_fm) {
        if (lamsa_hp_fm_load == nullptr || lamsa_hp_fm_seed == nullptr) { fprintf(stderr, "[lamsa_aln] --seed-fm: this library has no lamsa_hp_fm_load / lamsa_hp_fm_seed\n"); return 2; }
        std::string e2;
        if (!fm.load(opt.ref_prefix, e2)) { fprintf(stderr, "[lamsa_aln] --seed-fm needs %s.bwt and %s.sa (lamsa index): %s\n", opt.ref_prefix.c_str(), opt.ref_prefix.c_str(), e2.c_str()); return 2; }
        fm_loaded = true;
    }
    if (from_hits) {
        HitsHeader hh;
        if (!hitsf.open(opt.hits) || hitsf.n < sizeof hh) { fprintf(stderr, "[lamsa_aln] Can't open hit stream %s\n", opt.hits.c_str()); return 1; }
        memcpy(&hh, hitsf.p, sizeof hh);
        if (memcmp(hh.magic, HITS_MAGIC, 8) != 0 || hh.read_type != P.read_type || hh.seed_len != P.seed_len || hh.seed_step != P.seed_step || hh.per_aln_m != P.per_aln_m) {
            fprintf(stderr, "[lamsa_aln] %s is not a hit stream written with these seeding options (-T, -l, -i, -p)\n", opt.hits.c_str()); return 1;
        }
        hitsf.pos = sizeof hh;
    } else if (seed_fm) {                               // (no seed result to open)
    } else if (opt.mapper_pid) { mapt.open_follow(map_path, opt.mapper_pid);
    } else if (!mapt.open(map_path)) { fprintf(stderr, "[lamsa_aln] Can't open seed-result file %s (seeding is not run by this build: provide the GEM map, as with the reference's -N)\n", map_path.c_str()); return 1; }
    FastxReader fx;
    if (!fx.open(opt.reads)) { fprintf(stderr, "[lamsa_aln] Can't open read file %s\n", opt.reads.c_str()); return 1; }
    // ---- --shard i/N (the read stream shards naturally; one process -- one parser -- per GPU).  This process
    // takes the i-th of N contiguous parts: a mapped read file is cut by bytes (no pass over the parts before it: the first read's
    // name finds its lines in the GEM map, whose lines begin "<read name>_<seed>:"), a compressed one by record count, a hit stream
    // by chunks.  Shards 0 .. N-1 written one after the other are the unsharded output; only shard 0 writes the header.
    long reads_left = -1, chunks_left = -1;                 // -1: no limit
    if (opt.shard_n > 1) {
        const int si = opt.shard_i, sn = opt.shard_n;
        if (opt.mapper_pid) { fprintf(stderr, "[lamsa_aln] --shard needs an existing seed result (-N or --hits): the shards would each run the seeding\n"); return 1; }
        if (from_hits) {
            std::vector<int64_t> n_in; std::vector<size_t> at;
            for (size_t q = hitsf.pos; q + sizeof(HitsChunkHeader) <= hitsf.n; ) {
                HitsChunkHeader ch; memcpy(&ch, hitsf.p + q, sizeof ch);
                if (ch.n_reads <= 0 || ch.bytes < 0 || q + sizeof ch + (size_t)ch.bytes > hitsf.n) { fprintf(stderr, "[lamsa_read_seq] damaged hit stream\n"); return 1; }
                n_in.push_back(ch.n_reads); at.push_back(q); q += sizeof ch + (size_t)ch.bytes;
            }
            const size_t C = n_in.size(), c0 = C * (size_t)si / (size_t)sn, c1 = C * (size_t)(si + 1) / (size_t)sn;
            int64_t skip = 0;
            for (size_t c = 0; c < c0; ++c) skip += n_in[c];
            Read d;
            for (int64_t k = 0; k < skip; ++k) if (!fx.next(d)) { fprintf(stderr, "[lamsa_read_seq] the hit stream does not match the reads\n"); return 1; }
            hitsf.pos = c0 < C ? at[c0] : hitsf.n;
            chunks_left = (long)(c1 - c0);
        } else if (fx.mapped()) {
            const size_t S = fx.size(), lo = S / (size_t)sn * (size_t)si, hi = si + 1 == sn ? S : S / (size_t)sn * (size_t)(si + 1);
            fx.restrict(lo, hi);
            if (si > 0 && !seed_fm) {
                FastxReader probe; Read first;
                if (probe.open(opt.reads)) probe.restrict(lo, hi);
                // the first read of the part that has seeds at all (a read shorter than a seed has no line in the map)
                bool have_first = probe.next(first);
                while (have_first && seeds_of(P, (int)first.seq.size()) == 0) have_first = probe.next(first);
                if (!have_first) mapt.pos = mapt.n;              // no record with seeds starts in this part: no map line is taken
                else {
                    std::string nm = first.name.substr(0, first.name.find_first_of(" \t"));
                    // the lines of a read's seeds are consecutive and begin "<read name>_<seed>:" (split_seed, src/lamsa_aln.c:287): the first
                    // of them at or after a guess of where this part begins, then back over the lines of the same read before it.  A line of
                    // ANOTHER read whose name merely begins with "<name>_" ("r1_2_0:0" for the read "r1") is told apart by what follows the
                    // key: digits, then a colon (or the end of the name).
                    const std::string key = "\n" + nm + "_";
                    auto is_seed_line = [&](const char *q) {       // q: just behind "<name>_"
                        const char *e = mapt.p + mapt.n, *d = q;
                        while (d < e && *d >= '0' && *d <= '9') ++d;
                        return d > q && d < e && (*d == ':' || *d == '\t' || *d == ' ');       // "<name>_<seed>:<offset>" as split_seed writes it; a mapper may cut the name at the colon
                    };
                    auto find_from = [&](size_t from) -> const char * {
                        while (from < mapt.n) {
                            const char *h = (const char *)memmem(mapt.p + from, mapt.n - from, key.data(), key.size());
                            if (!h) return nullptr;
                            if (is_seed_line(h + key.size())) return h;
                            from = (size_t)(h - mapt.p) + 1;
                        }
                        return nullptr;
                    };
                    const size_t est = (size_t)((double)mapt.n * ((double)lo / (double)(S ? S : 1)));
                    const size_t from = est > (mapt.n >> 3) ? est - (mapt.n >> 3) : 0;
                    const char *hit = find_from(from);
                    if (!hit && from) hit = find_from(0);
                    if (!hit && mapt.n >= key.size() - 1 && memcmp(mapt.p, key.data() + 1, key.size() - 1) == 0 && is_seed_line(mapt.p + key.size() - 1)) hit = mapt.p - 1;      // the very first line
                    if (!hit) { fprintf(stderr, "[lamsa_aln] --shard %d/%d: no line of %s begins with %s_<seed>: (the seeds of the shard's first read)\n", si, sn, map_path.c_str(), nm.c_str()); return 1; }
                    size_t at = (size_t)(hit + 1 - mapt.p);
                    while (at > 1) {                            // the line before `at`: does it belong to the same read?
                        const char *pe = mapt.p + at - 1;       // its newline
                        const char *ps = (const char *)memrchr(mapt.p, '\n', (size_t)(pe - mapt.p));
                        const size_t b = ps ? (size_t)(ps - mapt.p) + 1 : 0;
                        if (at - 1 - b >= key.size() - 1 && memcmp(mapt.p + b, key.data() + 1, key.size() - 1) == 0 && is_seed_line(mapt.p + b + key.size() - 1)) at = b; else break;
                    }
                    mapt.pos = at;
                }
            }
        } else {                                            // compressed reads: count the records, then skip to this shard's first
            long total = 0; { FastxReader cnt; Read d; if (cnt.open(opt.reads)) while (cnt.next(d)) ++total; }
            const long r0 = total * si / sn, r1 = total * (si + 1) / sn;
            Read d; const char *la, *lb;
            for (long k = 0; k < r0; ++k) {
                if (!fx.next(d) || (!seed_fm && !mapt.take(seeds_of(P, (int)d.seq.size()), la, lb))) { fprintf(stderr, "[lamsa_read_seq] seeds' GEM map result does not match the reads\n"); return 1; }
            }
            reads_left = r1 - r0;
        }
    }
    lamsa_hp_ref ref; ref.pac = ix.pac.data(); ref.l_pac = ix.l_pac; ref.n_seqs = (int32_t)ix.name.size(); ref.seq_offset = ix.off.data(); ref.seq_len = ix.len.data();
    // one handle per GPU: the read stream is dealt out chunk by chunk, the reference is resident on
    // every device, nothing is exchanged between devices
    std::vector<int> devs = opt.devices.empty() ? std::vector<int>(1, opt.device) : opt.devices;
    std::vector<lamsa_hp_handle *> hs;
    int rc = LAMSA_HP_OK;
    for (size_t g = 0; g < devs.size() && rc == LAMSA_HP_OK && !opt.parse_only; ++g) { lamsa_hp_handle *hh = nullptr; rc = lamsa_hp_create(&hh, &P, &ref, devs[g]); if (rc == LAMSA_HP_OK) hs.push_back(hh); }
    if (rc != LAMSA_HP_OK) for (lamsa_hp_handle *hh : hs) lamsa_hp_destroy(hh);
    const int G = (int)std::max<size_t>(1, hs.size());
    if (rc != LAMSA_HP_OK) { fprintf(stderr, "[lamsa_aln] no usable MI355X / HIP device (lamsa_hp_create: %d); this build has no CPU path\n", rc); return 2; }
    // --MD, --cs: every handle lists the mismatches of its records in the result stream; --eqx: it writes the CIGARs in =/X form;
    // --left-align: it shifts the gaps before it counts.  --paf: every handle ships a record's 15-word summary in place of its CIGAR
    // (--left-align changes no word of it and is not passed on).  What the output needs of every record is `fin_all` (rec_finish); what
    // the device has done of it the host leaves out for rounds 1 and 2 (`what`) -- nothing against a library without
    // lamsa_hp_set_result_tags, where the host does it all -- and the stage-4 records, made on the host, get all of it (rescue_finish).
    const bool need_mm = opt.tag_md || opt.tag_cs, paf_any = opt.paf || opt.paf_cg, have_tags = lamsa_hp_set_result_tags != nullptr;
    const int dev_tags = !have_tags ? 0 : opt.paf ? LAMSA_HP_TAG_SUMMARY :
                         (need_mm ? LAMSA_HP_TAG_MISMATCHES : 0) | (opt.tag_eqx ? LAMSA_HP_TAG_EQX : 0) | (opt.left_align ? LAMSA_HP_TAG_LEFT_ALIGN : 0);
    const int fin_all = (opt.left_align && !opt.paf ? FIN_LEFT_ALIGN : 0) | (need_mm || opt.tag_eqx ? FIN_AUX : 0) | (opt.tag_eqx ? FIN_EQX : 0) | (paf_any ? FIN_SUMMARY : 0);
    const int what = fin_all & ~((have_tags ? FIN_AUX : 0) | ((dev_tags & LAMSA_HP_TAG_LEFT_ALIGN) ? FIN_LEFT_ALIGN : 0) | ((dev_tags & LAMSA_HP_TAG_EQX) ? FIN_EQX : 0) |
                                 ((dev_tags & LAMSA_HP_TAG_SUMMARY) ? FIN_SUMMARY : 0));
    for (lamsa_hp_handle *hh : hs) {
        if (!dev_tags) break;
        const int e = lamsa_hp_set_result_tags(hh, dev_tags);
        if (e != LAMSA_HP_OK) { fprintf(stderr, "[lamsa_aln] lamsa_hp_set_result_tags failed: %d %s\n", e, lamsa_hp_last_error(hh)); for (lamsa_hp_handle *x : hs) lamsa_hp_destroy(x); return 2; }
    }
    // stage (4): needs the reference's FM index files and a second handle for its DP batches (a handle is single-threaded)
    lamsa_hp_handle *h_dp = nullptr; bool rescue = false; long n_rescue_jobs = 0, n_rescue_kmers = 0;
    if (P.bwt_max_len > 0 && !opt.parse_only) {
        std::string e2;
        if (!fm_loaded && !fm.load(opt.ref_prefix, e2)) fprintf(stderr, "[lamsa_aln] note: stage 4 (BWT rescue of uncovered regions <= -R %d bp) is skipped: %s; output equals the reference's with -R 0\n", P.bwt_max_len, e2.c_str());
        else if (lamsa_hp_create(&h_dp, &P, nullptr, devs[0]) != LAMSA_HP_OK) { fprintf(stderr, "[lamsa_aln] cannot create the stage-4 handle\n"); for (lamsa_hp_handle *hh : hs) lamsa_hp_destroy(hh); return 2; }
        else rescue = true;
    }
    // --rescue-gpu: the index goes into the stage-4 handle once; every chunk's windows are then searched there in one call
    lamsa_hp_fm_index fmx; memset(&fmx, 0, sizeof fmx);
    if (fm_loaded || rescue) {
        fmx.seq_len = fm.seq_len; fmx.primary = fm.primary; for (int c = 0; c < 5; ++c) fmx.L2[c] = fm.L2[c];
        fmx.bwt = fm.bwt.data(); fmx.bwt_words = (uint64_t)fm.bwt.size() - 4; fmx.sa = fm.sa.data(); fmx.n_sa = fm.n_sa; fmx.sa_intv = fm.sa_intv;      // (FmIndex::load keeps 4 spare words)
    }
    // --seed-fm: a handle of its own per device for the seeding calls, the index loaded into it once: a handle is single-threaded, and a chunk
    // is seeded beside the kernels and beside stage 4 of earlier chunks.  With --rescue-gpu too, stage 4 searches in the seeding handle of its
    // device, one call at a time (fm_m), so that the device holds the index once.
    std::map<int, lamsa_hp_handle *> seed_h; std::mutex fm_m; long n_seeded = 0; double seed_s = 0, seed_kernel_ms = 0;
    auto destroy_seed_handles = [&]() { for (auto &kv : seed_h) lamsa_hp_destroy(kv.second); seed_h.clear(); };
    for (size_t g = 0; seed_fm && g < devs.size(); ++g) {
        if (seed_h.count(devs[g])) continue;
        lamsa_hp_handle *hh = nullptr;
        int e = lamsa_hp_create(&hh, &P, nullptr, devs[g]);
        if (e == LAMSA_HP_OK) { seed_h[devs[g]] = hh; e = lamsa_hp_fm_load(hh, &fmx); }
        if (e != LAMSA_HP_OK) {
            fprintf(stderr, "[lamsa_aln] --seed-fm: cannot put the FM index on device %d: %d %s\n", devs[g], e, hh ? lamsa_hp_last_error(hh) : "no usable MI355X / HIP device");
            destroy_seed_handles(); if (h_dp) lamsa_hp_destroy(h_dp); for (lamsa_hp_handle *x : hs) lamsa_hp_destroy(x); return 2;
        }
    }
    lamsa_hp_handle *h_fm = h_dp;                          // where stage 4 searches
    bool rescue_gpu = false;
    if (rescue && opt.rescue_gpu) {
        if (lamsa_hp_fm_load == nullptr || lamsa_hp_fm_search == nullptr) fprintf(stderr, "[lamsa_aln] note: --rescue-gpu: this library has no lamsa_hp_fm_load / lamsa_hp_fm_search; stage 4 searches on the host\n");
        else if (seed_fm) { h_fm = seed_h[devs[0]]; rescue_gpu = true; }
        else {
            const int e = lamsa_hp_fm_load(h_dp, &fmx);
            if (e != LAMSA_HP_OK) { fprintf(stderr, "[lamsa_aln] lamsa_hp_fm_load failed: %d %s\n", e, lamsa_hp_last_error(h_dp)); lamsa_hp_destroy(h_dp); for (lamsa_hp_handle *hh : hs) lamsa_hp_destroy(hh); return 2; }
            rescue_gpu = true;
        }
    }
    const double load_s = now_s() - t_begin;
    std::string sam;
    sam_header(sam, ix, pg_line);
    if (opt.shard_i == 0 && !paf_any) fwrite(sam.data(), 1, sam.size(), out);              // (PAF has no header)
    long n_reads = 0, n_bases = 0, n_bad = 0; double kernel_ms = 0;
    const int threads = opt.n_thread > 0 ? opt.n_thread : 1;
    bool eof = false; int ret = 0;
    // One chunk = reads + their hit records, ready for the GPU.  Four stages overlap: the sequential pass over the
    // input files that cuts the next chunk (reads + the line span of every read in the mapped GEM file), the parse of
    // the chunk before it on all host threads, the GPU on the one before that, and the SAM text of the oldest.
    // The chunk buffers are recycled.
    struct Chunk { Batch B; int ret = 0; std::vector<std::pair<const char *, const char *>> span; std::vector<std::pair<size_t, size_t>> rspan; std::vector<std::string> text; bool mapped = false; lamsa_hp_batch hb; int dev = 0;
                   int sub_rc = 0, col_rc = 0; lamsa_hp_result res; std::promise<void> collected; };
    // One worker thread per device runs that device's submit / collect calls in the order they are queued (a handle is not
    // thread-safe, and the copies of a submit block their caller): the uploads of different devices then run side by side.
    struct DevQ {
        std::thread th; std::mutex m; std::condition_variable cv; std::deque<std::function<void()>> ops; bool stop = false;
        void finish() { { std::lock_guard<std::mutex> lk(m); stop = true; } cv.notify_one(); if (th.joinable()) th.join(); }   // runs what is queued, then ends
        ~DevQ() { finish(); }                                   // every way out of run_aln (--parse-only, errors) ends the thread
    };
    std::mutex stat_m;
    HitsWriter saver;
    if (!opt.save_hits.empty() && !from_hits && !saver.open(opt.save_hits, P)) { fprintf(stderr, "[lamsa_aln] Can't write hit stream %s\n", opt.save_hits.c_str()); return 1; }
    std::vector<Chunk> pool((size_t)2 * G + 6); int n_scanned = 0;  // scanning, parsing, submitted (2 per device), being written, slack
    std::vector<Batch> parts((size_t)threads);              // per-thread partial batches of the parse, recycled too
    const bool trace = getenv("LAMSA_TRACE") != nullptr;
    auto scan = [&]() -> Chunk * {                          // sequential: FASTA/FASTQ records and their seed_all map lines
        Chunk *c = &pool[(size_t)(n_scanned++ % (2 * G + 6))];
        Batch &B = c->B;
        B.clear(); c->ret = 0; c->span.clear(); c->rspan.clear(); c->text.clear(); c->mapped = false;
        if (eof) return c;
        const double t0 = now_s();
        Read rd;
        int64_t chunk_bases = 0;
        if (from_hits) {                                    // the chunk as it was stored: its arrays are views into the mapped stream
            if (chunks_left == 0) { eof = true; return c; }
            if (chunks_left > 0) --chunks_left;
            if (hitsf.pos + sizeof(HitsChunkHeader) > hitsf.n) { eof = true; if (opt.shard_n <= 1 && fx.next(rd)) { fprintf(stderr, "[lamsa_read_seq] the hit stream ends before the reads\n"); c->ret = 1; } return c; }
            HitsChunkHeader ch; memcpy(&ch, hitsf.p + hitsf.pos, sizeof ch);
            const char *a = hitsf.p + hitsf.pos + sizeof ch;
            if (ch.n_reads <= 0 || ch.bytes < 0 || hitsf.pos + sizeof ch + (size_t)ch.bytes > hitsf.n) { fprintf(stderr, "[lamsa_read_seq] damaged hit stream\n"); c->ret = 1; eof = true; return c; }
            const size_t n = (size_t)ch.n_reads, nb = (size_t)ch.n_bases, ns = (size_t)ch.n_slots, nh = (size_t)ch.n_hits, nc = (size_t)ch.n_cig;
            lamsa_hp_batch &hb = c->hb;
            auto take = [&](size_t bytes) { const char *q = a; a += pad64(bytes); return q; };
            hb.n_reads = (int32_t)n; hb.n_cig = (int64_t)nc;
            hb.read_off = (const int64_t *)take(8 * (n + 1)); hb.read_seq = (const uint8_t *)take(nb); hb.seed_all = (const int32_t *)take(4 * n); hb.last_len = (const int32_t *)take(4 * n);
            hb.seed_off = (const int64_t *)take(8 * (n + 1)); hb.seed_id = (const int32_t *)take(4 * ns); hb.hit_off = (const int64_t *)take(8 * (ns + 1));
            hb.h_pos = (const int64_t *)take(8 * nh); hb.h_chr = (const int32_t *)take(4 * nh); hb.h_strand = (const int8_t *)take(nh); hb.h_nm = (const int16_t *)take(2 * nh);
            hb.h_len_dif = (const int16_t *)take(2 * nh); hb.h_cig_n = (const uint8_t *)take(nh);
            if (ch.cig_elem == 4) { hb.h_cig_off = (const int32_t *)take(4 * nh); hb.cig = (const int32_t *)take(4 * nc); hb.cig8 = nullptr; }
            else { hb.h_cig_off = nullptr; hb.cig = nullptr; hb.cig8 = (const uint8_t *)take(nc); }
            if ((size_t)(a - (hitsf.p + hitsf.pos + sizeof ch)) != (size_t)ch.bytes) { fprintf(stderr, "[lamsa_read_seq] damaged hit stream\n"); c->ret = 1; eof = true; return c; }
            {   // The chunk's pages of the mapping, touched by all threads now: a page of a file mapping costs a fault the first time it is read, and the
                // upload (one thread's copy into the runtime's page-locked staging buffers) otherwise pays 230 000 of them per chunk, one after the other.
                const char *p0 = hitsf.p + hitsf.pos; const size_t np = (sizeof ch + (size_t)ch.bytes + 4095) / 4096;
                static std::atomic<unsigned> sink(0);
                parallel_blocks((int)np, threads, [&](int, int b0, int b1) { unsigned v = 0; for (int k = b0; k < b1; ++k) v += (unsigned char)p0[(size_t)k * 4096]; sink += v; });
            }
            hitsf.pos += sizeof ch + (size_t)ch.bytes;
            if (fx.spans()) {                               // only where the records lie: they are parsed by all threads (prepare)
                c->rspan.resize(n);
                for (size_t r = 0; r < n; ++r)
                    if (!fx.next_span(c->rspan[r].first, c->rspan[r].second)) { fprintf(stderr, "[lamsa_read_seq] the hit stream does not match the reads\n"); c->ret = 1; eof = true; return c; }
                B.reads.resize(n);
            } else for (size_t r = 0; r < n; ++r) {
                if (!fx.next(rd) || (int64_t)rd.seq.size() != hb.read_off[r + 1] - hb.read_off[r]) { fprintf(stderr, "[lamsa_read_seq] the hit stream does not match the reads\n"); c->ret = 1; eof = true; return c; }
                B.reads.emplace_back(); std::swap(B.reads.back(), rd);
            }
            c->mapped = true;
            if (trace) fprintf(stderr, "[scan] %d reads of the hit stream in %.3f s\n", (int)n, now_s() - t0);
            return c;
        }
        while ((int)B.reads.size() < opt.chunk_reads && chunk_bases < opt.chunk_bases) {
            if (reads_left == 0) { eof = true; break; }
            if (reads_left > 0) --reads_left;
            if (!fx.next(rd)) {
                eof = true;
                if (mapt.following()) {                      // the reads are through: the mapper must have ended, and ended well
                    if (!mapt.follow_finish()) { fprintf(stderr, "[lamsa_aln] Seeding undone, gem-mapper exit abnormally.\n"); c->ret = 1; B.clear(); return c; }
                    fprintf(stderr, "[lamsa_aln] gem-mapper done!\n");
                }
                break;
            }
            const char *la = nullptr, *lb = nullptr;
            bool got;
            if (seed_fm) got = true;                         // no map lines: prepare() seeds the chunk on the GPU
            else if (mapt.following()) {
                if (c->text.capacity() < (size_t)opt.chunk_reads + 1) c->text.reserve((size_t)opt.chunk_reads + 1);      // no reallocation: the spans point into the strings
                c->text.emplace_back();
                got = mapt.take_follow(seeds_of(P, (int)rd.seq.size()), c->text.back());
                la = c->text.back().data(); lb = la + c->text.back().size();
            } else got = mapt.take(seeds_of(P, (int)rd.seq.size()), la, lb);
            if (!got) { fprintf(stderr, "[lamsa_read_seq] seeds' GEM map result does not match the reads\n"); c->ret = 1; eof = true; return c; }
            c->span.emplace_back(la, lb);
            chunk_bases += (int64_t)rd.seq.size();
            B.reads.emplace_back(); std::swap(B.reads.back(), rd);
        }
        if (trace) fprintf(stderr, "[scan] %d reads in %.3f s\n", (int)B.reads.size(), now_s() - t0);
        return c;
    };
    std::future<Chunk *> scanned = std::async(std::launch::async, scan);
    // Device buffers (scratch slabs, inter-launch state, input / output: tens of GB) are allocated while the first chunk is being
    // parsed, sized from that chunk, instead of inside the first submit.
    std::thread reserver; double reserve_s = 0; bool reserve_started = false;
    auto prepare = [&]() -> Chunk * {
        const double t0 = now_s();
        Chunk *c = scanned.get();
        scanned = std::async(std::launch::async, scan);      // the following chunk is cut while this one is parsed
        Batch &B = c->B;
        const int n = (int)B.reads.size();
        if (n == 0 || c->ret) return c;
        if (!reserve_started && !opt.parse_only && !hs.empty()) {
            reserve_started = true;
            int64_t nb = 0; int max_len = 0;
            if (c->mapped) { for (int r = 0; r < n; ++r) { const int len = (int)(c->hb.read_off[r + 1] - c->hb.read_off[r]); nb += len; max_len = std::max(max_len, len); } }     // (the records of a chunk of the hit stream may not be parsed yet)
            else for (const Read &rd : B.reads) { nb += (int64_t)rd.seq.size(); max_len = std::max(max_len, (int)rd.seq.size()); }
            const int32_t r_n = (int32_t)std::max(n, opt.chunk_reads > n ? std::min(opt.chunk_reads, 2 * n) : n);
            const int64_t r_nb = nb + nb / 4 + 4096;
            reserver = std::thread([&hs, &reserve_s, r_n, r_nb, max_len]() {
                const double t = now_s();
                for (lamsa_hp_handle *hh : hs) {
                    const int e = lamsa_hp_reserve(hh, r_n, r_nb, r_nb / 3, 3 * r_nb, max_len + max_len / 4 + 256, 8192);
                    if (e != LAMSA_HP_OK) fprintf(stderr, "[lamsa_aln] note: device buffers could not be reserved ahead (%d %s); the first batch allocates what it needs\n", e, lamsa_hp_last_error(hh));
                }
                reserve_s = now_s() - t;
            });
        }
        if (c->mapped) {
            if (!c->rspan.empty()) {                        // the records of a chunk of the hit stream, parsed side by side
                std::vector<int> bad((size_t)threads, 0);
                parallel_blocks(n, threads, [&](int t, int r0, int r1) {
                    for (int r = r0; r < r1; ++r)
                        if (!fx.parse_span(c->rspan[(size_t)r].first, c->rspan[(size_t)r].second, B.reads[(size_t)r]) || (int64_t)B.reads[(size_t)r].seq.size() != c->hb.read_off[r + 1] - c->hb.read_off[r]) bad[(size_t)t] = 1;
                });
                for (int b : bad) if (b) { fprintf(stderr, "[lamsa_read_seq] the hit stream does not match the reads\n"); c->ret = 1; break; }
            }
            parse_s += now_s() - t0; return c;
        }
        if (seed_fm) {
            // reads -> base codes on all threads, then one lamsa_hp_fm_seed on the seeding handle of the device the chunk will go to; its batch
            // is the handle's until the next seeding call, so it is copied into the chunk's arrays, which then go the way parsed ones go
            B.read_off.resize((size_t)n + 1); B.read_off[0] = 0;
            for (int r = 0; r < n; ++r) B.read_off[(size_t)r + 1] = B.read_off[(size_t)r] + (int64_t)B.reads[(size_t)r].seq.size();
            B.read_seq.resize((size_t)B.read_off[(size_t)n]);
            const uint8_t *t4 = nt4_table();
            parallel_blocks(n, threads, [&](int, int r0, int r1) {
                for (int r = r0; r < r1; ++r) { const std::string &s = B.reads[(size_t)r].seq; uint8_t *d = B.read_seq.data() + B.read_off[(size_t)r]; for (size_t i = 0; i < s.size(); ++i) d[i] = t4[(unsigned char)s[i]]; }
            });
            static const uint8_t zero8 = 0;
            lamsa_hp_seed_queries sq; memset(&sq, 0, sizeof sq);
            sq.n_reads = n; sq.read_off = B.read_off.data(); sq.read_seq = B.read_seq.empty() ? &zero8 : B.read_seq.data();
            sq.seed_len = P.seed_len; sq.seed_step = P.seed_step; sq.max_hits = P.per_aln_m;
            sq.n_seqs = (int32_t)ix.off.size(); sq.seq_offset = ix.off.data(); sq.seq_len = ix.len.data();
            lamsa_hp_batch sb; memset(&sb, 0, sizeof sb);
            lamsa_hp_handle *hsd = seed_h[devs[(size_t)(n_seeded++ % (long)devs.size())]];
            const double t1 = now_s();
            int e;
            { std::lock_guard<std::mutex> lk(fm_m); e = lamsa_hp_fm_seed(hsd, &sq, &sb); if (e == LAMSA_HP_OK) seed_kernel_ms += lamsa_hp_last_kernel_ms(hsd, 21) + lamsa_hp_last_kernel_ms(hsd, 22) + lamsa_hp_last_kernel_ms(hsd, 23); }
            if (e != LAMSA_HP_OK) { fprintf(stderr, "[lamsa_aln] lamsa_hp_fm_seed failed: %d %s\n", e, lamsa_hp_last_error(hsd)); c->ret = 2; return c; }
            const size_t ns = (size_t)sb.seed_off[n], nh = (size_t)sb.hit_off[ns];
            B.seed_all.assign(sb.seed_all, sb.seed_all + n); B.last_len.assign(sb.last_len, sb.last_len + n); B.seed_off.assign(sb.seed_off, sb.seed_off + n + 1);
            B.seed_id.assign(sb.seed_id, sb.seed_id + ns); B.hit_off.assign(sb.hit_off, sb.hit_off + ns + 1);
            B.h_pos.assign(sb.h_pos, sb.h_pos + nh); B.h_chr.assign(sb.h_chr, sb.h_chr + nh); B.h_strand.assign(sb.h_strand, sb.h_strand + nh);
            B.h_nm.assign(sb.h_nm, sb.h_nm + nh); B.h_len_dif.assign(sb.h_len_dif, sb.h_len_dif + nh); B.h_cig_n.assign(sb.h_cig_n, sb.h_cig_n + nh);
            B.cig8.assign(sb.cig8, sb.cig8 + (size_t)sb.n_cig); B.cig_wide = false;
            seed_s += now_s() - t1;
            if (trace) fprintf(stderr, "[prepare] %d reads seeded in the FM index in %.3f s: %zu slots, %zu hits\n", n, now_s() - t1, ns, nh);
            if (saver.fp && !saver.write(B)) { fprintf(stderr, "[lamsa_aln] writing %s failed\n", opt.save_hits.c_str()); c->ret = 1; }
            parse_s += now_s() - t0;
            return c;
        }
        const double t1 = now_s();
        // text -> hit records (gem_map_msg / map_cal_msg run inside the worker threads in the reference too)
        // The seed CIGARs are written in the boundary's compact form (a byte per element) as they are parsed; a chunk in which an element
        // does not fit a byte (longer than 63 -- no 50-base seed has one) is parsed once more into words.
        static const bool words_only = getenv("LAMSA_WIDE_CIGARS") != nullptr;      // tests: every chunk through the word form
        for (int pass = words_only ? 1 : 0; pass < 2; ++pass) {
            for (Batch &p : parts) { p.clear(); p.parse_compact = pass == 0; }
            parallel_blocks(n, threads, [&](int t, int r0, int r1) {
                for (int r = r0; r < r1; ++r) append_read_lines(parts[(size_t)t], ix, P, B.reads[(size_t)r], c->span[(size_t)r].first, c->span[(size_t)r].second, seeds_of(P, (int)B.reads[(size_t)r].seq.size()));
            });
            bool wide = false;
            for (const Batch &p : parts) wide |= p.saw_wide;
            if (!wide) break;
        }
        const double t2 = now_s();
        merge_batches(B, parts, threads);
        if (trace) fprintf(stderr, "[prepare] waited %.3f s for the scan, parse %.3f, merge %.3f\n", t1 - t0, t2 - t1, now_s() - t2);
        for (int32_t ch : B.h_chr) if (ch < 1) { fprintf(stderr, "[lamsa_aln] seed hit on a contig that is not in the index\n"); c->ret = 1; break; }
        if (saver.fp && !c->ret && !saver.write(B)) { fprintf(stderr, "[lamsa_aln] writing %s failed\n", opt.save_hits.c_str()); c->ret = 1; }
        parse_s += now_s() - t0;                            // one prepare() runs at a time
        return c;
    };
    std::vector<std::unique_ptr<DevQ>> devq;
    for (int g = 0; g < G; ++g) {
        devq.emplace_back(new DevQ);
        DevQ *q = devq.back().get();
        q->th = std::thread([q]() {
            for (;;) {
                std::function<void()> op;
                { std::unique_lock<std::mutex> lk(q->m); q->cv.wait(lk, [q] { return q->stop || !q->ops.empty(); }); if (q->ops.empty()) return; op = std::move(q->ops.front()); q->ops.pop_front(); }
                op();
            }
        });
    }
    auto enqueue = [&](int dev, std::function<void()> op) { DevQ *q = devq[(size_t)dev].get(); { std::lock_guard<std::mutex> lk(q->m); q->ops.push_back(std::move(op)); } q->cv.notify_one(); };
    auto stop_workers = [&]() { for (auto &q : devq) q->finish(); };
    long n_submitted = 0;
    auto submit = [&](Chunk &ck) -> int {
        Batch &B = ck.B;
        lamsa_hp_batch hb;
        if (ck.mapped) hb = ck.hb;
        else {
        hb.n_reads = (int32_t)B.reads.size(); hb.read_off = B.read_off.data(); hb.read_seq = B.read_seq.data(); hb.seed_all = B.seed_all.data(); hb.last_len = B.last_len.data();
        hb.seed_off = B.seed_off.data(); hb.seed_id = B.seed_id.data(); hb.hit_off = B.hit_off.data(); hb.h_pos = B.h_pos.data(); hb.h_chr = B.h_chr.data(); hb.h_strand = B.h_strand.data();
        hb.h_nm = B.h_nm.data(); hb.h_len_dif = B.h_len_dif.data(); hb.h_cig_n = B.h_cig_n.data(); hb.n_cig = (int64_t)B.cig8.size();
        if (B.cig_wide) { hb.h_cig_off = B.h_cig_off.data(); hb.cig = B.cig.data(); hb.cig8 = nullptr; }
        else { hb.h_cig_off = nullptr; hb.cig = nullptr; hb.cig8 = B.cig8.data(); }                 // compact form: a quarter of the CIGAR bytes, no offsets
        static const int32_t zero32 = 0; static const uint8_t zero8 = 0; static const int64_t zero64 = 0; static const int16_t zero16 = 0; static const int8_t zeroi8 = 0;
        if (!hb.seed_id) hb.seed_id = &zero32;
        if (!hb.h_pos) { hb.h_pos = &zero64; hb.h_chr = &zero32; hb.h_strand = &zeroi8; hb.h_nm = &zero16; hb.h_len_dif = &zero16; hb.h_cig_n = &zero8; }
        if (B.cig_wide && !hb.cig) hb.cig = &zero32;
        if (!B.cig_wide && !hb.cig8) hb.cig8 = &zero8;
        if (!hb.read_seq) hb.read_seq = &zero8;
        }
        const double t0 = now_s();
        const int e = lamsa_hp_submit_batch(hs[(size_t)ck.dev], &hb);
        { std::lock_guard<std::mutex> lk(stat_m); submit_s += now_s() - t0; }
        if (e != LAMSA_HP_OK) { fprintf(stderr, "[lamsa_aln] lamsa_hp_submit_batch failed: %d %s\n", e, lamsa_hp_last_error(hs[(size_t)ck.dev])); return 2; }
        return 0;
    };
    // records -> MAPQ / XA -> SAM text, on all host threads; written in input order
    // Everything after the GPU for one chunk: result streams -> records, stage (4) (rescue.h: plan on the host threads,
    // one DP batch on the GPU through the second handle, finish on the host threads), MAPQ / XA, SAM text in input order.
    // It runs as a task of its own beside the next collect; `res` stays valid until the collect after that.
    // The SAM text of a chunk, a part per thread, and the records it is made from: kept from chunk to chunk (one write_chunk runs at a time), so
    // their pages are touched and their vectors allocated once.  Two sets of text buffers: while the parts of chunk i are being written into the
    // file (pwrite, every thread its own part at its own offset) the text of chunk i + 1 is made in the other set.
    std::vector<std::string> sams_set[2] = {std::vector<std::string>((size_t)threads), std::vector<std::string>((size_t)threads)};
    std::future<int> file_write[2];
    int sams_turn = 0;
    off_t out_at = -1;                                        // where the next chunk goes in the output file (-1: not a regular file, or not asked yet)
    std::vector<ReadResult> RR;
    auto write_chunk = [&](Chunk *ck, lamsa_hp_result res) -> int {
        const double t1 = now_s();
        Batch &B = ck->B;
        const int n = (int)B.reads.size();
        const uint8_t *codes = ck->mapped ? ck->hb.read_seq : B.read_seq.data();
        const int64_t *roff = ck->mapped ? ck->hb.read_off : B.read_off.data();
        if (RR.size() < (size_t)n) RR.resize((size_t)n);
        std::vector<RescuePlan> plans(rescue ? (size_t)n : 0);
        std::vector<RescueJobs> tj((size_t)threads);
        std::vector<RescueWindows> tw(rescue_gpu ? (size_t)threads : 0);      // --rescue-gpu: the windows every thread lists
        std::vector<int> t_first((size_t)threads, 0), t_last((size_t)threads, 0);
        std::vector<long> bad_of((size_t)threads, 0);
        parallel_blocks(n, threads, [&](int t, int r0, int r1) {
            t_first[(size_t)t] = r0; t_last[(size_t)t] = r1;
            for (int r = r0; r < r1; ++r) {
                ReadResult &R = RR[(size_t)r];
                const int L = (int)B.reads[(size_t)r].seq.size();
                parse_stream(res.stream + res.read_off[r], res.read_len[r], L, R, dev_tags);
                read_finish(R, codes + roff[r], L, ix, what);
                if (rescue && R.status == 0 && !rescue_gpu) rescue_plan(R, codes + roff[r], L, ix, fm, P, plans[(size_t)r], tj[(size_t)t]);
                else if (rescue && R.status == 0) rescue_windows(R, codes + roff[r], L, P, plans[(size_t)r], tw[(size_t)t]);
            }
        });
        if (rescue_gpu) {
            // the windows of all threads as one search on the stage-4 handle, then seeds -> chains -> jobs on the threads again
            std::vector<int64_t> wbase((size_t)threads + 1, 0);
            RescueWindows all;
            all.win_off.push_back(0);
            for (int t = 0; t < threads; ++t) {
                const RescueWindows &w = tw[(size_t)t];
                const int64_t s0 = (int64_t)all.seq.size();
                for (size_t k = 1; k < w.win_off.size(); ++k) all.win_off.push_back(w.win_off[k] + s0);
                all.seq.insert(all.seq.end(), w.seq.begin(), w.seq.end());
                wbase[(size_t)t + 1] = (int64_t)all.win_off.size() - 1;
            }
            lamsa_hp_fm_queries fq; memset(&fq, 0, sizeof fq);
            fq.n_win = (int32_t)(all.win_off.size() - 1); fq.seq = all.seq.data(); fq.seq_bytes = (int64_t)all.seq.size(); fq.win_off = all.win_off.data();
            fq.k = P.bwt_seed_len; fq.max_occ = 500;                        // 5 * MAX_HIT (rescue.cpp): a seed with more rows is not located
            lamsa_hp_fm_out found; memset(&found, 0, sizeof found);
            int e;
            { std::unique_lock<std::mutex> lk(fm_m, std::defer_lock); if (seed_fm) lk.lock(); e = lamsa_hp_fm_search(h_fm, &fq, &found); }      // (the answers are the handle's until its next search: a seeding call leaves them alone)
            if (e != LAMSA_HP_OK) { fprintf(stderr, "[lamsa_aln] lamsa_hp_fm_search (stage 4) failed: %d %s\n", e, lamsa_hp_last_error(h_fm)); return 2; }
            n_rescue_kmers += found.n_kmers;
            std::atomic<int> bad_found(0);
            parallel_blocks(n, threads, [&](int t, int r0, int r1) {
                for (int r = r0; r < r1; ++r) {
                    const ReadResult &R = RR[(size_t)r];
                    if (R.status != 0) continue;
                    if (!rescue_plan_found(codes + roff[r], (int)B.reads[(size_t)r].seq.size(), ix, found, wbase[(size_t)t], P, plans[(size_t)r], tj[(size_t)t])) bad_found = 1;
                }
            });
            if (bad_found.load()) { fprintf(stderr, "[lamsa_aln] lamsa_hp_fm_search (stage 4) answered other windows than it was asked\n"); return 2; }
        }
        const double t2 = now_s();
        // the DP jobs of all threads as one batch
        std::vector<int64_t> base((size_t)threads + 1, 0);
        for (int t = 0; t < threads; ++t) base[(size_t)t + 1] = base[(size_t)t] + (int64_t)tj[(size_t)t].qlen.size();
        lamsa_hp_dp_out dpo; memset(&dpo, 0, sizeof dpo);
        if (base[(size_t)threads] > 0) {
            RescueJobs all;
            for (int t = 0; t < threads; ++t) {
                const RescueJobs &j = tj[(size_t)t];
                const int64_t s0 = (int64_t)all.seq.size();
                all.seq.insert(all.seq.end(), j.seq.begin(), j.seq.end());
                for (size_t k = 0; k < j.qlen.size(); ++k) { all.q_off.push_back(j.q_off[k] + s0); all.t_off.push_back(j.t_off[k] + s0); }
                all.qlen.insert(all.qlen.end(), j.qlen.begin(), j.qlen.end()); all.tlen.insert(all.tlen.end(), j.tlen.begin(), j.tlen.end());
                all.kind.insert(all.kind.end(), j.kind.begin(), j.kind.end()); all.w.insert(all.w.end(), j.w.begin(), j.w.end()); all.h0.insert(all.h0.end(), j.h0.begin(), j.h0.end());
            }
            all.seq.resize(all.seq.size() + 16, 0);
            lamsa_hp_dp_jobs dj;
            dj.n_jobs = (int32_t)all.qlen.size(); dj.seq = all.seq.data(); dj.seq_bytes = (int64_t)all.seq.size(); dj.q_off = all.q_off.data(); dj.qlen = all.qlen.data();
            dj.t_off = all.t_off.data(); dj.tlen = all.tlen.data(); dj.kind = all.kind.data(); dj.w = all.w.data(); dj.h0 = all.h0.data();
            const int e = lamsa_hp_dp_batch(h_dp, &dj, &dpo);
            if (e != LAMSA_HP_OK) { fprintf(stderr, "[lamsa_aln] lamsa_hp_dp_batch (stage 4) failed: %d %s\n", e, lamsa_hp_last_error(h_dp)); return 2; }
            for (int32_t k = 0; k < dj.n_jobs; ++k) if (dpo.status[k] != 0) { fprintf(stderr, "[lamsa_aln] a stage-4 DP job overflowed its work buffer\n"); return 2; }
            n_rescue_jobs += dj.n_jobs;
        }
        const double t3 = now_s();
        const int turn = sams_turn; sams_turn ^= 1;
        if (file_write[turn].valid()) { const int e = file_write[turn].get(); if (e) return e; }          // the write that still reads this set
        std::vector<std::string> &sams = sams_set[turn];
        for (std::string &x : sams) x.clear();
        parallel_blocks(n, threads, [&](int t, int, int) {
            std::string &o = sams[(size_t)t];
            DpResults dp; dp.score = dpo.score; dp.qle = dpo.qle; dp.tle = dpo.tle; dp.cig_off = dpo.cig_off; dp.cigar = dpo.cigar; dp.base = base[(size_t)t];
            for (int r = t_first[(size_t)t]; r < t_last[(size_t)t]; ++r) {
                ReadResult &R = RR[(size_t)r];
                const int L = (int)B.reads[(size_t)r].seq.size();
                if (rescue && R.status == 0 && !plans[(size_t)r].lines.empty()) rescue_finish(R, codes + roff[r], L, ix, P, plans[(size_t)r], dp, fin_all);
                if (R.status != 0) {
                    ++bad_of[(size_t)t];
                    fprintf(stderr, "[lamsa_aln] read %s: %s; reported unmapped\n", B.reads[(size_t)r].name.c_str(), (R.status & LAMSA_HP_ST_UNSUPPORTED) ? "more than 32767 seeds, or a seed hit with |len_dif| > 127: beyond what the device keeps" : (R.status & LAMSA_HP_ST_REFEXIT) ? "input on which the reference aligner exits" : "device work buffer overflow");
                    for (int st = 0; st < 3; ++st) R.stage[st].clear();
                }
                rank_results(R, L, P);
                if (paf_any) write_paf(o, R, B.reads[(size_t)r], ix, opt);
                else write_sam(o, R, B.reads[(size_t)r], ix, opt);
            }
        });
        // The chunk's text (15 KB per 10-kbp read) goes out in input order.  Into a regular file every thread writes its own part at its own
        // offset (pwrite: one thread's write() of 250 MB per chunk was the slowest stage of the loop once the hits came from a binary stream;
        // a mapping of the file's new end, round 3's way, pays a page fault per 4 KB and was slower still: profiles/r04_cli_bench.txt); a pipe
        // or a terminal takes the parts one after the other.
        const double t4 = now_s();
        bool mapped_out = false;
        {
            size_t total = 0; for (const std::string &x : sams) total += x.size();
            struct stat st; const int fd = fileno(out);
            static const size_t map_min = getenv("LAMSA_MAP_OUT_MIN") ? (size_t)atol(getenv("LAMSA_MAP_OUT_MIN")) : ((size_t)8 << 20);      // (tests lower it)
            if (threads > 1 && total >= map_min && fd >= 0 && fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && !(fcntl(fd, F_GETFL) & O_APPEND)) {
                if (out_at < 0 && fflush(out) == 0) out_at = lseek(fd, 0, SEEK_CUR);
                if (out_at >= 0) {
                    const off_t base = out_at;
                    out_at += (off_t)total;
                    // (the stream's own position follows: whatever is written through `out` later -- a small chunk, nothing else today -- lands behind this one)
                    if (fflush(out) != 0 || lseek(fd, out_at, SEEK_SET) != out_at) { fprintf(stderr, "[lamsa_aln] cannot position the output file\n"); return 2; }
                    file_write[turn] = std::async(std::launch::async, [&sams, fd, base, threads]() -> int {
                        std::vector<size_t> at((size_t)threads + 1, 0);
                        for (int t = 0; t < threads; ++t) at[(size_t)t + 1] = at[(size_t)t] + sams[(size_t)t].size();
                        std::atomic<int> werr(0);
                        std::vector<std::thread> th;
                        for (int t = 0; t < threads; ++t) if (!sams[(size_t)t].empty()) th.emplace_back([&, t]() {
                            const char *p = sams[(size_t)t].data(); size_t left = sams[(size_t)t].size(); off_t o = base + (off_t)at[(size_t)t];
                            while (left) { const ssize_t k = pwrite(fd, p, left, o); if (k <= 0) { if (k < 0 && errno == EINTR) continue; werr = errno ? errno : EIO; return; } p += k; left -= (size_t)k; o += k; }
                        });
                        for (auto &x : th) x.join();
                        if (werr.load()) { fprintf(stderr, "[lamsa_aln] cannot write the output file: %s\n", strerror(werr.load())); return 2; }
                        return 0;
                    });
                    mapped_out = true;
                    ++n_mapped_chunks;
                }
            }
        }
        if (!mapped_out) for (int k = 0; k < 2; ++k) if (file_write[k].valid()) { const int e = file_write[k].get(); if (e) return e; }     // (text through `out` goes behind what is still being written)
        if (!mapped_out) out_at = -1;                           // (asked again after this chunk has gone through the stream)
        for (int t = 0; t < threads; ++t) { if (!mapped_out) fwrite(sams[(size_t)t].data(), 1, sams[(size_t)t].size(), out); n_bad += bad_of[(size_t)t]; }
        for (const Read &q : B.reads) n_bases += (long)q.seq.size();
        n_reads += (long)B.reads.size();
        sam_s += now_s() - t1;
        if (trace) fprintf(stderr, "[write] %d reads: records%s %.3f s, stage-4 DP batch (%ld jobs) %.3f s, finish + rank + SAM text %.3f s, write started in %.3f s (it runs beside the next chunk's text)\n", n, rescue ? " + stage-4 plan" : "", t2 - t1, (long)base[(size_t)threads], t3 - t2, t4 - t3, now_s() - t4);
        return 0;
    };
    std::future<int> writer;                                 // the write_chunk task of the chunk collected last
    std::vector<std::future<int>> dev_writer((size_t)G);     // per device: the write task that still reads the results of its last collect
    auto collect_and_write = [&](Chunk *ck) -> int {
        // the results of a collect stay valid until the next collect on the same handle: the chunk collected from this device
        // before must have been written
        if (dev_writer[(size_t)ck->dev].valid()) { const int e = dev_writer[(size_t)ck->dev].get(); if (e) return e; }
        ck->collected = std::promise<void>();
        std::future<void> done = ck->collected.get_future();
        enqueue(ck->dev, [&, ck]() {
            const double t0 = now_s();
            lamsa_hp_handle *hc = hs[(size_t)ck->dev];
            ck->col_rc = ck->sub_rc ? ck->sub_rc : lamsa_hp_collect_batch(hc, &ck->res);
            { std::lock_guard<std::mutex> lk(stat_m); wait_s += now_s() - t0; if (ck->col_rc == LAMSA_HP_OK) kernel_ms += lamsa_hp_last_kernel_ms(hc, 0) + lamsa_hp_last_kernel_ms(hc, 1); }
            if (ck->col_rc != LAMSA_HP_OK && !ck->sub_rc) fprintf(stderr, "[lamsa_aln] lamsa_hp_collect_batch failed: %d %s\n", ck->col_rc, lamsa_hp_last_error(hc));
            ck->collected.set_value();
        });
        done.wait();
        if (ck->col_rc != LAMSA_HP_OK) return 2;
        if (writer.valid()) { const int e = writer.get(); if (e) return e; }      // SAM text is written in input order, one chunk at a time
        std::shared_future<int> sf = std::async(std::launch::async, write_chunk, ck, ck->res).share();
        writer = std::async(std::launch::deferred, [sf]() { return sf.get(); });
        dev_writer[(size_t)ck->dev] = std::async(std::launch::deferred, [sf]() { return sf.get(); });
        return 0;
    };
    // Two chunks are in flight on the device (lamsa_hp_submit_batch): while the GPU aligns chunk i-1, chunk i is
    // uploaded behind it, chunk i+1 is read and parsed, and -- once collected -- chunk i-1's SAM text is written.
    if (opt.parse_only) {
        for (;;) {
            Chunk *c = prepare();
            if (c->ret || c->B.reads.empty()) { ret = c->ret; break; }
            n_reads += (long)c->B.reads.size(); for (const Read &q : c->B.reads) n_bases += (long)q.seq.size();
        }
        if (scanned.valid()) scanned.wait();
        saver.close();
        destroy_seed_handles();
        if (seed_fm) fprintf(stderr, "[lamsa_aln] --seed-fm: %ld chunks seeded in %.2f s (kernels %.1f ms)\n", n_seeded, seed_s, seed_kernel_ms);
        if (stats) { stats->n_reads = n_reads; stats->n_bases = n_bases; stats->wall_s = now_s() - t_begin; stats->load_s = load_s; stats->parse_s = parse_s; }
        return ret;
    }
    std::future<Chunk *> next = std::async(std::launch::async, prepare);
    std::deque<Chunk *> flying;                              // submitted, not yet collected: at most two per device
    for (;;) {
        Chunk *cur = next.get();
        if (cur->ret) ret = cur->ret;
        const bool have = ret == 0 && !cur->B.reads.empty();
        if (have) {
            next = std::async(std::launch::async, prepare);  // overlaps with everything below
            if (reserver.joinable()) reserver.join();
            cur->dev = (int)(n_submitted++ % G); cur->sub_rc = 0;
            enqueue(cur->dev, [&, cur]() { cur->sub_rc = submit(*cur); });       // on the device's own thread: the next chunk can go to the next device meanwhile
            flying.push_back(cur);
        }
        while (!flying.empty() && ((int)flying.size() >= 2 * G || !have || ret)) {
            const int e = collect_and_write(flying.front()); if (e && !ret) ret = e;
            flying.pop_front();
        }
        if (!have || ret) break;
    }
    if (writer.valid()) { const int e = writer.get(); if (e && !ret) ret = e; }
    for (auto &f : dev_writer) if (f.valid()) f.get();
    for (auto &f : file_write) if (f.valid()) { const int e = f.get(); if (e && !ret) ret = e; }
    stop_workers();
    if (next.valid()) next.wait();                       // the reader threads must be done before the files are closed
    if (scanned.valid()) scanned.wait();
    saver.close();
    if (reserver.joinable()) reserver.join();
    for (lamsa_hp_handle *hh : hs) lamsa_hp_destroy(hh);
    if (h_dp) lamsa_hp_destroy(h_dp);
    destroy_seed_handles();
    if (seed_fm) fprintf(stderr, "[lamsa_aln] --seed-fm: %ld chunks seeded in %.2f s (kernels %.1f ms)\n", n_seeded, seed_s, seed_kernel_ms);
    if (trace) fprintf(stderr, "[write] %ld chunks written by all threads side by side (pwrite)\n", n_mapped_chunks);
    if (stats) { stats->n_reads = n_reads; stats->n_bases = n_bases; stats->n_bad = n_bad; stats->kernel_ms = kernel_ms;
                 stats->wall_s = now_s() - t_begin; stats->load_s = load_s; stats->parse_s = parse_s; stats->submit_s = submit_s; stats->wait_s = wait_s; stats->sam_s = sam_s; stats->reserve_s = reserve_s; }
    return ret;
}

}  // namespace lamsa
