// hp_track.h -- branch tracking (branch_track_new / cut_branch / get_max_son, src/lamsa_dp_con.c:873,:831,:808) written once for two
// storages of the node state.  Included by hp_chain.h.
//
// Tracking is a pointer chase: every step of a walk, every son looked at by get_max_son, every detach depends on the load before it.
// Through HBM that is one memory round trip each.  No chaining edge joins two clusters (hp_cluster.h), so a track that starts at a
// hit of a cluster never leaves it: for the first round's tracking the read's LARGEST cluster is copied into this wave's LDS -- the
// IMAGE, six words per hit, next to the leaf bits of track_leaves -- and every track that starts at one of its hits runs on the
// image; the tracks of all other hits run through HBM as before.  The driver (track_leaves) and its order are the same for both, so
// the end nodes reach `ns` in the reference's order whatever the storage.  After tracking, what later code reads of the resident
// hits (predecessor, node count, pass flag) is written back once.
//
// The routines are templates over an accessor: TrHbm (a node is its hit index, the fields are the arrays of ReadCtx) or TrLds (a node
// is its PLACE in the cluster, rank - first rank, as in line_build; the fields are bit fields of the image).  Everything here is
// wave-uniform except where a comment says "per lane".
#pragma once

namespace hp {

#ifndef HP_TRACK_MIN
#define HP_TRACK_MIN 16           // smallest cluster worth an image (the value of HP_WALK_MIN, hp_gaps.h)
#endif
#define HP_TRACK_WORDS 6          // image words per hit
#define HP_TRACK_MAX_N 1020       // places (+ 1) and son counts are 10-bit fields

// member functions of the accessors (HP_INL of the tests' CPU build says `static`, which a member cannot be)
#ifdef __HIPCC__
#define HP_MEM __device__ __forceinline__
#else
#define HP_MEM inline
#endif

// the image of one cluster: on (a flag: LDS offset 0 is a valid address), first rank, hits, first LDS word
struct TrImg { int on, lo, n, base; };

struct TrHbm {
    static constexpr bool IMG = false;
    ReadCtx &r;
    HP_G int32_t *g_from, *g_son_n, *g_in_de, *g_ms, *g_mn, *g_mx;      // what a step of the walk touches; the rest goes through r
    HP_G NodeS *gd;
    HP_MEM TrHbm(ReadCtx &r_)
        : r(r_), g_from((HP_G int32_t *)r_.n_from), g_son_n((HP_G int32_t *)r_.n_son_n), g_in_de((HP_G int32_t *)r_.n_in_de), g_ms((HP_G int32_t *)r_.n_max_score),
          g_mn((HP_G int32_t *)r_.n_max_NM), g_mx((HP_G int32_t *)r_.n_max_node), gd((HP_G NodeS *)r_.nd) {}
    HP_MEM int hit(int n) const { return n; }
    HP_MEM int from(int n) const { return g_from[n]; }
    HP_MEM int son_n(int n) const { return g_son_n[n]; }
    HP_MEM int first(int n) const { return r.n_first[n]; }
    HP_MEM int next(int n) const { return r.n_next[n]; }
    HP_MEM int in_de(int n) const { return g_in_de[n]; }
    HP_MEM int score(int n) const { return gd[n].score; }
    HP_MEM int NM(int n) const { return gd[n].NM; }
    HP_MEM int match_flag(int n) const { return r.nd[n].match_flag; }
    HP_MEM int h_nm(int n) const { return r.h_nm[n]; }
    HP_MEM int slot(int n) const { return r.n_seed[n]; }
    HP_MEM int max_score(int n) const { return g_ms[n]; }
    HP_MEM int max_NM(int n) const { return g_mn[n]; }
    HP_MEM int max_node(int n) const { return g_mx[n]; }
    HP_MEM int node_n(int n) const { return r.n_node_n[n]; }
    HP_MEM void set_from(int n, int v) const { r.n_from[n] = v; }
    HP_MEM void set_in_de(int n, int v) const { g_in_de[n] = v; }
    HP_MEM void set_next(int n, int v) const { r.n_next[n] = v; }
    HP_MEM void set_sons(int n, int cnt, int only) const { r.n_son_n[n] = cnt; r.n_first[n] = only; r.n_last[n] = only; }     // no son, or the one kept
    HP_MEM void set_max_sn(int n, int s, int nm) const { g_ms[n] = s; g_mn[n] = nm; }
    HP_MEM void set_max(int n, int s, int nm, int node) const { g_ms[n] = s; g_mn[n] = nm; g_mx[n] = node; }
    HP_MEM void set_node_n(int n, int v) const { r.n_node_n[n] = v; }
    HP_MEM void mark(int n) const { gd[n].dp_flag = TRACKED_FLAG; }        // per lane too
    HP_MEM void marks_done() const {}
};

// The image: six arrays of n words, array k at word k * n.
//   0  score << 16 | NM                      (16 bits each: the checks of dp_cluster_lds)
//   1  max_score << 16 | max_NM
//   2  from + 1 | (first + 1) << 10 | (next + 1) << 20           places; 0: none
//   3  son_n | (in_de + 1) << 10 | max_node << 21
//   4  node_n | h_nm << 11
//   5  seed slot | match_flag << 14 | (dp_flag & 15) << 19
struct TrLds {
    static constexpr bool IMG = true;
    HP_L int32_t *w; int n, lo; const HP_G int32_t *g_srt;
    HP_MEM TrLds(const ReadCtx &r, const TrImg &m) : w(r.cx.lds + m.base), n(m.n), lo(m.lo), g_srt((const HP_G int32_t *)r.srt) {}
    HP_MEM int rd(int k, int i) const { return wv::uni(w[k * n + i]); }
    HP_MEM void fld(int k, int i, int shift, int mask, int v) const { HP_L int32_t *p = w + k * n + i; *p = (*p & ~(mask << shift)) | ((v & mask) << shift); }
    HP_MEM int hit(int i) const { return g_srt[lo + i]; }
    HP_MEM int from(int i) const { return (rd(2, i) & 1023) - 1; }
    HP_MEM int first(int i) const { return ((rd(2, i) >> 10) & 1023) - 1; }
    HP_MEM int next(int i) const { return ((rd(2, i) >> 20) & 1023) - 1; }
    HP_MEM int son_n(int i) const { return rd(3, i) & 1023; }
    HP_MEM int in_de(int i) const { return ((rd(3, i) >> 10) & 2047) - 1; }
    HP_MEM int max_node(int i) const { return (rd(3, i) >> 21) & 1023; }
    HP_MEM int score(int i) const { return rd(0, i) >> 16; }
    HP_MEM int NM(int i) const { return rd(0, i) & 0xffff; }
    HP_MEM int max_score(int i) const { return rd(1, i) >> 16; }
    HP_MEM int max_NM(int i) const { return rd(1, i) & 0xffff; }
    HP_MEM int node_n(int i) const { return rd(4, i) & 2047; }
    HP_MEM int h_nm(int i) const { return (rd(4, i) >> 11) & 0xffff; }
    HP_MEM int slot(int i) const { return rd(5, i) & 16383; }
    HP_MEM int match_flag(int i) const { return (rd(5, i) >> 14) & 31; }
    HP_MEM void set_from(int i, int v) const { fld(2, i, 0, 1023, v + 1); }
    HP_MEM void set_next(int i, int v) const { fld(2, i, 20, 1023, v + 1); }
    HP_MEM void set_in_de(int i, int v) const { fld(3, i, 10, 2047, v + 1); }
    HP_MEM void set_sons(int i, int cnt, int only) const { fld(3, i, 0, 1023, cnt); fld(2, i, 10, 1023, only + 1); }
    HP_MEM void set_max_sn(int i, int s, int nm) const { w[n + i] = (int)(((unsigned)s << 16) | ((unsigned)nm & 0xffffu)); }
    HP_MEM void set_max(int i, int s, int nm, int node) const { set_max_sn(i, s, nm); fld(3, i, 21, 1023, node); }
    HP_MEM void set_node_n(int i, int v) const { fld(4, i, 0, 2047, v); }
    HP_MEM void mark(int i) const { HP_L int32_t *p = w + 5 * n + i; *p = (*p & ~(15 << 19)) | (TRACKED_FLAG << 19); }      // per lane too (no wv::uni)
    HP_MEM void marks_done() const { wv::sync(); }         // marks made one per lane are read wave-uniformly afterwards
    // per lane: is place i a leaf of the pass (the test of track_slot)
    HP_MEM int leaf(int i, int dp_flag, bool skip_lone) const {
        const int lk = w[2 * n + i], ct = w[3 * n + i], id = w[5 * n + i];
        int v = ((int)((unsigned)id << 9) >> 28) == dp_flag && ((ct >> 10) & 2047) == 1;
        if (v && skip_lone && (lk & 1023) == 0 && (ct & 1023) == 0) v = 0;
        return v;
    }
};

// path (may be null): the ancestors of `node` in lane order, n_path <= 64 of them, when the caller has just walked them -- they are
// then marked with one store instead of being chased through `from` again
template <class A>
HP_HOT void ns_add_end(const A &a, ReadCtx &r, NScore &ns, int score, int NM, int node, const wv::Lane<int> *path = nullptr, int n_path = 0)
{   // node_add_score, lamsa_dp_con.c:786
    if (score < ns.min_score_thd) return;
    if (ns.node_n >= ns.cap) { r.cx.status |= ST_OVERFLOW; return; }
    ns.score[ns.node_n] = score; ns.NM[ns.node_n] = NM; ns.node[ns.node_n++] = a.hit(node);
    a.mark(node);
    if (path) { WAVE_FOR(l) { if (l < n_path) a.mark((*path)[l]); } a.marks_done(); return; }
    for (int t = a.from(node); t >= 0; t = a.from(t)) a.mark(t);
}

// ---------------------------------------------------------------- forest -> disjoint paths
template <class A>
HP_HOT int best_son(const A &a, int f)
{   // get_max_son, :808
    int max_score = 0, max_NM = 0, max_dis = 0, flag_thd = F_INIT, max = -1;
    const int x = a.slot(f);
    for (int s = a.first(f), c = 0, nn = a.son_n(f); c < nn && s >= 0; s = a.next(s), ++c) {
        const int mf = a.match_flag(s), sx = a.slot(s), ms = a.max_score(s), mn = a.max_NM(s);
        if (A::IMG && max >= 0) {                     // which tie rule a test's read has met (counters of the tests' CPU build only)
            if (mf > flag_thd) HP_STAT_ADD(60, 1);
            else if (ms == max_score && sx - x != max_dis) HP_STAT_ADD(58, 1);
            else if (ms == max_score) HP_STAT_ADD(59, 1);
        }
        if (mf <= flag_thd && (ms > max_score || (ms == max_score && (sx - x < max_dis || mn < max_NM)))) {
            max = s; max_score = ms; max_NM = mn; max_dis = sx - x;
            if (mf <= F_MATCH_THD) flag_thd = F_MATCH_THD;
        }
    }
    return max;
}
template <class A>
HP_HOT void detach(const A &a, ReadCtx &r, int s, int max_node, NScore &ns)
{   // :842-847 / :851-857 / :893-899
    a.set_from(s, -1);
    const int ms = a.max_score(s) - (a.score(s) - 1), mn = a.max_NM(s) - (a.NM(s) - a.h_nm(s));
    a.set_max_sn(s, ms, mn);
    a.set_node_n(max_node, a.node_n(max_node) - (a.node_n(s) - 1));
    ns_add_end(a, r, ns, ms, mn, max_node);
}
template <class A>
HP_HOT void leaf_mark(const A &a, ReadCtx &r, int f)
{   // see track_leaves: the driver only visits seeds whose bit is set
    if (r.leaf_on) { const int x = a.slot(f); r.leaf_bits[x >> 5] |= (int)(1u << (x & 31)); }
}
template <class A>
HP_HOT void cut_branch(const A &a, ReadCtx &r, int f, NScore &ns)
{   // :831-870
    const int keep = best_son(a, f);
    if (keep < 0) { r.cx.status |= ST_REFEXIT; a.set_in_de(f, 0); leaf_mark(a, r, f); return; }
    const int nn = a.son_n(f);
    if (A::IMG && nn >= 2) HP_STAT_ADD(53, 1);
    if (A::IMG && nn >= 3) HP_STAT_ADD(62, 1);
    for (int s = a.first(f), c = 0; c < nn && s >= 0; ++c) {
        const int nxt = a.next(s);
        if (s != keep) detach(a, r, s, a.max_node(s), ns);
        s = nxt;
    }
    if (a.score(f) > a.max_score(keep)) {             // negative edge
        if (A::IMG) HP_STAT_ADD(55, 1);
        a.set_in_de(keep, -1);
        detach(a, r, keep, a.max_node(keep), ns);
        a.set_sons(f, 0, -1);
        a.set_max(f, a.score(f), a.NM(f), f);
    } else {
        a.set_sons(f, 1, keep); a.set_next(keep, -1);
        a.set_max(f, a.max_score(keep), a.max_NM(keep), a.max_node(keep));
    }
    a.set_in_de(f, 0);
    leaf_mark(a, r, f);                               // f is complete: a track starts from it when its seed is reached
}
template <class A>
HP_HOT void branch_track(const A &a, ReadCtx &r, int n, NScore &ns)
{   // branch_track_new, :873-920
    // The walk up a chain is a pointer chase: what a step needs (son count, score, predecessor) is requested together, one round trip
    // per step (HBM) or one LDS access time (image), and the nodes walked are kept in a lane register so that node_add_score need not
    // chase them again.
    int max_score, max_NM, max_node;
    a.set_in_de(n, -1);
    const int n_sons = a.son_n(n), n_score = a.score(n), n_NM = a.NM(n);
    int fa = a.from(n);
    if (n_sons == 0) { max_node = n; max_score = n_score; max_NM = n_NM; }      // (stored below, when and where they are read again)
    else { max_node = a.max_node(n); max_score = a.max_score(n); max_NM = a.max_NM(n); }
    wv::Lane<int> path;                               // the ancestors of max_node walked so far, while path_ok
    WAVE_FOR(l) { path[l] = 0; }
    int n_path = 0; bool path_ok = n_sons == 0;       // a leaf: max_node is n itself, its ancestors are exactly the nodes walked below
    // What the reference stores in every node it walks over (max_score, max_NM, max_node, in_de = -1; :885-910) is read again only for
    // the node right below a node with several sons (get_max_son / cut_branch look at their sons) or below a negative edge: the walk
    // keeps the three values in registers and stores them for that node alone -- four stores less per step.  in_de is only ever
    // compared with 0 (is the node a leaf?), and a walked node with one son keeps its 1.
    int prev = n;                                     // the node below fa
    while (fa >= 0) {
        const int fa_sons = a.son_n(fa), fa_score = a.score(fa), fa_from = a.from(fa);
#ifdef HP_PROF_TRACK
        if (HP_PROF_CHAIN_ON && r.prof) r.prof[20] += 1;
#endif
        if (A::IMG) HP_STAT_ADD(52, 1);
        if (fa_sons == 1) {
            if (fa_score > max_score) {               // negative edge
                if (A::IMG) HP_STAT_ADD(54, 1);
                const int s = a.first(fa);
                a.set_max(prev, max_score, max_NM, max_node);          // s == prev: detach reads them
                wv::sync();
                a.set_in_de(s, -1);
                detach(a, r, s, max_node, ns);
                a.set_sons(fa, 0, -1);
                max_score = a.score(fa); max_NM = a.NM(fa); max_node = fa;
                n_path = 0; path_ok = true;           // from here on the ancestors of max_node = fa are what is walked next
            } else if (path_ok) {
                if (n_path < 64) { WAVE_FOR(l) { if (l == n_path) path[l] = fa; } ++n_path; } else path_ok = false;
            }
            prev = fa;
            fa = fa_from;                             // detach() above changes `from` of the son only, never of fa
        } else {
            a.set_max(prev, max_score, max_NM, max_node);              // prev is a son of fa: what get_max_son / cut_branch read
            const int left_ = a.in_de(fa) - 1;
            a.set_in_de(fa, left_);
#ifdef HP_PROF_TRACK
            if (HP_PROF_CHAIN_ON && r.prof) r.prof[21] += 1;
            const long long tcb_ = wv::clock();
#endif
            if (left_ == 0) { wv::sync(); cut_branch(a, r, fa, ns); }
#ifdef HP_PROF_TRACK
            if (HP_PROF_CHAIN_ON && r.prof) r.prof[22] += wv::clock() - tcb_;
#endif
            return;
        }
    }
    if (A::IMG && !path_ok) HP_STAT_ADD(56, 1);
    ns_add_end(a, r, ns, max_score, max_NM, max_node, path_ok ? &path : nullptr, n_path);
}

// ---------------------------------------------------------------- the image of the read's largest cluster
// cs: first rank of each of the n_cl clusters (cs[n_cl] = H); last_slot: the last seed slot of the tracking that follows, whose leaf
// bits take the first words of the LDS.  The cluster becomes resident when it has at least HP_TRACK_MIN hits, its image fits behind
// the bits, and every field fits its width; otherwise the image is off and tracking runs through HBM alone.
// Built from what the main pass and build_sons have just written.  max_score / max_NM / max_node are written by tracking before it
// reads them (the walk stores them for a node before cut_branch or detach looks at it); they start as the node's own.
HP_NOINL TrImg track_image_build(ReadCtx &r, const int32_t *cs, int n_cl, int last_slot)
{
    TrImg m; m.on = 0; m.lo = 0; m.n = 0; m.base = 0;
    const HP_G int32_t *g_cs = (const HP_G int32_t *)cs;
    int n = 0, lo = 0;
    for (int c0 = 0; c0 < n_cl; c0 += 64) {           // the largest cluster; ties: the lowest rank
        wv::Lane<int> sz, e;
        WAVE_FOR(l) { const int c = c0 + l; sz[l] = c < n_cl ? g_cs[c + 1] - g_cs[c] : 0; }
        const int mx = wv::reduce_max(sz);
        if (mx > n) { WAVE_FOR(l) e[l] = sz[l] == mx; n = mx; lo = g_cs[c0 + __builtin_ctzll(wv::ballot(e))]; }
    }
    const int nw = (last_slot >> 5) + 1;
    if (last_slot < 0 || n < HP_TRACK_MIN || n > HP_TRACK_MAX_N || nw > r.cx.lds_words || HP_TRACK_WORDS * n > r.cx.lds_words - nw) return m;
    const HP_G NodeS *ns_ = (const HP_G NodeS *)r.nd;
    const HP_G int32_t *g_srt = (const HP_G int32_t *)r.srt, *g_rnk = (const HP_G int32_t *)r.rnk, *g_seed = (const HP_G int32_t *)r.n_seed;
    const HP_G int32_t *g_from = (const HP_G int32_t *)r.n_from, *g_son_n = (const HP_G int32_t *)r.n_son_n, *g_first = (const HP_G int32_t *)r.n_first;
    const HP_G int32_t *g_next = (const HP_G int32_t *)r.n_next, *g_in_de = (const HP_G int32_t *)r.n_in_de, *g_node_n = (const HP_G int32_t *)r.n_node_n;
    const HP_G int16_t *g_hnm = (const HP_G int16_t *)r.h_nm;
    HP_L int32_t *w = r.cx.lds + nw;
    int nm_sum = 0, bad = 0;
    wv::sync();                                        // whatever used this LDS before is done
    for (int i0 = 0; i0 < n; i0 += 64) {
        wv::Lane<int> nml, badl;
        WAVE_FOR(l) {
            const int i = i0 + l;
            int nmv = 0, bv = 0;
            if (i < n) {
                const int id = g_srt[lo + i];
                int q[4]; hp_load16((const HP_G char *)(ns_ + id) + 16, q);
                const int dpf = (int)(int8_t)(q[1] & 0xff), mf = (q[1] >> 16) & 0xff, score = q[2], NM = q[3];
                const int fr = g_from[id], sn = g_son_n[id], fi = g_first[id], nx_ = g_next[id], ide = g_in_de[id], nn = g_node_n[id], slot = g_seed[id];
                nmv = g_hnm[id];
                const int pf = fr >= 0 ? g_rnk[fr] - lo : -1;                         // places inside the cluster
                const int p1 = sn > 0 && fi >= 0 ? g_rnk[fi] - lo : -1;
                const int pn = fr >= 0 && nx_ >= 0 ? g_rnk[nx_] - lo : -1;            // `next` is set for every hit that has a predecessor (build_sons)
                bv = score < -30000 || score > 30000 || NM < 0 || NM > 65535 || nmv < 0 || sn < 0 || sn > n || (sn > 0 && fi < 0) || ide < 0 || ide > n ||
                     nn < 1 || nn > n || slot < 0 || slot > 16383 || mf > 31 || dpf < -8 || dpf > 7 ||
                     pf >= n || p1 >= n || pn >= n || (fr >= 0 && pf < 0) || (p1 < -1) || (pn < -1);
                w[i] = (int)(((unsigned)score << 16) | ((unsigned)NM & 0xffffu));
                w[n + i] = w[i];
                w[2 * n + i] = ((pf + 1) & 1023) | (((p1 + 1) & 1023) << 10) | (((pn + 1) & 1023) << 20);
                w[3 * n + i] = (sn & 1023) | (((ide + 1) & 2047) << 10) | (i << 21);
                w[4 * n + i] = (nn & 2047) | ((nmv & 0xffff) << 11);
                w[5 * n + i] = (slot & 16383) | ((mf & 31) << 14) | ((dpf & 15) << 19);
            }
            nml[l] = nmv; badl[l] = bv;
        }
        nm_sum += wv::reduce_sum(nml);
        if (wv::ballot(badl) != 0) bad = 1;
    }
    wv::sync();
    if (bad || nm_sum > 65535) { HP_STAT_ADD(61, 1); return m; }              // a chain's NM is at most the sum over the cluster: 16 bits suffice
    HP_STAT_ADD(49, 1); HP_STAT_MAX(57, n);
    m.on = 1; m.lo = lo; m.n = n; m.base = nw;
    return m;
}

// What tracking changes and later code reads: the predecessor (detach), the node count of an end node, the pass flag (TRACKED).
// Score, NM and match_flag are not changed by tracking; in_de, the son lists and max_* are read by tracking alone (the next pass that
// tracks -- frag_mini_dp_multi_line -- resets every hit it uses by fnode_set and builds its own lists: nodes_per_init, dp_update_range
// with `sons`).
HP_NOINL void track_image_store(ReadCtx &r, TrImg m)
{
    const HP_G int32_t *g_srt = (const HP_G int32_t *)r.srt;
    HP_G int32_t *g_from = (HP_G int32_t *)r.n_from, *g_node_n = (HP_G int32_t *)r.n_node_n;
    HP_G NodeS *gd = (HP_G NodeS *)r.nd;
    const HP_L int32_t *w = r.cx.lds + m.base;
    const int n = m.n, lo = m.lo;
    wv::sync();
    for (int i0 = 0; i0 < n; i0 += 64) {
        WAVE_FOR(l) {
            const int i = i0 + l;
            if (i < n) {
                const int id = g_srt[lo + i];
                const int fp = w[2 * n + i] & 1023;
                g_from[id] = fp ? g_srt[lo + fp - 1] : -1;
                g_node_n[id] = w[4 * n + i] & 2047;
                gd[id].dp_flag = (int8_t)((int)((unsigned)w[5 * n + i] << 9) >> 28);
            }
        }
    }
    wv::sync();
}

}  // namespace hp
