// emu_edge.cpp -- TEST INFRASTRUCTURE (tests/test_edge_cpu.py): the edge classifier in diagonal form (hit_diag / edge_dis / edge_class_diag /
// edge_match_diag of lamsa_amd/csrc/hp_chain.h) and gap_edge (hp_cluster.h) against edge_flag_packed, the general 64-bit definition, on
// explicit pairs of hits under the CPU lane emulation.  The set-up is emu_api.cpp's, which is included as it is.
// the pair count of dp_cluster_lds' target loop two ways (hooks of hp_cluster.h): block by block as the loop scans them, and the closed form that
// goes into r.n_pairs; and the blocks that the block minimum kept out of a target's scan
long long g_edge_pairs_blocks = 0, g_edge_pairs_formula = 0, g_edge_blocks_skipped = 0, g_edge_targets = 0;
#define HP_PAIRS_BLOCK(hits) (g_edge_pairs_blocks += (hits))
#define HP_PAIRS_TARGET(pairs, blocks_skipped) (g_edge_pairs_formula += (pairs), g_edge_blocks_skipped += (blocks_skipped), ++g_edge_targets)
#include "emu_api.cpp"

extern "C" void emu_edge_pairs_reset() { g_edge_pairs_blocks = g_edge_pairs_formula = g_edge_blocks_skipped = g_edge_targets = 0; }
extern "C" void emu_edge_pairs(long long *out) { out[0] = g_edge_pairs_blocks; out[1] = g_edge_pairs_formula; out[2] = g_edge_blocks_skipped; out[3] = g_edge_targets; }

// n pairs of hits of one contig and strand sp[i]: `a` the hit of the earlier seed, `b` the other (positions 1-based, 64-bit).  Out, per pair:
//   want[i]     edge_flag_packed(a, b)            want_rev[i]  edge_flag_packed(b, a)   (the definition is symmetric in its arguments)
//   diag[i]     edge_class_diag on the two diagonals, positions relative to `base[i]`, seed ids relative to sid0
//   match[i]    edge_match_diag on the same
//   gap[i]      gap_edge on the relative positions
// Returns edge_k24 of the handle's constants.
extern "C" int emu_edge_grid(const lamsa_hp_para *P, int n, int sid0, const int32_t *sp, const int64_t *base,
                             const int64_t *apos, const int32_t *asid, const int32_t *ald, const int64_t *bpos, const int32_t *bsid, const int32_t *bld,
                             int32_t *want, int32_t *want_rev, int32_t *diag, int32_t *match, int32_t *gap)
{
    const EdgeK K = edge_consts(P);
    for (int i = 0; i < n; ++i) {
        NodeS A, B;
        memset(&A, 0, sizeof A); memset(&B, 0, sizeof B);
        A.pos = apos[i]; A.chr = 1; A.slot_j = asid[i] << 14; A.sid = (int16_t)asid[i]; A.strand = (int8_t)sp[i]; A.len_dif8 = (int8_t)ald[i];
        B.pos = bpos[i]; B.chr = 1; B.slot_j = bsid[i] << 14; B.sid = (int16_t)bsid[i]; B.strand = (int8_t)sp[i]; B.len_dif8 = (int8_t)bld[i];
        want[i] = edge_flag_packed(K, A, B);
        want_rev[i] = edge_flag_packed(K, B, A);
        const int ra = (int)(apos[i] - base[i]), rb = (int)(bpos[i] - base[i]);
        const int da = hit_diag(K, sp[i], ra, asid[i] - sid0), db = hit_diag(K, sp[i], rb, bsid[i] - sid0);
        const int dsid = bsid[i] - asid[i];
        const int dis = edge_dis(da, db, sp[i] > 0 ? ald[i] : bld[i]);
        diag[i] = edge_class_diag(K, dis, dsid);
        match[i] = edge_match_diag(K, dis, dsid) ? 1 : 0;
        gap[i] = gap_edge(K, sp[i], ra, asid[i], ald[i], rb, bsid[i], bld[i]);
    }
    return edge_k24(K) ? 1 : 0;
}
