// hp_api.hip -- C-ABI of liblamsa_hp.so (include/lamsa_hp.h) and the gfx950 kernels behind it.
// HIP only: there is no CPU path in this library; every entry point fails with
// LAMSA_HP_ENODEV when no HIP device is usable.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>
#include <algorithm>
#include <string>
#include "hp_dp_batch.h"
#include "hp_wavejob.h"

using namespace hp;

// ------------------------------------------------------------------ kernels
// One wavefront (64 threads) per workgroup; a persistent grid pulls units from a queue head.
__global__ __launch_bounds__(64) void k_dp_batch(DpBatchArgs a)
{
    __shared__ int32_t lds[HP_LDS_WORDS];
    const int slot = blockIdx.x;
    for (;;) {
        int job = 0;
        if (wv::leader()) job = atomicAdd(a.counter, 1);
        job = wv::uni(job);
        if (job >= a.n_jobs) break;
        dp_run_job(a, job, slot, (HP_L int32_t *)lds);
    }
}

// The same jobs by the routines the read path's lane-per-job launch uses: kinds 4 / 5 / 6 = ksw_global2 / ksw_extend_core / ksw_bi_extend one
// job per LANE (hp_lanedp.h, what k_filldp_small runs).  Targets come 2 bits per base (tk: first base of every job in `pac`), as those
// routines read the reference.
__global__ __launch_bounds__(64, 1) void k_dp_batch_lane(DpBatchArgs a, const uint8_t *pac, const int64_t *tk)
{
    __shared__ int32_t lds[HP_LJ_LDS_WORDS(HP_LJ_QCAP)];
    const lamsa_hp_para *P = &a.P;
    char *slab = a.slab + (size_t)blockIdx.x * a.slab_per_wave;
    cig_t *cbuf = (cig_t *)slab;
    uint8_t *zbuf = (uint8_t *)(slab + sizeof(cig_t) * 3 * HP_LJ_CIG * 64);
    for (;;) {
        int g = 0;
        if (wv::leader()) g = atomicAdd(a.counter, 1);
        g = wv::uni(g);
        if (g * 64 >= a.n_jobs) break;
        wv::sync();
        WAVE_FOR(l) {
            const int job = g * 64 + l;
            if (job < a.n_jobs) {
                LaneJob J;
                J.q = (const HP_G uint8_t *)(a.seq + a.q_off[job]); J.qs = 1; J.qcomp = 0; J.qlen = a.qlen[job]; J.pac = (const HP_G uint8_t *)pac; J.tk = tk[job]; J.ts = 1; J.tlen = a.tlen[job];
                J.z = (HP_G uint8_t *)zbuf; J.zl = l; J.zs = HP_LJ_QCAP; J.cells = 0; J.row = (HP_L int32_t *)lds + l; J.qrow = (HP_L uint8_t *)((HP_L int32_t *)lds + (HP_LJ_QCAP + 2) * 64) + l; J.rev = 0;
                lj_stage_query(J);
                LCig out, Lc, Rc;
                out.c = cbuf + (size_t)l * 3 * HP_LJ_CIG; out.n = 0; Lc.c = out.c + HP_LJ_CIG; Lc.n = 0; Rc.c = Lc.c + HP_LJ_CIG; Rc.n = 0;
                int sc = 0, qle = 0, tle = 0;
                const int kind = a.kind[job];
                if (kind == 4) sc = lj_global(P, J, P->del_gapo, P->del_gape, P->ins_gapo, P->ins_gape, a.w[job], &out);
                else if (kind == 5) sc = lj_extend(P, J, a.w[job], a.h0[job], &qle, &tle, &out);
                else sc = lj_bi_extend(P, J, a.h0[job], a.h0[job], Lc, Rc, out);
                a.score[job] = sc; a.qle[job] = qle; a.tle[job] = tle; a.status[job] = 0; a.cig_n[job] = out.n;
                cig_t *dst = a.cig + a.cig_cap_off[job];
                for (int k = 0; k < out.n; ++k) dst[k] = out.c[k];
            }
        }
        wv::sync();
    }
}
// Kinds 8 .. 11: a job as the wave-per-job launch of the read path runs it (hp_wavejob.h: k_filldp_wave's registers and LDS, sequences staged
// from the read bytes and the packed reference, the direction matrix in LDS where it fits): 8 = a junction's ksw_bi_extend(h0, h0), 9 = a
// seed gap's ksw_global2(w), 10 / 11 = a line's head / tail extension (ksw_extend_r / ksw_extend_c with (w, h0), the rest of the query
// clipped, the head's CIGAR turned round -- frag_check.c:640-648, :699-703).
__global__ __launch_bounds__(64, HP_WJ_WAVES_PER_SIMD) void k_dp_batch_wave(DpBatchArgs a, const uint8_t *pac, const int64_t *tk)
{
    __shared__ int32_t lds[HP_WJ_LDS_WORDS];
    for (;;) {
        int job = 0;
        if (wv::leader()) job = atomicAdd(a.counter, 1);
        job = wv::uni(job);
        if (job >= a.n_jobs) break;
        Ctx cx;
        cx.P = &a.P; cx.lds = (HP_L int32_t *)lds; cx.lds_words = HP_WJ_LDS_WORDS; cx.status = 0; cx.n_cells = 0; cx.lds_epoch = 0; cx.prof = nullptr;
        arena_init(cx.tmp, a.slab + (size_t)blockIdx.x * a.slab_per_wave, a.slab_per_wave);
        const int type = wv::uni(a.kind[job]) - 7, qlen = wv::uni(a.qlen[job]), tlen = wv::uni(a.tlen[job]);
        const bool back = type == WJ_HEAD;
        CigV out; cig_bind(out, a.cig + a.cig_cap_off[job], (int)(a.cig_cap_off[job + 1] - a.cig_cap_off[job]));
        WjOut o;
        wj_run(cx, a.seq, pac, type, 0, a.q_off[job] + (back && qlen > 0 ? qlen - 1 : 0), back ? -1 : 1, qlen, tk[job] + (back && tlen > 0 ? tlen - 1 : 0), back ? -1 : 1, tlen,
               wv::uni(a.w[job]), wv::uni(a.h0[job]), out, o);
        if (wv::leader()) { a.score[job] = o.score; a.qle[job] = o.qle; a.tle[job] = o.tle; a.status[job] = cx.status; a.cig_n[job] = out.n; }
        wv::sync();
    }
}

#include "hp_handle.h"

#include "hp_para.h"

extern "C" int lamsa_hp_create(lamsa_hp_handle **out, const lamsa_hp_para *para, const lamsa_hp_ref *ref, int device_id)
{
    if (!out || !para) return LAMSA_HP_EINVAL;
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device_id < 0 || device_id >= n_dev) return LAMSA_HP_ENODEV;
    if (hipSetDevice(device_id) != hipSuccess) return LAMSA_HP_ENODEV;
    lamsa_hp_handle *h = new lamsa_hp_handle();
    h->device = device_id; h->para = *para;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) h->n_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&h->stream_b, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) { delete h; return LAMSA_HP_ENODEV; }
    if (ref && ref->pac) {
        size_t pb = (size_t)(ref->l_pac / 4 + 1);
        h->l_pac = ref->l_pac; h->n_seqs = ref->n_seqs;
        if (hipMalloc((void **)&h->d_pac, pb + 16) != hipSuccess ||
            hipMalloc((void **)&h->d_seq_off, sizeof(int64_t) * (size_t)(ref->n_seqs + 1)) != hipSuccess ||
            hipMalloc((void **)&h->d_seq_len, sizeof(int32_t) * (size_t)(ref->n_seqs + 1)) != hipSuccess) { lamsa_hp_destroy(h); return LAMSA_HP_ENOMEM; }
        hipMemcpy(h->d_pac, ref->pac, pb, hipMemcpyHostToDevice);
        hipMemcpy(h->d_seq_off, ref->seq_offset, sizeof(int64_t) * (size_t)ref->n_seqs, hipMemcpyHostToDevice);
        hipMemcpy(h->d_seq_len, ref->seq_len, sizeof(int32_t) * (size_t)ref->n_seqs, hipMemcpyHostToDevice);
    }
    *out = h;
    return LAMSA_HP_OK;
}

extern "C" void lamsa_hp_release_state_(lamsa_hp_handle *h);
extern "C" void lamsa_hp_destroy(lamsa_hp_handle *h)
{
    if (!h) return;
    hipSetDevice(h->device);
    lamsa_hp_release_state_(h);
    if (h->d_pac) hipFree(h->d_pac);
    if (h->d_seq_off) hipFree(h->d_seq_off);
    if (h->d_seq_len) hipFree(h->d_seq_len);
    h->in.release(); h->out.release(); h->slab.release(); h->misc.release(); h->pac2.release();
    if (h->fm_bwt) hipFree(h->fm_bwt);
    if (h->fm_sa) hipFree(h->fm_sa);
    h->fm_in.release(); h->fm_out.release(); h->fm_pos.release();
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->stream) hipStreamDestroy(h->stream);
    if (h->copy_stream) hipStreamDestroy(h->copy_stream);
    if (h->stream_b) hipStreamDestroy(h->stream_b);
    delete h;
}

extern "C" const char *lamsa_hp_last_error(const lamsa_hp_handle *h) { return h ? h->err.c_str() : "null handle"; }
extern "C" float lamsa_hp_last_kernel_ms(const lamsa_hp_handle *h, int which) { return (h && which >= 0 && which < 24) ? h->kernel_ms[which] : -1.f; }


extern "C" int lamsa_hp_dp_batch_staged_(lamsa_hp_handle *h, const lamsa_hp_dp_jobs *J, lamsa_hp_dp_out *O);      // kinds 12 / 13 (hp_align_api.hip)
extern "C" int lamsa_hp_dp_batch(lamsa_hp_handle *h, const lamsa_hp_dp_jobs *J, lamsa_hp_dp_out *O)
{
    if (!h || !J || !O || J->n_jobs < 0) return LAMSA_HP_EINVAL;
    HIPCHK(h, hipSetDevice(h->device), LAMSA_HP_ENODEV);
    const int n = J->n_jobs;
    if (n > 0 && J->kind[0] >= 12) return lamsa_hp_dp_batch_staged_(h, J, O);
    // capacities: a DP CIGAR has at most qlen+tlen words (+ slack for the S/H pair of sw_mid_fix)
    std::vector<int64_t> cap_off((size_t)n + 1, 0);
    size_t z_need = 4096;
    for (int i = 0; i < n; ++i) {
        int ql = J->qlen[i], tl = J->tlen[i];
        if (ql < 0) ql = 0;
        if (tl < 0) tl = 0;
        if (J->q_off[i] < 0 || J->t_off[i] < 0 || J->q_off[i] + ql > J->seq_bytes || J->t_off[i] + tl > J->seq_bytes) { h->err = "dp job sequence out of range"; return LAMSA_HP_EINVAL; }
        cap_off[i + 1] = cap_off[i] + ql + tl + (J->kind[i] >= 8 ? 72 : 8);
        // worst-case scratch of one job: H,E rows + row bounds + direction matrix + 3 temporary CIGARs (bi-extend)
        size_t wmax = (size_t)(abs(ql - tl) + 3 > (J->kind[i] == 2 ? h->para.band_w : J->w[i]) ? abs(ql - tl) + 3 : (J->kind[i] == 2 ? h->para.band_w : J->w[i]));
        size_t ncol = (size_t)ql < 2 * wmax + 1 ? (size_t)ql : 2 * wmax + 1;
        if (ql <= HP_PK_QMAX(2) && ncol < 128) ncol = 128;          // the two-columns-per-lane extension keeps whole rows of its direction matrix (hp_ksw.h)
        size_t need = 2 * 4 * ((size_t)ql + 18) + 8 * ((size_t)tl + 17) + ncol * tl + 64 + 3 * 4 * ((size_t)ql + tl + 24) + 1024;
        if (need > z_need) z_need = need;
    }
    // kinds 4..6: the lane-per-job routines (they take jobs up to their buffers' sizes and, like the read path, only when the handle's penalties
    // keep their 16-bit cells exact -- else the jobs run on the wave routines, kind - 4); kinds 8..11: a job as the wave-per-job launch runs it.
    // One class per call.
    int cls = 0;                                          // 0: wave routines (k_dp_batch), 1: a job per lane, 2: the wave-per-job launch's way
    std::vector<int32_t> kind_v;
    std::vector<uint8_t> pac; std::vector<int64_t> tkv;
    if (n > 0 && J->kind[0] >= 4) {
        cls = J->kind[0] >= 8 ? 2 : 1;
        for (int i = 0; i < n; ++i) {
            const int k = J->kind[i];
            if (k < 4 || k == 7 || k > 11 || (k >= 8) != (cls == 2)) { h->err = "dp batch mixes job classes"; return LAMSA_HP_EINVAL; }
            if (cls == 1 && (J->qlen[i] < 0 || J->qlen[i] > HP_LJ_QCAP || J->tlen[i] < 0 || J->tlen[i] > HP_LJ_TCAP || (k != 4 && J->h0[i] <= 0))) { h->err = "dp job beyond the lane routines' buffers"; return LAMSA_HP_EINVAL; }
            if (cls == 2 && (J->qlen[i] < 0 || J->tlen[i] < 0 || (k != 9 && J->h0[i] <= 0))) { h->err = "dp job with a negative length or without a start score"; return LAMSA_HP_EINVAL; }
        }
        if (cls == 1 && !lj_params_ok(&h->para)) {          // as the read path does: these parameters stay on the wave routines
            kind_v.assign(J->kind, J->kind + n);
            for (int i = 0; i < n; ++i) kind_v[i] -= 4;
            cls = 0;
        } else {
            int64_t tot = 0;
            for (int i = 0; i < n; ++i) tot += J->tlen[i];
            pac.assign((size_t)tot / 4 + 16, 0); tkv.assign((size_t)n + 1, 0);
            int64_t k = 0;
            for (int i = 0; i < n; ++i) {
                tkv[i] = k;
                for (int j = 0; j < J->tlen[i]; ++j, ++k) {
                    const uint8_t b = J->seq[J->t_off[i] + j];
                    if (b > 3) { h->err = "these routines read the target 2 bits per base: no N"; return LAMSA_HP_EINVAL; }
                    pac[(size_t)(k >> 2)] |= (uint8_t)(b << ((~k & 3) << 1));
                }
            }
            if (cls == 1) z_need = sizeof(cig_t) * 3 * HP_LJ_CIG * 64 + (size_t)HP_LJ_QCAP * HP_LJ_TCAP * 64 + 64;
        }
    }
    const int32_t *kind_src = kind_v.empty() ? J->kind : kind_v.data();
    size_t slab_per_wave = al256(z_need);
    int n_waves = h->n_cu * (cls == 1 ? 3 : (cls == 2 ? 16 : 8));
    if (cls == 2) {   // every job's worst case: the wave routines' scratch (above: computed from the forward band) plus the staged sequences
        size_t zz = 4096;
        for (int i = 0; i < n; ++i) {
            const size_t ql = (size_t)J->qlen[i], tl = (size_t)J->tlen[i];
            const size_t wmax = std::max<size_t>((size_t)abs((int)ql - (int)tl) + 3, (size_t)std::max(J->w[i], h->para.band_w));
            const size_t ncol = std::max<size_t>(std::min(ql, 2 * wmax + 1), 256);
            zz = std::max(zz, 2 * (ql + tl + 64) + 2 * 4 * (ql + 18) + 8 * (tl + 17) + ncol * tl + 64 + 4 * 4 * (ql + tl + 72) + 4096);
        }
        slab_per_wave = al256(zz);
    }
    if (n_waves > n) n_waves = n > 0 ? n : 1;
    while (n_waves > 1 && slab_per_wave * (size_t)n_waves > ((size_t)64 << 30)) n_waves /= 2;

    // ---- pack inputs into one upload
    size_t o_seq = 0, o_qoff = al256((size_t)J->seq_bytes + 16), o_toff = o_qoff + al256(8 * (size_t)n), o_cap = o_toff + al256(8 * (size_t)n),
           o_ql = o_cap + al256(8 * ((size_t)n + 1)), o_tl = o_ql + al256(4 * (size_t)n), o_kind = o_tl + al256(4 * (size_t)n),
           o_w = o_kind + al256(4 * (size_t)n), o_h0 = o_w + al256(4 * (size_t)n), in_bytes = o_h0 + al256(4 * (size_t)n);
    if (h->in.ensure(in_bytes)) { h->err = "hipMalloc(in)"; return LAMSA_HP_ENOMEM; }
    size_t o_score = 0, o_qle = al256(4 * (size_t)n), o_tle = 2 * o_qle, o_st = 3 * o_qle, o_cn = 4 * o_qle, o_cig = 5 * o_qle, out_bytes = o_cig + al256(4 * (size_t)cap_off[n] + 16);
    if (h->out.ensure(out_bytes)) { h->err = "hipMalloc(out)"; return LAMSA_HP_ENOMEM; }
    if (h->slab.ensure(slab_per_wave * (size_t)n_waves)) { h->err = "hipMalloc(slab)"; return LAMSA_HP_ENOMEM; }
    if (h->misc.ensure(256)) { h->err = "hipMalloc(misc)"; return LAMSA_HP_ENOMEM; }
    char *din = (char *)h->in.p, *dout = (char *)h->out.p;
    hipStream_t s = h->stream;
    if (n > 0) {
        HIPCHK(h, hipMemcpyAsync(din + o_seq, J->seq, (size_t)J->seq_bytes, hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(din + o_qoff, J->q_off, 8 * (size_t)n, hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(din + o_toff, J->t_off, 8 * (size_t)n, hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(din + o_cap, cap_off.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(din + o_ql, J->qlen, 4 * (size_t)n, hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(din + o_tl, J->tlen, 4 * (size_t)n, hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(din + o_kind, kind_src, 4 * (size_t)n, hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(din + o_w, J->w, 4 * (size_t)n, hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(din + o_h0, J->h0, 4 * (size_t)n, hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
    }
    HIPCHK(h, hipMemsetAsync(h->misc.p, 0, 256, s), LAMSA_HP_EKERNEL);

    DpBatchArgs a;
    a.P = h->para; a.n_jobs = n;
    a.seq = (const uint8_t *)(din + o_seq); a.q_off = (const int64_t *)(din + o_qoff); a.t_off = (const int64_t *)(din + o_toff);
    a.qlen = (const int32_t *)(din + o_ql); a.tlen = (const int32_t *)(din + o_tl); a.kind = (const int32_t *)(din + o_kind);
    a.w = (const int32_t *)(din + o_w); a.h0 = (const int32_t *)(din + o_h0);
    a.score = (int32_t *)(dout + o_score); a.qle = (int32_t *)(dout + o_qle); a.tle = (int32_t *)(dout + o_tle);
    a.status = (int32_t *)(dout + o_st); a.cig_n = (int32_t *)(dout + o_cn);
    a.cig_cap_off = (const int64_t *)(din + o_cap); a.cig = (cig_t *)(dout + o_cig);
    a.slab = (char *)h->slab.p; a.slab_per_wave = slab_per_wave; a.counter = (int32_t *)h->misc.p;

    HIPCHK(h, hipEventRecord(h->ev0, s), LAMSA_HP_EKERNEL);
    if (n > 0 && cls == 0) hipLaunchKernelGGL(k_dp_batch, dim3(n_waves), dim3(64), 0, s, a);
    else if (n > 0) {
        const size_t pb = al256(pac.size()), tb = al256(8 * ((size_t)n + 1));
        if (h->pac2.ensure(pb + tb)) { h->err = "hipMalloc(pac)"; return LAMSA_HP_ENOMEM; }
        HIPCHK(h, hipMemcpy(h->pac2.p, pac.data(), pac.size(), hipMemcpyHostToDevice), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpy((char *)h->pac2.p + pb, tkv.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice), LAMSA_HP_EKERNEL);
        if (cls == 1) hipLaunchKernelGGL(k_dp_batch_lane, dim3(n_waves), dim3(64), 0, s, a, (const uint8_t *)h->pac2.p, (const int64_t *)((char *)h->pac2.p + pb));
        else hipLaunchKernelGGL(k_dp_batch_wave, dim3(n_waves), dim3(64), 0, s, a, (const uint8_t *)h->pac2.p, (const int64_t *)((char *)h->pac2.p + pb));
    }
    HIPCHK(h, hipGetLastError(), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipEventRecord(h->ev1, s), LAMSA_HP_EKERNEL);

    // ---- fetch results, compact the CIGARs
    h->h_score.assign((size_t)n, 0); h->h_qle.assign((size_t)n, 0); h->h_tle.assign((size_t)n, 0); h->h_status.assign((size_t)n, 0);
    std::vector<int32_t> cn((size_t)n, 0), raw((size_t)cap_off[n] + 4, 0);
    if (n > 0) {
        HIPCHK(h, hipMemcpyAsync(h->h_score.data(), dout + o_score, 4 * (size_t)n, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(h->h_qle.data(), dout + o_qle, 4 * (size_t)n, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(h->h_tle.data(), dout + o_tle, 4 * (size_t)n, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(h->h_status.data(), dout + o_st, 4 * (size_t)n, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(cn.data(), dout + o_cn, 4 * (size_t)n, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(raw.data(), dout + o_cig, 4 * (size_t)cap_off[n], hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
    }
    HIPCHK(h, hipStreamSynchronize(s), LAMSA_HP_EKERNEL);
    hipEventElapsedTime(&h->kernel_ms[0], h->ev0, h->ev1);
    h->h_i64.assign((size_t)n + 1, 0);
    h->h_cig.clear();
    for (int i = 0; i < n; ++i) {
        h->h_i64[i] = (int64_t)h->h_cig.size();
        h->h_cig.insert(h->h_cig.end(), raw.begin() + cap_off[i], raw.begin() + cap_off[i] + cn[i]);
    }
    h->h_i64[n] = (int64_t)h->h_cig.size();
    if (h->h_cig.empty()) h->h_cig.push_back(0);
    O->score = h->h_score.data(); O->qle = h->h_qle.data(); O->tle = h->h_tle.data(); O->status = h->h_status.data();
    O->cig_off = h->h_i64.data(); O->cigar = h->h_cig.data();
    return LAMSA_HP_OK;
}

// ------------------------------------------------------------------ the resident FM index: lamsa_hp_fm_load / lamsa_hp_fm_search
#include "hp_fm.h"

// Plain grids, 256 lanes per workgroup, grid-strided beyond 2 048 workgroups (8 waves on every SIMD of 256 CUs).  Consecutive lanes take
// consecutive k-mers / positions: a wave's query bytes are one stretch and its stores are coalesced.  No LDS; 64 VGPRs at the most.
enum { FM_BLOCK = 256, FM_MAX_GRID = 2048 };
__global__ __launch_bounds__(FM_BLOCK, 8) void k_fm_search(FmSearchArgs a)
{
    const int64_t step = (int64_t)gridDim.x * FM_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * FM_BLOCK + threadIdx.x; j < a.n_kmers; j += step) fm_search_lane(a, j);
}
__global__ __launch_bounds__(FM_BLOCK, 8) void k_fm_locate(FmLocateArgs a)
{
    const int64_t step = (int64_t)gridDim.x * FM_BLOCK;
    for (int64_t t = a.t0 + (int64_t)blockIdx.x * FM_BLOCK + threadIdx.x; t < a.t1; t += step) fm_locate_lane(a, t);
}
// the scan of the counts between the two: one wave per workgroup, a tile of HP_FM_TILE counts per wave
__global__ __launch_bounds__(64) void k_fm_scan_sums(FmScanArgs a) { for (int64_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) fm_scan_sums(a, t); }
__global__ __launch_bounds__(64) void k_fm_scan_tiles(FmScanArgs a) { fm_scan_tiles(a); }
__global__ __launch_bounds__(64) void k_fm_scan_write(FmScanArgs a) { for (int64_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) fm_scan_write(a, t); }

static void fm_drop(lamsa_hp_handle *h)
{
    if (h->fm_bwt) hipFree(h->fm_bwt);
    if (h->fm_sa) hipFree(h->fm_sa);
    h->fm_bwt = h->fm_sa = nullptr;
}

extern "C" int lamsa_hp_fm_load(lamsa_hp_handle *h, const lamsa_hp_fm_index *ix)
{
    if (!h) return LAMSA_HP_EINVAL;
    HIPCHK(h, hipSetDevice(h->device), LAMSA_HP_ENODEV);
    fm_drop(h);                                               // whatever happens, the earlier index is gone
    if (!ix || !ix->bwt || !ix->sa) { h->err = "fm index: null pointer"; return LAMSA_HP_EINVAL; }
    bool ok = ix->seq_len > 0 && ix->seq_len < ((uint64_t)1 << 62) && ix->primary >= 1 && ix->primary <= ix->seq_len && ix->L2[0] == 0 && ix->L2[4] == ix->seq_len &&
              ix->sa_intv > 0 && (ix->sa_intv & (ix->sa_intv - 1)) == 0;
    for (int c = 0; ok && c < 4; ++c) ok = ix->L2[c] <= ix->L2[c + 1];
    ok = ok && ix->bwt_words >= ((ix->seq_len + 15) >> 4) + ((ix->seq_len + 127) >> 7) * 8 && ix->bwt_words < ((uint64_t)1 << 60) &&
         ix->n_sa == (ix->seq_len + ix->sa_intv) / ix->sa_intv;
    if (!ok) { h->err = "fm index: sizes that contradict each other"; return LAMSA_HP_EINVAL; }
    const size_t bb = (size_t)ix->bwt_words * 4, sb = (size_t)ix->n_sa * 8;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (bb + 64 > total_b || sb > total_b - (bb + 64))) { h->err = "fm index: larger than the device memory"; return LAMSA_HP_ENOMEM; }
    // 64 bytes behind the words: the last block is read whole wherever the file ends inside it
    if (hipMalloc(&h->fm_bwt, bb + 64) != hipSuccess) { h->fm_bwt = nullptr; (void)hipGetLastError(); h->err = "hipMalloc(fm bwt)"; return LAMSA_HP_ENOMEM; }
    if (hipMalloc(&h->fm_sa, sb) != hipSuccess) { h->fm_sa = nullptr; (void)hipGetLastError(); fm_drop(h); h->err = "hipMalloc(fm sa)"; return LAMSA_HP_ENOMEM; }
    if (hipMemset((char *)h->fm_bwt + bb, 0, 64) != hipSuccess || hipMemcpy(h->fm_bwt, ix->bwt, bb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->fm_sa, ix->sa, sb, hipMemcpyHostToDevice) != hipSuccess) { fm_drop(h); h->err = "fm index: copy to the device failed"; return LAMSA_HP_EKERNEL; }
    h->fm_ix = *ix; h->fm_ix.bwt = nullptr; h->fm_ix.sa = nullptr;
    return LAMSA_HP_OK;
}

extern "C" int lamsa_hp_fm_search(lamsa_hp_handle *h, const lamsa_hp_fm_queries *q, lamsa_hp_fm_out *out)
{
    if (!h || !q || !out) return LAMSA_HP_EINVAL;
    if (!h->fm_bwt) { h->err = "fm search: no index loaded"; return LAMSA_HP_EINVAL; }
    if (q->k < 1 || q->k > 255 || q->max_occ < 0 || q->max_occ > HP_FM_MAX_OCC || q->n_win < 0 || q->seq_bytes < 0 || (q->n_win > 0 && (!q->win_off || !q->seq))) { h->err = "fm search: k outside 1..255, max_occ outside 0..2^20 or a null array"; return LAMSA_HP_EINVAL; }
    const int nw = q->n_win;
    if (nw > 0 && q->win_off[0] < 0) { h->err = "fm search: negative window offset"; return LAMSA_HP_EINVAL; }
    for (int w = 0; w < nw; ++w) if (q->win_off[w + 1] < q->win_off[w]) { h->err = "fm search: window offsets decrease"; return LAMSA_HP_EINVAL; }
    if (nw > 0 && q->win_off[nw] > q->seq_bytes) { h->err = "fm search: window beyond seq_bytes"; return LAMSA_HP_EINVAL; }
    HIPCHK(h, hipSetDevice(h->device), LAMSA_HP_ENODEV);
    h->fm_kmer_off.assign((size_t)nw + 1, 0);
    for (int w = 0; w < nw; ++w) { const int64_t len = q->win_off[w + 1] - q->win_off[w]; h->fm_kmer_off[(size_t)w + 1] = h->fm_kmer_off[(size_t)w] + (len >= q->k ? len - q->k + 1 : 0); }
    const int64_t n = h->fm_kmer_off[(size_t)nw];
    h->fm_lo.assign((size_t)n + 1, 0); h->fm_hi.assign((size_t)n + 1, 0); h->fm_pos_off.assign((size_t)n + 1, 0); h->fm_posv.assign(1, 0);
    h->kernel_ms[21] = h->kernel_ms[22] = h->kernel_ms[23] = 0;
    out->n_kmers = n; out->kmer_off = h->fm_kmer_off.data(); out->lo = h->fm_lo.data(); out->hi = h->fm_hi.data(); out->pos_off = h->fm_pos_off.data(); out->pos = h->fm_posv.data();
    if (n == 0) return LAMSA_HP_OK;

    const int64_t s0 = q->win_off[0], sbytes = q->win_off[nw] - s0;          // only the bytes the windows cover travel
    const int64_t n_tiles = (n + HP_FM_TILE - 1) / HP_FM_TILE;
    const size_t o_win = al256((size_t)sbytes + 16), o_koff = o_win + al256(8 * ((size_t)nw + 1)), in_bytes = o_koff + al256(8 * ((size_t)nw + 1));
    const size_t o_hi = al256(8 * (size_t)n), o_cnt = 2 * o_hi, o_poff = o_cnt + al256(4 * (size_t)n), o_tsum = o_poff + al256(8 * ((size_t)n + 1)),
                 o_toff = o_tsum + al256(4 * (size_t)n_tiles), out_bytes = o_toff + al256(8 * ((size_t)n_tiles + 1));
    if (h->fm_in.ensure(in_bytes)) { (void)hipGetLastError(); h->err = "hipMalloc(fm in)"; return LAMSA_HP_ENOMEM; }
    if (h->fm_out.ensure(out_bytes)) { (void)hipGetLastError(); h->err = "hipMalloc(fm out)"; return LAMSA_HP_ENOMEM; }
    char *din = (char *)h->fm_in.p, *dout = (char *)h->fm_out.p;
    hipStream_t s = h->stream;
    std::vector<int64_t> woff((size_t)nw + 1);
    for (int w = 0; w <= nw; ++w) woff[(size_t)w] = q->win_off[w] - s0;
    HIPCHK(h, hipMemcpyAsync(din, q->seq + s0, (size_t)sbytes, hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(din + o_win, woff.data(), 8 * ((size_t)nw + 1), hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(din + o_koff, h->fm_kmer_off.data(), 8 * ((size_t)nw + 1), hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);

    FmIx ix;
    ix.seq_len = h->fm_ix.seq_len; ix.primary = h->fm_ix.primary; for (int c = 0; c < 5; ++c) ix.L2[c] = h->fm_ix.L2[c];
    ix.bwt = (const uint32_t *)h->fm_bwt; ix.sa = (const uint64_t *)h->fm_sa; ix.sa_intv = h->fm_ix.sa_intv;
    FmSearchArgs a;
    a.ix = ix; a.seq = (const uint8_t *)din; a.win_off = (const int64_t *)(din + o_win); a.kmer_off = (const int64_t *)(din + o_koff);
    a.n_win = nw; a.k = q->k; a.max_occ = q->max_occ; a.n_kmers = n;
    a.lo = (uint64_t *)dout; a.hi = (uint64_t *)(dout + o_hi); a.cnt = (int32_t *)(dout + o_cnt);
    auto grid_of = [](int64_t items) { const int64_t g = (items + FM_BLOCK - 1) / FM_BLOCK; return dim3((unsigned)(g < FM_MAX_GRID ? g : FM_MAX_GRID)); };
    HIPCHK(h, hipEventRecord(h->ev0, s), LAMSA_HP_EKERNEL);
    hipLaunchKernelGGL(k_fm_search, grid_of(n), dim3(FM_BLOCK), 0, s, a);
    HIPCHK(h, hipGetLastError(), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipEventRecord(h->ev1, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(h->fm_lo.data(), a.lo, 8 * (size_t)n, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(h->fm_hi.data(), a.hi, 8 * (size_t)n, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipStreamSynchronize(s), LAMSA_HP_EKERNEL);
    hipEventElapsedTime(&h->kernel_ms[21], h->ev0, h->ev1);
    if (q->max_occ == 0) return LAMSA_HP_OK;

    // counts -> offsets on the device; the host only learns the offsets it hands out anyway
    FmScanArgs sc;
    sc.cnt = a.cnt; sc.n = n; sc.n_tiles = n_tiles; sc.tile_sum = (int32_t *)(dout + o_tsum); sc.tile_off = (int64_t *)(dout + o_toff); sc.pos_off = (int64_t *)(dout + o_poff);
    const dim3 sgrid((unsigned)(n_tiles < 8 * FM_MAX_GRID ? n_tiles : 8 * FM_MAX_GRID));
    HIPCHK(h, hipEventRecord(h->ev0, s), LAMSA_HP_EKERNEL);
    hipLaunchKernelGGL(k_fm_scan_sums, sgrid, dim3(64), 0, s, sc);
    hipLaunchKernelGGL(k_fm_scan_tiles, dim3(1), dim3(64), 0, s, sc);
    hipLaunchKernelGGL(k_fm_scan_write, sgrid, dim3(64), 0, s, sc);
    HIPCHK(h, hipGetLastError(), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipEventRecord(h->ev1, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(h->fm_pos_off.data(), sc.pos_off, 8 * ((size_t)n + 1), hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipStreamSynchronize(s), LAMSA_HP_EKERNEL);
    hipEventElapsedTime(&h->kernel_ms[23], h->ev0, h->ev1);
    const int64_t total = h->fm_pos_off[(size_t)n];
    if (total < 0 || total > n * (int64_t)q->max_occ) { h->err = "fm search: the device scan went wrong"; return LAMSA_HP_EKERNEL; }
    h->fm_posv.assign((size_t)total + 1, 0);
    out->pos = h->fm_posv.data();

    // rows -> text positions, a slice of the flat position list at a time: the device buffer stays bounded whatever n * max_occ is
    const int64_t slice = getenv("LAMSA_HP_FM_SLICE") ? std::max<int64_t>(1, atoll(getenv("LAMSA_HP_FM_SLICE"))) : ((int64_t)4 << 20);      // 32 MB of positions (tests lower it)
    if (total > 0 && h->fm_pos.ensure(8 * (size_t)std::min(slice, total))) { (void)hipGetLastError(); h->err = "hipMalloc(fm pos)"; return LAMSA_HP_ENOMEM; }
    FmLocateArgs la;
    la.ix = ix; la.lo = a.lo; la.pos_off = sc.pos_off; la.n_kmers = n; la.pos = (uint64_t *)h->fm_pos.p;
    for (int64_t t0 = 0; t0 < total; t0 += slice) {
        la.t0 = t0; la.t1 = std::min(total, t0 + slice);
        HIPCHK(h, hipEventRecord(h->ev0, s), LAMSA_HP_EKERNEL);
        hipLaunchKernelGGL(k_fm_locate, grid_of(la.t1 - la.t0), dim3(FM_BLOCK), 0, s, la);
        HIPCHK(h, hipGetLastError(), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipEventRecord(h->ev1, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(h->fm_posv.data() + t0, la.pos, 8 * (size_t)(la.t1 - la.t0), hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipStreamSynchronize(s), LAMSA_HP_EKERNEL);
        float ms = 0; hipEventElapsedTime(&ms, h->ev0, h->ev1);
        h->kernel_ms[22] += ms;
    }
    return LAMSA_HP_OK;
}

// ------------------------------------------------------------------ seeding in the resident index: lamsa_hp_fm_seed
#include "hp_seed.h"

// The same plain grids as the two FM kernels: one seed / one located row per lane, chains of dependent 64-byte block reads, no LDS.
__global__ __launch_bounds__(FM_BLOCK, 8) void k_seed_search(SeedArgs a)
{
    const int64_t step = (int64_t)gridDim.x * FM_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * FM_BLOCK + threadIdx.x; j < a.n_seeds; j += step) seed_search_lane(a, j);
}
__global__ __launch_bounds__(FM_BLOCK, 8) void k_seed_locate(SeedArgs a)
{
    const int64_t step = (int64_t)gridDim.x * FM_BLOCK;
    for (int64_t t = a.t0 + (int64_t)blockIdx.x * FM_BLOCK + threadIdx.x; t < a.t1; t += step) seed_locate_lane(a, t);
}
__global__ __launch_bounds__(FM_BLOCK, 8) void k_seed_hits(SeedArgs a)
{
    const int64_t step = (int64_t)gridDim.x * FM_BLOCK;
    for (int64_t t = a.t0 + (int64_t)blockIdx.x * FM_BLOCK + threadIdx.x; t < a.t1; t += step) seed_hits_lane(a, t);
}
__global__ __launch_bounds__(FM_BLOCK, 8) void k_seed_slot(SeedArgs a)
{
    const int64_t step = (int64_t)gridDim.x * FM_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * FM_BLOCK + threadIdx.x; j < a.n_seeds; j += step) seed_slot_lane(a, j);
}
__global__ __launch_bounds__(FM_BLOCK, 8) void k_seed_emit(SeedArgs a)
{
    const int64_t step = (int64_t)gridDim.x * FM_BLOCK, n = a.n_seeds + a.n_reads + 1;
    for (int64_t x = (int64_t)blockIdx.x * FM_BLOCK + threadIdx.x; x < n; x += step) seed_emit_lane(a, x);
}

extern "C" int lamsa_hp_fm_seed(lamsa_hp_handle *h, const lamsa_hp_seed_queries *q, lamsa_hp_batch *out)
{
    if (!h || !q || !out) return LAMSA_HP_EINVAL;
    if (!h->fm_bwt) { h->err = "fm seed: no index loaded"; return LAMSA_HP_EINVAL; }
    if (q->seed_len < 1 || q->seed_len > 63 || q->seed_step < 1 || q->max_hits < 1 || q->max_hits > HP_SEED_MAX_HITS) { h->err = "fm seed: seed_len outside 1..63, seed_step < 1 or max_hits outside 1..16383"; return LAMSA_HP_EINVAL; }
    const int n = q->n_reads, nc = q->n_seqs;
    if (n < 0 || (n > 0 && (!q->read_off || !q->read_seq))) { h->err = "fm seed: negative n_reads or a null array"; return LAMSA_HP_EINVAL; }
    // the contig table must be the one of the loaded index: contiguous from 0 to half the doubled text
    if (nc < 1 || !q->seq_offset || !q->seq_len || q->seq_offset[0] != 0) { h->err = "fm seed: empty contig table, or one that does not start at 0"; return LAMSA_HP_EINVAL; }
    for (int c = 0; c < nc; ++c)
        if (q->seq_len[c] < 0 || (c + 1 < nc && q->seq_offset[c + 1] != q->seq_offset[c] + q->seq_len[c])) { h->err = "fm seed: the contigs do not lie back to back"; return LAMSA_HP_EINVAL; }
    const int64_t l_pac = q->seq_offset[nc - 1] + q->seq_len[nc - 1];
    if ((h->fm_ix.seq_len & 1) || (uint64_t)l_pac != h->fm_ix.seq_len / 2) { h->err = "fm seed: the contig table does not end where the index's forward text ends (the index of another genome?)"; return LAMSA_HP_EINVAL; }
    if (n > 0 && q->read_off[0] != 0) { h->err = "fm seed: offsets must start at 0"; return LAMSA_HP_EINVAL; }
    const int64_t sl = q->seed_len, ss = q->seed_step;
    h->sd_all.assign((size_t)n + 1, 0); h->sd_last.assign((size_t)n + 1, 0); h->sd_off.assign((size_t)n + 1, 0); h->sd_seed_off.assign((size_t)n + 1, 0);
    for (int r = 0; r < n; ++r) {
        const int64_t L = q->read_off[r + 1] - q->read_off[r];
        if (L < 0) { h->err = "fm seed: read offsets decrease"; return LAMSA_HP_EINVAL; }
        if (L > (1 << 24)) { h->err = "fm seed: read longer than 2^24 bases"; return LAMSA_HP_EINVAL; }
        const int64_t sa = L < sl ? 0 : 1 + (L - sl) / ss;
        h->sd_all[(size_t)r] = (int32_t)sa; h->sd_last[(size_t)r] = (int32_t)(L - sl - (sa - 1) * ss);
        h->sd_off[(size_t)r + 1] = h->sd_off[(size_t)r] + sa;
    }
    const int64_t n_bases = n ? q->read_off[n] : 0, N = h->sd_off[(size_t)n];
    { unsigned bad = 0; for (int64_t i = 0; i < n_bases; ++i) bad |= q->read_seq[i] > 4; if (bad) { h->err = "fm seed: read base code > 4"; return LAMSA_HP_EINVAL; } }
    HIPCHK(h, hipSetDevice(h->device), LAMSA_HP_ENODEV);
    h->sd_seed_id.assign(1, 0); h->sd_hit_off.assign(1, 0); h->sd_pos.assign(1, 0); h->sd_chr.assign(1, 0); h->sd_strand.assign(1, 0);
    h->sd_nm.assign(1, 0); h->sd_len_dif.assign(1, 0); h->sd_cig_n.assign(1, 0); h->sd_cig8.assign(1, 0);
    h->kernel_ms[21] = h->kernel_ms[22] = h->kernel_ms[23] = 0;
    static const int64_t zero64 = 0; static const uint8_t zero8 = 0;
    int64_t n_slots = 0, n_hits = 0;
    auto hand_out = [&]() {
        out->n_reads = n; out->read_off = q->read_off ? q->read_off : &zero64; out->read_seq = q->read_seq ? q->read_seq : &zero8;
        out->seed_all = h->sd_all.data(); out->last_len = h->sd_last.data(); out->seed_off = h->sd_seed_off.data(); out->seed_id = h->sd_seed_id.data(); out->hit_off = h->sd_hit_off.data();
        out->h_pos = h->sd_pos.data(); out->h_chr = h->sd_chr.data(); out->h_strand = h->sd_strand.data(); out->h_nm = h->sd_nm.data(); out->h_len_dif = h->sd_len_dif.data();
        out->h_cig_off = nullptr; out->h_cig_n = h->sd_cig_n.data(); out->cig = nullptr; out->n_cig = n_hits; out->cig8 = h->sd_cig8.data();
    };
    hand_out();
    if (N == 0) return LAMSA_HP_OK;

    const int64_t slice = getenv("LAMSA_HP_FM_SLICE") ? std::max<int64_t>(1, atoll(getenv("LAMSA_HP_FM_SLICE"))) : ((int64_t)4 << 20);      // rows located per pass (tests lower it)
    const size_t nN = (size_t)N, nT = (size_t)((N + HP_FM_TILE - 1) / HP_FM_TILE);
    const size_t i_off = al256((size_t)n_bases + 16), i_sd = i_off + al256(8 * ((size_t)n + 1)), i_co = i_sd + al256(8 * ((size_t)n + 1)), i_cl = i_co + al256(8 * (size_t)nc), in_bytes = i_cl + al256(4 * (size_t)nc);
    const size_t o_cnt = al256(8 * nN), o_over = o_cnt + al256(4 * nN), o_kept = o_over + al256(4 * nN), o_slot = o_kept + al256(4 * nN), o_roff = o_slot + al256(4 * nN),
                 o_soff = o_roff + al256(8 * (nN + 1)), o_koff = o_soff + al256(8 * (nN + 1)), o_sid = o_koff + al256(8 * (nN + 1)), o_hoff = o_sid + al256(4 * nN),
                 o_sdo = o_hoff + al256(8 * (nN + 1)), o_tsum = o_sdo + al256(8 * ((size_t)n + 1)), o_toff = o_tsum + al256(4 * nT), out_bytes = o_toff + al256(8 * (nT + 1));
    if (h->fm_in.ensure(in_bytes)) { (void)hipGetLastError(); h->err = "hipMalloc(fm seed in)"; return LAMSA_HP_ENOMEM; }
    if (h->fm_out.ensure(out_bytes)) { (void)hipGetLastError(); h->err = "hipMalloc(fm seed out)"; return LAMSA_HP_ENOMEM; }
    char *din = (char *)h->fm_in.p, *dout = (char *)h->fm_out.p;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(din, q->read_seq, (size_t)n_bases, hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(din + i_off, q->read_off, 8 * ((size_t)n + 1), hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(din + i_sd, h->sd_off.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(din + i_co, q->seq_offset, 8 * (size_t)nc, hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(din + i_cl, q->seq_len, 4 * (size_t)nc, hipMemcpyHostToDevice, s), LAMSA_HP_EKERNEL);

    SeedArgs a; memset(&a, 0, sizeof a);
    a.ix.seq_len = h->fm_ix.seq_len; a.ix.primary = h->fm_ix.primary; for (int c = 0; c < 5; ++c) a.ix.L2[c] = h->fm_ix.L2[c];
    a.ix.bwt = (const uint32_t *)h->fm_bwt; a.ix.sa = (const uint64_t *)h->fm_sa; a.ix.sa_intv = h->fm_ix.sa_intv;
    a.read_seq = (const uint8_t *)din; a.read_off = (const int64_t *)(din + i_off); a.sd_off = (const int64_t *)(din + i_sd);
    a.n_reads = n; a.seed_len = q->seed_len; a.seed_step = q->seed_step; a.max_hits = q->max_hits; a.n_seeds = N;
    a.seq_offset = (const int64_t *)(din + i_co); a.seq_len = (const int32_t *)(din + i_cl); a.n_seqs = nc; a.l_pac = l_pac;
    a.lo = (uint64_t *)dout; a.cnt = (int32_t *)(dout + o_cnt); a.over = (int32_t *)(dout + o_over); a.kept = (int32_t *)(dout + o_kept); a.slot = (int32_t *)(dout + o_slot);
    a.row_off = (const int64_t *)(dout + o_roff); a.slot_off = (const int64_t *)(dout + o_soff); a.kept_off = (const int64_t *)(dout + o_koff);
    a.seed_id = (int32_t *)(dout + o_sid); a.hit_off = (int64_t *)(dout + o_hoff); a.seed_off = (int64_t *)(dout + o_sdo);
    auto grid_of = [](int64_t items) { const int64_t g = (items + FM_BLOCK - 1) / FM_BLOCK; return dim3((unsigned)(g < FM_MAX_GRID ? g : FM_MAX_GRID)); };
    auto scan = [&](const int32_t *cnt, int64_t items, const int64_t *off, char *tiles) {       // exclusive scan of cnt[items] -> off[items + 1]; tiles: the tile sums, then their offsets
        FmScanArgs sc;
        sc.cnt = cnt; sc.n = items; sc.n_tiles = (items + HP_FM_TILE - 1) / HP_FM_TILE; sc.pos_off = (int64_t *)off;
        sc.tile_sum = (int32_t *)tiles; sc.tile_off = (int64_t *)(tiles + al256(4 * (size_t)sc.n_tiles));
        const dim3 sgrid((unsigned)(sc.n_tiles < 8 * FM_MAX_GRID ? sc.n_tiles : 8 * FM_MAX_GRID));
        hipLaunchKernelGGL(k_fm_scan_sums, sgrid, dim3(64), 0, s, sc);
        hipLaunchKernelGGL(k_fm_scan_tiles, dim3(1), dim3(64), 0, s, sc);
        hipLaunchKernelGGL(k_fm_scan_write, sgrid, dim3(64), 0, s, sc);
    };
    float ms = 0;
    // ---- seeds -> row intervals -> the flat row list
    int64_t total = 0;
    HIPCHK(h, hipEventRecord(h->ev0, s), LAMSA_HP_EKERNEL);
    hipLaunchKernelGGL(k_seed_search, grid_of(N), dim3(FM_BLOCK), 0, s, a);
    scan(a.cnt, N, a.row_off, dout + o_tsum);
    HIPCHK(h, hipGetLastError(), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipEventRecord(h->ev1, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(&total, a.row_off + N, 8, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipStreamSynchronize(s), LAMSA_HP_EKERNEL);
    hipEventElapsedTime(&h->kernel_ms[21], h->ev0, h->ev1);
    if (total < 0 || total > N * (int64_t)q->max_hits) { h->err = "fm seed: the device scan went wrong"; return LAMSA_HP_EKERNEL; }

    // ---- rows -> hits, a slice of the flat row list at a time: the device buffers stay bounded whatever n_seeds * max_hits is, and the hits of
    // a slice, compacted in flat row order, are the next hits of the batch
    const size_t m_max = (size_t)std::min(slice, total), mT = (m_max + HP_FM_TILE - 1) / HP_FM_TILE;
    const size_t p_pos = al256(8 * m_max), p_chr = 2 * p_pos, p_keep = p_chr + al256(4 * m_max), p_koff = p_keep + al256(4 * m_max), p_spos = p_koff + al256(8 * (m_max + 1)),
                 p_schr = p_spos + al256(8 * m_max), p_sstr = p_schr + al256(4 * m_max), p_tiles = p_sstr + al256(m_max), pos_bytes = p_tiles + al256(4 * mT) + al256(8 * (mT + 1));
    if (total > 0 && h->fm_pos.ensure(pos_bytes)) { (void)hipGetLastError(); h->err = "hipMalloc(fm seed rows)"; return LAMSA_HP_ENOMEM; }
    char *dp = (char *)h->fm_pos.p;
    a.p_seed = (int64_t *)dp; a.p_pos = (int64_t *)(dp + p_pos); a.p_chr = (int32_t *)(dp + p_chr); a.keep = (int32_t *)(dp + p_keep); a.keep_off = (const int64_t *)(dp + p_koff);
    a.s_pos = (int64_t *)(dp + p_spos); a.s_chr = (int32_t *)(dp + p_schr); a.s_strand = (int8_t *)(dp + p_sstr);
    h->sd_pos.clear(); h->sd_chr.clear(); h->sd_strand.clear();
    h->sd_pos.reserve((size_t)total + 1); h->sd_chr.reserve((size_t)total + 1); h->sd_strand.reserve((size_t)total + 1);
    for (int64_t t0 = 0; t0 < total; t0 += slice) {
        a.t0 = t0; a.t1 = std::min(total, t0 + slice);
        const int64_t m = a.t1 - a.t0;
        int64_t got = 0;
        HIPCHK(h, hipEventRecord(h->ev0, s), LAMSA_HP_EKERNEL);
        hipLaunchKernelGGL(k_seed_locate, grid_of(m), dim3(FM_BLOCK), 0, s, a);
        scan(a.keep, m, a.keep_off, dp + p_tiles);
        hipLaunchKernelGGL(k_seed_hits, grid_of(m), dim3(FM_BLOCK), 0, s, a);
        HIPCHK(h, hipGetLastError(), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipEventRecord(h->ev1, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(&got, a.keep_off + m, 8, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipStreamSynchronize(s), LAMSA_HP_EKERNEL);
        hipEventElapsedTime(&ms, h->ev0, h->ev1); h->kernel_ms[22] += ms;
        if (got < 0 || got > m) { h->err = "fm seed: the device scan went wrong"; return LAMSA_HP_EKERNEL; }
        if (got == 0) continue;
        const size_t at = (size_t)n_hits;
        n_hits += got;
        h->sd_pos.resize((size_t)n_hits); h->sd_chr.resize((size_t)n_hits); h->sd_strand.resize((size_t)n_hits);
        HIPCHK(h, hipMemcpyAsync(h->sd_pos.data() + at, a.s_pos, 8 * (size_t)got, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(h->sd_chr.data() + at, a.s_chr, 4 * (size_t)got, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipMemcpyAsync(h->sd_strand.data() + at, a.s_strand, (size_t)got, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
        HIPCHK(h, hipStreamSynchronize(s), LAMSA_HP_EKERNEL);
    }

    // ---- slots: a seed with a kept row, or with more rows than max_hits; then every slot's seed id and first hit, every read's first slot
    int64_t ends[2] = {0, 0};
    HIPCHK(h, hipEventRecord(h->ev0, s), LAMSA_HP_EKERNEL);
    hipLaunchKernelGGL(k_seed_slot, grid_of(N), dim3(FM_BLOCK), 0, s, a);
    scan(a.slot, N, a.slot_off, dout + o_tsum);
    scan(a.kept, N, a.kept_off, dout + o_tsum);
    hipLaunchKernelGGL(k_seed_emit, grid_of(N + n + 1), dim3(FM_BLOCK), 0, s, a);
    HIPCHK(h, hipGetLastError(), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipEventRecord(h->ev1, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(&ends[0], a.slot_off + N, 8, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(&ends[1], a.kept_off + N, 8, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(h->sd_seed_off.data(), a.seed_off, 8 * ((size_t)n + 1), hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipStreamSynchronize(s), LAMSA_HP_EKERNEL);
    hipEventElapsedTime(&h->kernel_ms[23], h->ev0, h->ev1);
    n_slots = ends[0];
    if (n_slots < 0 || n_slots > N || ends[1] != n_hits) { h->err = "fm seed: the slices' hits and the seeds' counts do not add up"; return LAMSA_HP_EKERNEL; }
    h->sd_seed_id.assign((size_t)n_slots + 1, 0); h->sd_hit_off.assign((size_t)n_slots + 1, 0);
    if (n_slots > 0) HIPCHK(h, hipMemcpyAsync(h->sd_seed_id.data(), a.seed_id, 4 * (size_t)n_slots, hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipMemcpyAsync(h->sd_hit_off.data(), a.hit_off, 8 * ((size_t)n_slots + 1), hipMemcpyDeviceToHost, s), LAMSA_HP_EKERNEL);
    HIPCHK(h, hipStreamSynchronize(s), LAMSA_HP_EKERNEL);
    // what is the same for every exact hit never crosses the bus: NM 0, no length difference, one CIGAR element "seed_len M"
    h->sd_pos.resize((size_t)n_hits + 1); h->sd_chr.resize((size_t)n_hits + 1); h->sd_strand.resize((size_t)n_hits + 1);
    h->sd_nm.assign((size_t)n_hits + 1, 0); h->sd_len_dif.assign((size_t)n_hits + 1, 0); h->sd_cig_n.assign((size_t)n_hits + 1, 1); h->sd_cig8.assign((size_t)n_hits + 1, (uint8_t)q->seed_len);
    hand_out();
    return LAMSA_HP_OK;
}
