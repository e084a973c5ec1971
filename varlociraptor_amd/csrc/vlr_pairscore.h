// vlr_pairscore.h — what the sessions that realign read windows against allele windows have in common (vlr_indelpileup.hip: indel
// candidates; vlr_fragpileup.hip: indel-bearing reads over SNV / MNV candidates): the window gather, the band rule, the scoring of a
// range of pairs through the engine's own edit-distance and pair-HMM kernels (vlr_realign.hip, entered through vlr_launch_*), the
// collect pass, and the normalisation of mod.rs:358-376 for the host.  Internal to those .hip files, in the spirit of vlr_bamsession.h.
//
// Pair 2e = (ref allele window, read window), pair 2e + 1 = (alt allele window, read window) of evidence e.  Bounds: the gather pass
// writes window byte k of a pair only below the pair's own length as its offsets state it, and reads the contig and the record only
// through vlr_ip::window_byte, which checks every index.
#pragma once
#include <cmath>

#include "vlr_bamsession.h"
#include "vlr_indelpileup.h"

extern "C" int vlr_launch_edit_kernel(const vlr_realign_batch_desc* b, int32_t* dist, int32_t* end, int32_t* n_hits, void* stream);
extern "C" int vlr_launch_realign_kernel(const vlr_realign_batch_desc* b, double* ln_prob, void* stream);
extern "C" int vlr_launch_pathhmm_kernel(const vlr_realign_batch_desc* b, double* ln_prob, void* stream);
extern "C" int vlr_launch_homopoly_kernel(const vlr_realign_batch_desc* b, const double* hop, double* ln_prob, void* stream);

namespace vlr_ip {

constexpr int kThreads = 256;
constexpr int kEditBand = 4;                 // pairhmm.rs:20
constexpr uint64_t kPairByteLimit = 1ull << 31;

// where the read windows of an evidence come from (chunk-local, one per evidence)
struct Src {
    uint64_t seq, qual;   // offsets of the record's packed SEQ and its QUAL from the chunk's base
    uint32_t l_seq, pad;
};

// The reference of a realigning session: the contigs its loci lie on are read when a BAM header names them, upper-cased and uploaded
// once; entry k of the table = contig k of the header of the file being read (length -1: no locus lies on it).
struct ContigTable {
    std::string fasta;
    vlr_bam::Fai fai;
    vlr_bam::Contigs contigs;        // uploaded contigs by name
    const uint8_t** d_ctg = nullptr; int64_t* d_len = nullptr; size_t cap = 0;
    std::vector<int64_t> h_len;      // the lengths of the table, on the host

    int on_header(const std::vector<int32_t>& locus_ref_id, const std::vector<std::string>& names, const char* path) {
        using vlr_bam::bfail;
        using vlr_bam::grow;
        const size_t n = names.size();
        std::vector<const uint8_t*> ctg(n + 1, nullptr);
        h_len.assign(n + 1, -1);
        for (int32_t id : locus_ref_id) {
            if ((size_t)id >= n) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: a locus lies on reference id %d, the header has %zu contigs", path, (int)id, n);
            if (h_len[(size_t)id] >= 0) continue;
            std::pair<uint8_t*, uint64_t> c;
            const int rc = vlr_bam::load_contig(fasta, fai, contigs, names[(size_t)id], path, true, c);
            if (rc != VLR_OK) return rc;
            ctg[(size_t)id] = c.first; h_len[(size_t)id] = (int64_t)c.second;
        }
        if (n + 1 > cap) {
            size_t c1 = cap, c2 = cap;
            int rc;
            if ((rc = grow(d_ctg, c1, n + 1)) != VLR_OK || (rc = grow(d_len, c2, n + 1)) != VLR_OK) return rc;
            cap = std::min(c1, c2);
        }
        VLR_HIP_OK(hipMemcpy((void*)d_ctg, ctg.data(), (n + 1) * sizeof(uint8_t*), hipMemcpyHostToDevice));
        VLR_HIP_OK(hipMemcpy(d_len, h_len.data(), (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        return VLR_OK;
    }
    void free() {
        if (d_ctg) (void)hipFree((void*)d_ctg);
        if (d_len) (void)hipFree(d_len);
        for (auto& c : contigs) if (c.second.first) (void)hipFree(c.second.first);
    }
};

// the windows of an indel candidate's evidence: the alt allele window is the locus's own, computed by the caller
struct IndelWindows {
    Loci L;
    const uint8_t* const* ctg;
    const uint8_t* alt_bases;
    __device__ int64_t n_loci() const { return L.n; }
    __device__ int32_t ref_id(uint32_t locus) const { return L.ref_id[locus]; }
    __device__ const uint8_t* contig(int32_t ref_id) const { return ctg[ref_id]; }
    __device__ int64_t contig_len(int32_t ref_id) const { return L.ctg_len[ref_id]; }
    __device__ uint32_t alt_len(uint32_t locus, int64_t) const { return (uint32_t)(L.alt_off[locus + 1] - L.alt_off[locus]); }
    __device__ uint8_t alt_byte(uint32_t locus, const uint8_t*, int64_t, uint32_t k) const { return alt_bases[L.alt_off[locus] + k]; }
};

// One wave per evidence: lane-contiguous copies of its four windows.  W says where the contig of a hit lies and what byte k of its
// alt allele window is; Off is the type of the pair offsets (uint32 within a scored range, uint64 over a whole session).
template <class W, class Off>
__global__ __launch_bounds__(kThreads) void indelpileup_gather_kernel(const uint8_t* __restrict__ base, uint64_t n_ev, const vlr_indelpileup_hit* __restrict__ hits, W w,
                                                                      const Src* __restrict__ src, const Off* __restrict__ x_offset, const Off* __restrict__ y_offset,
                                                                      uint8_t* __restrict__ x_bases, uint8_t* __restrict__ y_bases, uint8_t* __restrict__ y_quals) {
    const uint64_t e = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (e >= n_ev) return;
    const vlr_indelpileup_hit h = hits[e];
    if (h.status || (int64_t)h.locus >= w.n_loci()) return;
    const int32_t ref_id = w.ref_id(h.locus);
    const uint8_t* contig = w.contig(ref_id);
    const int64_t contig_len = w.contig_len(ref_id);
    const Src s = src[e];
    const Off x_ref = x_offset[2 * e], x_alt = x_offset[2 * e + 1], x_end = x_offset[2 * e + 2];
    const Off y_ref = y_offset[2 * e], y_alt = y_offset[2 * e + 1], y_end = y_offset[2 * e + 2];
    for (uint32_t k = lane; k < h.ref_len && x_ref + k < x_alt; k += 64) x_bases[x_ref + k] = window_byte(WB_REF_BASE, contig, contig_len, h.ref_begin, k);
    const uint32_t alt_len = w.alt_len(h.locus, contig_len);
    for (uint32_t k = lane; k < alt_len && x_alt + k < x_end; k += 64) x_bases[x_alt + k] = w.alt_byte(h.locus, contig, contig_len, k);
    for (uint32_t k = lane; k < h.read_len && y_ref + k < y_alt && y_alt + k < y_end; k += 64) {
        const uint8_t b = window_byte(WB_READ_BASE, base + s.seq, s.l_seq, h.read_begin, k);
        const uint8_t q = window_byte(WB_READ_QUAL, base + s.qual, s.l_seq, h.read_begin, k);
        y_bases[y_ref + k] = b; y_quals[y_ref + k] = q;
        y_bases[y_alt + k] = b; y_quals[y_alt + k] = q;
    }
}

static __global__ __launch_bounds__(kThreads) void indelpileup_band_kernel(const int32_t* __restrict__ dist, int64_t n_pairs, int32_t* __restrict__ band) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n_pairs) band[p] = dist[p] >= 0 ? dist[p] + kEditBand : -1;
}

static __global__ __launch_bounds__(kThreads) void indelpileup_collect_kernel(const double* __restrict__ lnp, const int32_t* __restrict__ dist, uint64_t n_ev, uint64_t hit0,
                                                                              uint64_t capacity, vlr_indelpileup_hit* __restrict__ hits) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_ev || hit0 + e >= capacity) return;
    vlr_indelpileup_hit* h = hits + hit0 + e;
    h->ln_ref = lnp[2 * e]; h->ln_alt = lnp[2 * e + 1];
    h->dist_ref = dist[2 * e]; h->dist_alt = dist[2 * e + 1];
}

inline int sync_stage(hipStream_t st, double& t, double& t0) {
    VLR_HIP_OK(hipStreamSynchronize(st));
    VLR_HIP_OK(hipGetLastError());
    const double now = vlr_bam::now_s();
    t += now - t0;
    t0 = now;
    return VLR_OK;
}

// how a session scores its pairs: --pairhmm-mode with the gap and homopolymer parameters of the alignment properties
struct ScoreParams {
    int mode = VLR_INDELPILEUP_EXACT;
    double gap[4] = {0, 0, 0, 0};
    double hop[16];
};

// the checks of the open calls on window, mode, gap and hop; fills `sp`
inline int check_score_params(const char* api, int window, int mode, const double gap[4], const double* hop, ScoreParams& sp) {
    using vlr_bam::bfail;
    if (window < 1 || window > VLR_INDELPILEUP_MAX_WINDOW)
        return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: window %d outside 1 .. %d (a read window must fit the 128 bases of the kernels)", api, window, VLR_INDELPILEUP_MAX_WINDOW);
    if (mode != VLR_INDELPILEUP_EXACT && mode != VLR_INDELPILEUP_FAST && mode != VLR_INDELPILEUP_HOMOPOLYMER) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: unknown mode %d", api, mode);
    for (int k = 0; k < 4; ++k)
        if (gap[k] != gap[k] || gap[k] > 0.0) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: gap[%d] is not a log probability", api, k);
    if (std::exp(gap[0]) + std::exp(gap[1]) > 1.0 + 1e-12) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: P(gap in x) + P(gap in y) exceeds one", api);
    if (mode == VLR_INDELPILEUP_HOMOPOLYMER) {
        if (!hop) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: null hop parameters", api);
        for (int k = 0; k < 16; ++k)
            if (!(hop[k] <= 0.0)) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: hop parameter %d is not a ln probability", api, k);
    }
    sp.mode = mode;
    for (int k = 0; k < 4; ++k) sp.gap[k] = gap[k];
    for (int k = 0; k < 16; ++k) sp.hop[k] = hop && mode == VLR_INDELPILEUP_HOMOPOLYMER ? hop[k] : -HUGE_VAL;
    return VLR_OK;
}

// Score np pairs whose offsets, bytes and bands (-1) lie on the device: the edit-distance kernel, band = distance + 4 (not in fast
// mode), the pair HMM of the mode.  dist[np] and lnp[np] come back filled; t_edit / t_hmm take the seconds of the two stages from t0 on.
inline int score_pairs(const ScoreParams& sp, size_t np, const uint32_t* d_xoff, const uint8_t* d_xb, const uint32_t* d_yoff, const uint8_t* d_yb, const uint8_t* d_yq,
                       int32_t* d_band, int32_t* d_dist, double* d_lnp, hipStream_t st, double& t_edit, double& t_hmm, double& t0) {
    using vlr_bam::bfail;
    int rc;
    vlr_realign_batch_desc b;
    b.n_pairs = (int64_t)np;
    b.x_offset = d_xoff; b.x_bases = d_xb; b.y_offset = d_yoff; b.y_bases = d_yb; b.y_quals = d_yq;
    b.max_edit_dist = d_band;
    for (int k = 0; k < 4; ++k) b.gap[k] = sp.gap[k];
    const unsigned pair_blocks = (unsigned)((np + kThreads - 1) / kThreads);
    hipError_t e = (hipError_t)vlr_launch_edit_kernel(&b, d_dist, nullptr, nullptr, (void*)st);
    if (e != hipSuccess) return bfail(VLR_ERR_HIP, "edit-distance kernel launch: %s", hipGetErrorString(e));
    if (sp.mode != VLR_INDELPILEUP_FAST) hipLaunchKernelGGL(indelpileup_band_kernel, dim3(pair_blocks), dim3(kThreads), 0, st, d_dist, (int64_t)np, d_band);
    if ((rc = sync_stage(st, t_edit, t0)) != VLR_OK) return rc;
    if (sp.mode == VLR_INDELPILEUP_FAST) e = (hipError_t)vlr_launch_pathhmm_kernel(&b, d_lnp, (void*)st);
    else if (sp.mode == VLR_INDELPILEUP_HOMOPOLYMER) e = (hipError_t)vlr_launch_homopoly_kernel(&b, sp.hop, d_lnp, (void*)st);
    else e = (hipError_t)vlr_launch_realign_kernel(&b, d_lnp, (void*)st);
    if (e != hipSuccess) return bfail(VLR_ERR_HIP, "realign kernel launch: %s", hipGetErrorString(e));
    return sync_stage(st, t_hmm, t0);
}

// The pair HMM of the mode alone, over a batch whose bands are already set (a session with competitors: the edit distances of all pairs
// are taken first, and only the pairs its select pass keeps come here).  Not synchronised.
inline int score_hmm(const ScoreParams& sp, const vlr_realign_batch_desc& b, double* d_lnp, hipStream_t st) {
    hipError_t e;
    if (sp.mode == VLR_INDELPILEUP_FAST) e = (hipError_t)vlr_launch_pathhmm_kernel(&b, d_lnp, (void*)st);
    else if (sp.mode == VLR_INDELPILEUP_HOMOPOLYMER) e = (hipError_t)vlr_launch_homopoly_kernel(&b, sp.hop, d_lnp, (void*)st);
    else e = (hipError_t)vlr_launch_realign_kernel(&b, d_lnp, (void*)st);
    if (e != hipSuccess) return vlr_bam::bfail(VLR_ERR_HIP, "realign kernel launch: %s", hipGetErrorString(e));
    return VLR_OK;
}

}  // namespace vlr_ip
