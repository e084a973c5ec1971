// vlr_indelpileup.hip — indel allele supports from BAM records for gfx950 (vlr_indelpileup_*, include/vlr.h): the evidence text of
// vlr_indelpileup.h over every record of a BAM file streamed through the device reader (vlr_bamstream.h), the window gather, the
// engine's own edit-distance and pair-HMM kernels (vlr_realign.hip, through their vlr_launch_* entry points) on the gathered pairs, and
// the host driver of the session.
//
// Per chunk of split records:
//   indelpileup_count_kernel    one record per thread: decode and validate (vlr_bp::decode), find the loci the alignment with its clips
//                               overlaps, candidate region of each -> evidences and x / y bytes of the record (nothing else is written);
//                               rejected and bad records go to integer counters (sums and a minimum: order-independent)
//   vlr_bam::scan_kernel        one workgroup per count array: exclusive prefix sums -> offsets, the chunk's totals (vlr_bamsession.h,
//                               u64 counts)
//   indelpileup_fill_kernel     one record per thread: the same text again writes the evidence descriptors (the hits, scores unset) at
//                               hits[hit0 + ev_off[i] ...) and the x_offset / y_offset entries of pairs 2e (ref allele, read) and 2e + 1
//                               (alt allele, read) from the scanned byte offsets
//   indelpileup_gather_kernel   one wave per evidence: its lanes copy the read window (bases unpacked from the 4-bit SEQ, qualities; once
//                               per pair), the ref allele window from the contig and the locus's alt window, lane-contiguous — the only
//                               pass that moves more than a few bytes per item
//   vlr_launch_edit_kernel, indelpileup_band_kernel (band = dist + 4, -1 without a hit; not in fast mode), then the pair HMM of the mode
//   indelpileup_collect_kernel  one evidence per thread: ln_ref / ln_alt / dist_ref / dist_alt into the hits
// A hit's place and a pair's bytes are functions of the record order alone: no atomics decide a position, and how the file was cut
// into feeds and chunks (window_bytes) cannot change the output.  The pair offsets are uint32: a chunk whose x or y bytes pass
// kPairByteLimit is processed in record sub-ranges cut at the scanned offsets.  The hits leave the device record-major;
// vlr_indelpileup_result puts them locus-major with a stable counting sort on the host (vlr_bam::locus_major, which also keeps the
// permutation for the kept pairs).  The session's common state, the wiring of a file into the device reader and the buffer helpers are
// vlr_bamsession.h's; the contigs come through vlr_bam::load_contig (vlr_bamstream.h), upper-cased.
//
// Bounds: see vlr_indelpileup.h.  The fill pass runs only when all evidences of the chunk fit the hit buffer and writes hits[k] only for
// k < capacity; guard bytes behind the buffer are checked at the end.  The pair buffers are sized from the scanned totals before the
// fill pass, and the gather pass writes window k of a pair only below the pair's own length.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "vlr_bamsession.h"
#include "vlr_indelpileup.h"
#include "vlr_pairscore.h"

static_assert(sizeof(vlr_indelpileup_hit) == 64, "hit layout");

namespace vlr_ip {

using vlr_bam::C_BAD;
using vlr_bam::C_FIRST_BAD;
using vlr_bam::C_REJECTED;
enum { K_EV = 0, K_X = 1, K_Y = 2, K_N = 3 };   // the three counts of a record
// (kThreads, kEditBand, kPairByteLimit, Src, the gather / band / collect kernels and the scoring of a range of pairs: vlr_pairscore.h)

__global__ __launch_bounds__(kThreads) void indelpileup_count_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0, Loci L,
                                                                     int window, uint64_t* __restrict__ cnt, int64_t stride, unsigned long long* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = starts[i], end = starts[i + 1];
    const RecEvidence r = record_evidence(L, base + o, end - o, rec0 + (uint64_t)i, window, nullptr, 0);
    cnt[K_EV * stride + i] = r.n_ev;
    cnt[K_X * stride + i] = r.x_bytes;
    cnt[K_Y * stride + i] = r.y_bytes;
    if (r.cls == REC_REJECTED) atomicAdd(&counters[C_REJECTED], 1ull);
    if (r.cls == REC_BAD) { atomicAdd(&counters[C_BAD], 1ull); atomicMin(&counters[C_FIRST_BAD], (unsigned long long)(rec0 + (uint64_t)i)); }
}

// records [i0, i1) of the chunk: their evidences are [e0, e0 + n_ev) of the chunk and go to hits[hit0 + (e - e0)], their pair bytes
// start at x0 / y0 of the chunk's scanned offsets
struct Range {
    int64_t i0, i1;
    uint64_t e0, x0, y0, n_ev, x_bytes, y_bytes;
};

__global__ __launch_bounds__(kThreads) void indelpileup_fill_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, uint64_t rec0, Loci L, int window,
                                                                    const uint64_t* __restrict__ cnt, const uint64_t* __restrict__ off, int64_t stride, Range g,
                                                                    uint64_t hit0, uint64_t capacity, vlr_indelpileup_hit* __restrict__ hits, Src* __restrict__ src,
                                                                    uint32_t* __restrict__ x_offset, uint32_t* __restrict__ y_offset, int32_t* __restrict__ band) {
    const int64_t i = g.i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == g.i0) { x_offset[2 * g.n_ev] = (uint32_t)g.x_bytes; y_offset[2 * g.n_ev] = (uint32_t)g.y_bytes; }
    if (i >= g.i1 || cnt[K_EV * stride + i] == 0) return;
    const uint64_t e = off[K_EV * stride + i] - g.e0;   // first evidence of the record within the range
    const uint64_t first = hit0 + e;
    if (first >= capacity) return;
    const uint64_t o = starts[i], end = starts[i + 1];
    const RecEvidence r = record_evidence(L, base + o, end - o, rec0 + (uint64_t)i, window, hits + first, capacity - first);
    uint64_t x = off[K_X * stride + i] - g.x0, y = off[K_Y * stride + i] - g.y0;
    for (uint32_t k = 0; k < r.n_ev && e + k < g.n_ev && first + k < capacity; ++k) {
        const vlr_indelpileup_hit h = hits[first + k];
        const uint64_t alt = h.status ? 0ull : L.alt_off[h.locus + 1] - L.alt_off[h.locus];
        const uint64_t p = 2 * (e + k);
        x_offset[p] = (uint32_t)x; x += h.ref_len;
        x_offset[p + 1] = (uint32_t)x; x += alt;
        y_offset[p] = (uint32_t)y; y += h.read_len;
        y_offset[p + 1] = (uint32_t)y; y += h.read_len;
        band[p] = -1; band[p + 1] = -1;
        src[e + k] = Src{o + r.seq_off, o + r.qual_off, r.l_seq, 0u};
    }
}

}  // namespace vlr_ip

struct vlr_indelpileup : vlr_bam::Session {
    int window = 64;
    bool keep_pairs = false;
    vlr_ip::ScoreParams score;   // mode, gap, hop
    int64_t n_loci = 0;
    uint64_t capacity = 0;
    uint64_t pair_byte_limit = vlr_ip::kPairByteLimit;
    std::vector<int32_t> h_ref_id;   // of the loci
    vlr_ip::ContigTable ctg;         // the reference, the uploaded contigs and the table of the file being read
    // device state (the record arrays of the base: [K_N][rec_cap] u64 counts and their offsets; d_total[K_N])
    int32_t* d_ref_id = nullptr; int64_t *d_start = nullptr, *d_end = nullptr; uint64_t* d_alt_off = nullptr; uint8_t* d_altb = nullptr;
    vlr_indelpileup_hit* d_hits = nullptr;
    vlr_ip::Src* d_src = nullptr; uint32_t *d_xoff = nullptr, *d_yoff = nullptr; int32_t *d_band = nullptr, *d_dist = nullptr; double* d_lnp = nullptr; size_t ev_cap = 0;
    uint8_t *d_xb = nullptr, *d_yb = nullptr, *d_yq = nullptr; size_t x_cap = 0, y_cap = 0;
    vlr_ip::Loci loci{};
    // host state
    uint64_t n_total = 0;        // evidences the input produced so far
    uint64_t x_total = 0, y_total = 0;
    bool overflow = false;
    std::vector<vlr_indelpileup_hit> hits;
    std::vector<uint64_t> perm;  // hits[k] is evidence perm[k] of the record-major order
    // kept pairs, record-major: per pair its lengths, the bytes one behind the other
    std::vector<uint32_t> p_xlen, p_ylen; std::vector<int32_t> p_band; std::vector<uint8_t> p_xb, p_yb, p_yq;
    double t[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

namespace vlr_ip {
using vlr_bam::bfail;
using vlr_bam::grow;
using vlr_bam::now_s;
using vlr_bam::upload;


// the contig table of a file (vlr_pairscore.h), into the loci the kernels see
int on_header(vlr_indelpileup* s, const std::vector<std::string>& names, const char* path) {
    const int rc = s->ctg.on_header(s->h_ref_id, names, path);
    if (rc != VLR_OK) return rc;
    s->loci.n_refs = (int64_t)names.size();
    s->loci.ctg_len = s->ctg.d_len;
    return VLR_OK;
}

// fill, gather, score and collect the evidences of one record sub-range
int run_range(vlr_indelpileup* s, const uint8_t* d_base, const uint64_t* d_starts, uint64_t rec0, const Range& g, hipStream_t st) {
    int rc;
    const size_t ne = (size_t)g.n_ev, np = 2 * ne;
    if (ne > s->ev_cap) {
        size_t c = s->ev_cap, p[5] = {0, 0, 0, 0, 0};   // (0: the arrays below are all allocated anew)
        if ((rc = grow(s->d_src, c, ne)) != VLR_OK) return rc;
        s->ev_cap = 0;
        const size_t pairs = 2 * c + 1;   // two pairs per evidence, one more offset
        if ((rc = grow(s->d_xoff, p[0], pairs)) != VLR_OK || (rc = grow(s->d_yoff, p[1], pairs)) != VLR_OK || (rc = grow(s->d_band, p[2], pairs)) != VLR_OK ||
            (rc = grow(s->d_dist, p[3], pairs)) != VLR_OK || (rc = grow(s->d_lnp, p[4], pairs)) != VLR_OK)
            return rc;
        s->ev_cap = c;
    }
    if ((rc = grow(s->d_xb, s->x_cap, (size_t)g.x_bytes + 8)) != VLR_OK) return rc;
    if ((size_t)g.y_bytes + 8 > s->y_cap) {
        size_t c1 = s->y_cap, c2 = s->y_cap;
        if ((rc = grow(s->d_yb, c1, (size_t)g.y_bytes + 8)) != VLR_OK || (rc = grow(s->d_yq, c2, (size_t)g.y_bytes + 8)) != VLR_OK) return rc;
        s->y_cap = std::min(c1, c2);
    }
    double t0 = now_s();
    const int64_t stride = (int64_t)s->rec_cap;
    const unsigned rec_blocks = (unsigned)((g.i1 - g.i0 + kThreads - 1) / kThreads);
    const uint64_t hit0 = s->n_total;
    hipLaunchKernelGGL(indelpileup_fill_kernel, dim3(rec_blocks), dim3(kThreads), 0, st, d_base, d_starts, rec0, s->loci, s->window, (const uint64_t*)s->d_cnt, s->d_off, stride, g, hit0,
                       s->capacity, s->d_hits, s->d_src, s->d_xoff, s->d_yoff, s->d_band);
    const unsigned waves_per_block = kThreads / 64;
    hipLaunchKernelGGL((indelpileup_gather_kernel<IndelWindows, uint32_t>), dim3((unsigned)((ne + waves_per_block - 1) / waves_per_block)), dim3(kThreads), 0, st, d_base,
                       (uint64_t)ne, s->d_hits + hit0, IndelWindows{s->loci, s->ctg.d_ctg, s->d_altb}, s->d_src, s->d_xoff, s->d_yoff, s->d_xb, s->d_yb, s->d_yq);
    if ((rc = sync_stage(st, s->t[4], t0)) != VLR_OK) return rc;
    if ((rc = score_pairs(s->score, np, s->d_xoff, s->d_xb, s->d_yoff, s->d_yb, s->d_yq, s->d_band, s->d_dist, s->d_lnp, st, s->t[5], s->t[6], t0)) != VLR_OK) return rc;
    hipLaunchKernelGGL(indelpileup_collect_kernel, dim3((unsigned)((ne + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, s->d_lnp, s->d_dist, (uint64_t)ne, hit0, s->capacity,
                       s->d_hits);
    if (s->keep_pairs) {
        std::vector<uint32_t> xo(np + 1), yo(np + 1);
        const size_t at = s->p_xlen.size(), ax = s->p_xb.size(), ay = s->p_yb.size();
        s->p_xlen.resize(at + np); s->p_ylen.resize(at + np); s->p_band.resize(at + np);
        s->p_xb.resize(ax + (size_t)g.x_bytes); s->p_yb.resize(ay + (size_t)g.y_bytes); s->p_yq.resize(ay + (size_t)g.y_bytes);
        VLR_HIP_OK(hipMemcpyAsync(xo.data(), s->d_xoff, (np + 1) * 4, hipMemcpyDeviceToHost, st));
        VLR_HIP_OK(hipMemcpyAsync(yo.data(), s->d_yoff, (np + 1) * 4, hipMemcpyDeviceToHost, st));
        VLR_HIP_OK(hipMemcpyAsync(s->p_band.data() + at, s->d_band, np * 4, hipMemcpyDeviceToHost, st));
        if (g.x_bytes) VLR_HIP_OK(hipMemcpyAsync(s->p_xb.data() + ax, s->d_xb, (size_t)g.x_bytes, hipMemcpyDeviceToHost, st));
        if (g.y_bytes) VLR_HIP_OK(hipMemcpyAsync(s->p_yb.data() + ay, s->d_yb, (size_t)g.y_bytes, hipMemcpyDeviceToHost, st));
        if (g.y_bytes) VLR_HIP_OK(hipMemcpyAsync(s->p_yq.data() + ay, s->d_yq, (size_t)g.y_bytes, hipMemcpyDeviceToHost, st));
        VLR_HIP_OK(hipStreamSynchronize(st));
        for (size_t p = 0; p < np; ++p) { s->p_xlen[at + p] = xo[p + 1] - xo[p]; s->p_ylen[at + p] = yo[p + 1] - yo[p]; }
    }
    if ((rc = sync_stage(st, s->t[7], t0)) != VLR_OK) return rc;
    s->n_total += g.n_ev;
    s->x_total += g.x_bytes;
    s->y_total += g.y_bytes;
    return VLR_OK;
}

int run_chunk(vlr_indelpileup* s, vlr_dev_file* df, int64_t n, hipStream_t st) {
    const uint8_t* d_base; const uint64_t* d_starts;
    int rc = vlr_dev_file_split_view(df, &d_base, &d_starts);
    if (rc != VLR_OK || (rc = vlr_bam::reserve_records<uint64_t>(*s, n, K_N, st)) != VLR_OK) return rc;
    const double t0 = now_s();
    const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
    const uint64_t rec0 = s->n_records;
    hipLaunchKernelGGL(indelpileup_count_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->loci, s->window, (uint64_t*)s->d_cnt, (int64_t)s->rec_cap,
                       s->d_counters);
    uint64_t total[K_N] = {0, 0, 0};
    if ((rc = vlr_bam::scan_records<uint64_t>(*s, n, K_N, total, st)) != VLR_OK) return rc;
    s->t[3] += now_s() - t0;
    s->n_records += (uint64_t)n;
    if (total[K_EV] == 0) return VLR_OK;
    if (s->overflow || s->n_total + total[K_EV] > s->capacity) {   // counted, not written: the caller opens again with needed_capacity
        s->overflow = true;
        s->n_total += total[K_EV];
        return VLR_OK;
    }
    if (total[K_X] <= s->pair_byte_limit && total[K_Y] <= s->pair_byte_limit)
        return run_range(s, d_base, d_starts, rec0, Range{0, n, 0, 0, 0, total[K_EV], total[K_X], total[K_Y]}, st);
    // sub-ranges of records whose pair bytes fit the uint32 offsets, cut at the scanned offsets
    std::vector<uint64_t> off((size_t)K_N * (size_t)n);
    for (int k = 0; k < K_N; ++k) VLR_HIP_OK(hipMemcpy(off.data() + (size_t)k * (size_t)n, s->d_off + (size_t)k * s->rec_cap, (size_t)n * 8, hipMemcpyDeviceToHost));
    auto at = [&](int k, int64_t i) { return i < n ? off[(size_t)k * (size_t)n + (size_t)i] : total[k]; };
    for (int64_t i0 = 0; i0 < n;) {
        int64_t i1 = i0 + 1;
        while (i1 < n && at(K_X, i1 + 1) - at(K_X, i0) <= s->pair_byte_limit && at(K_Y, i1 + 1) - at(K_Y, i0) <= s->pair_byte_limit) ++i1;
        const Range g{i0, i1, at(K_EV, i0), at(K_X, i0), at(K_Y, i0), at(K_EV, i1) - at(K_EV, i0), at(K_X, i1) - at(K_X, i0), at(K_Y, i1) - at(K_Y, i0)};
        if (g.x_bytes >= (1ull << 32) || g.y_bytes >= (1ull << 32))
            return bfail(VLR_ERR_UNSUPPORTED, "record %llu: the windows of its evidences take 4 GiB or more", (unsigned long long)(rec0 + (uint64_t)i0));
        if (g.n_ev && (rc = run_range(s, d_base, d_starts, rec0, g, st)) != VLR_OK) return rc;
        i0 = i1;
    }
    return VLR_OK;
}

}  // namespace vlr_ip

extern "C" {

int vlr_indelpileup_open(int device, const char* fasta_path, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int64_t* end, const uint8_t* kind,
                         const uint64_t* alt_offset, const uint8_t* alt_bases, int window, int mode, const double gap[4], const double* hop, int keep_pairs,
                         int64_t hit_capacity, int64_t window_bytes, vlr_indelpileup** out) {
    using namespace vlr_ip;
    if (!out || !fasta_path || !gap || n_loci < 0 || n_loci > 0x7fffffff || hit_capacity < 0 || window_bytes < 0 ||
        (n_loci > 0 && (!ref_id || !start || !end || !kind || !alt_offset || !alt_bases)))
        return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_open: bad argument");
    *out = nullptr;
    ScoreParams sp;
    int rc = check_score_params("vlr_indelpileup_open", window, mode, gap, hop, sp);
    if (rc != VLR_OK) return rc;
    int64_t max_len = 0;
    for (int64_t k = 0; k < n_loci; ++k) {
        if (kind[k] > VLR_INDELPILEUP_REPLACEMENT || ref_id[k] < 0 || start[k] < 0 || end[k] <= start[k] || alt_offset[k + 1] < alt_offset[k] || (k == 0 && alt_offset[0] != 0))
            return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_open: locus %lld: kind %d, [%lld, %lld), or its alt window's offsets", (long long)k, (int)kind[k],
                         (long long)start[k], (long long)end[k]);
        if (k > 0 && (ref_id[k] < ref_id[k - 1] || (ref_id[k] == ref_id[k - 1] && start[k] < start[k - 1])))
            return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_open: loci are not sorted by (ref_id, start) at %lld", (long long)k);
        max_len = std::max(max_len, end[k] - start[k]);
    }
    if ((rc = vlr_bam::use_device(device)) != VLR_OK) return rc;
    vlr_indelpileup* s = new vlr_indelpileup();
    s->device = device;
    s->window = window; s->score = sp; s->keep_pairs = keep_pairs != 0;
    s->n_loci = n_loci;
    s->capacity = (uint64_t)hit_capacity;
    // tuning / test knob: the pair bytes a record sub-range may hold (the uint32 offsets need at most 2^31)
    if (const char* v = getenv("VLR_INDELPILEUP_PAIR_BYTES")) {
        const unsigned long long x = strtoull(v, nullptr, 10);
        if (x >= 1 && x <= kPairByteLimit) s->pair_byte_limit = x;
    }
    s->ctg.fasta = fasta_path;
    s->h_ref_id.assign(ref_id, ref_id + n_loci);
    const uint64_t zero = 0;
    rc = vlr_bam::read_fai(s->ctg.fasta, s->ctg.fai);
    auto step = [&](int r) { if (rc == VLR_OK) rc = r; };
    step(upload(s->d_ref_id, ref_id, (size_t)n_loci));
    step(upload(s->d_start, start, (size_t)n_loci));
    step(upload(s->d_end, end, (size_t)n_loci));
    step(n_loci ? upload(s->d_alt_off, alt_offset, (size_t)n_loci + 1) : upload(s->d_alt_off, &zero, 1));
    step(upload(s->d_altb, alt_bases, n_loci ? (size_t)alt_offset[n_loci] : 0));
    step(vlr_bam::open_session(*s, device, window_bytes, K_N));
    step(vlr_bam::guarded(s->d_hits, (size_t)s->capacity));
    if (rc != VLR_OK) { vlr_indelpileup_close(s); return rc; }
    s->loci = Loci{n_loci, s->d_ref_id, s->d_start, s->d_end, s->d_alt_off, max_len, 0, nullptr};
    *out = s;
    return VLR_OK;
}

int vlr_indelpileup_add_bam(vlr_indelpileup* s, const char* bam_path) {
    if (!s) return vlr_bam::bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_add_bam: null");
    return vlr_bam::add_bam(*s, bam_path, "vlr_indelpileup_add_bam", {&s->t[0], &s->t[1], &s->t[2], &s->t[10], &s->t[9]},
                            [s, bam_path](const std::vector<std::string>& names) { return vlr_ip::on_header(s, names, bam_path); },
                            [s](vlr_dev_file* df, int64_t n, hipStream_t st) { return vlr_ip::run_chunk(s, df, n, st); });
}

int vlr_indelpileup_result(vlr_indelpileup* s, vlr_indelpileup_counts* r) {
    using namespace vlr_ip;
    if (!s || !r) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_result: null");
    VLR_HIP_OK(hipSetDevice(s->device));
    if (!s->collected) {
        const double t0 = now_s();
        bool intact = true;
        int rc = vlr_bam::read_counters(*s);
        if (rc != VLR_OK || (rc = vlr_bam::guard_intact(s->d_hits, (size_t)s->capacity, &intact)) != VLR_OK) return rc;
        if (!intact) s->status |= VLR_INDELPILEUP_GUARD_DAMAGED;
        if (vlr_bam::bad_record_seen(*s)) s->status |= VLR_INDELPILEUP_BAD_RECORD;
        if (s->overflow) s->status |= VLR_INDELPILEUP_OVERFLOW;
        else if (s->n_total) {
            std::vector<vlr_indelpileup_hit> raw((size_t)s->n_total);
            VLR_HIP_OK(hipMemcpy(raw.data(), s->d_hits, raw.size() * sizeof(vlr_indelpileup_hit), hipMemcpyDeviceToHost));
            vlr_bam::locus_major(raw, s->n_loci, s->hits, &s->perm);
        }
        s->t[8] += now_s() - t0;
        s->collected = true;
    }
    r->n_hits = (int64_t)s->hits.size();
    r->n_records = (int64_t)s->n_records;
    r->n_rejected = (int64_t)s->counters[C_REJECTED];
    r->n_pairs = 2 * r->n_hits;
    r->x_bytes = s->overflow ? 0 : (int64_t)s->x_total;
    r->y_bytes = s->overflow ? 0 : (int64_t)s->y_total;
    r->status = s->status;
    r->needed_capacity = (int64_t)s->n_total;
    r->first_bad_record = vlr_bam::first_bad_record(*s);
    for (int k = 0; k < 12; ++k) r->seconds[k] = s->t[k];
    return VLR_OK;
}

int vlr_indelpileup_read(vlr_indelpileup* s, vlr_indelpileup_hit* hits, int64_t n) {
    using namespace vlr_ip;
    if (!s || !s->collected) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_read: call vlr_indelpileup_result first");
    if (n != (int64_t)s->hits.size() || (n > 0 && !hits)) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_read: size differs from vlr_indelpileup_result");
    if (n) memcpy(hits, s->hits.data(), (size_t)n * sizeof(vlr_indelpileup_hit));
    return VLR_OK;
}

int vlr_indelpileup_read_pairs(vlr_indelpileup* s, uint32_t* x_offset, uint8_t* x_bases, int64_t x_bytes, uint32_t* y_offset, uint8_t* y_bases, uint8_t* y_quals,
                               int64_t y_bytes, int32_t* band, int64_t n_pairs) {
    using namespace vlr_ip;
    if (!s || !s->collected) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_read_pairs: call vlr_indelpileup_result first");
    if (!s->keep_pairs) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_read_pairs: the session was opened without keep_pairs");
    if (s->overflow) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_read_pairs: the hit buffer overflowed");
    const size_t np = 2 * s->hits.size();
    if (n_pairs != (int64_t)np || x_bytes != (int64_t)s->x_total || y_bytes != (int64_t)s->y_total || !x_offset || !y_offset || (np && !band) ||
        (x_bytes && !x_bases) || (y_bytes && (!y_bases || !y_quals)))
        return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_read_pairs: sizes differ from vlr_indelpileup_result");
    if (s->x_total >= (1ull << 32) || s->y_total >= (1ull << 32)) return bfail(VLR_ERR_UNSUPPORTED, "vlr_indelpileup_read_pairs: the pair bytes do not fit 32-bit offsets");
    if (s->p_xlen.size() != 2 * (size_t)s->n_total) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_read_pairs: kept pairs and hits differ");
    // record-major starts of every kept pair, then the pairs in hit order
    std::vector<uint64_t> xs(s->p_xlen.size() + 1, 0), ys(s->p_ylen.size() + 1, 0);
    for (size_t p = 0; p < s->p_xlen.size(); ++p) { xs[p + 1] = xs[p] + s->p_xlen[p]; ys[p + 1] = ys[p] + s->p_ylen[p]; }
    uint64_t x = 0, y = 0;
    for (size_t k = 0; k < s->hits.size(); ++k)
        for (size_t j = 0; j < 2; ++j) {
            const size_t from = 2 * (size_t)s->perm[k] + j, to = 2 * k + j;
            const uint32_t xl = s->p_xlen[from], yl = s->p_ylen[from];
            if (x + xl > (uint64_t)x_bytes || y + yl > (uint64_t)y_bytes) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_indelpileup_read_pairs: kept pairs and sizes differ");
            x_offset[to] = (uint32_t)x; y_offset[to] = (uint32_t)y;
            band[to] = s->p_band[from];
            if (xl) memcpy(x_bases + x, s->p_xb.data() + xs[from], xl);
            if (yl) { memcpy(y_bases + y, s->p_yb.data() + ys[from], yl); memcpy(y_quals + y, s->p_yq.data() + ys[from], yl); }
            x += xl; y += yl;
        }
    x_offset[np] = (uint32_t)x; y_offset[np] = (uint32_t)y;
    return VLR_OK;
}

void vlr_indelpileup_close(vlr_indelpileup* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    vlr_bam::close_session(*s);
    void* p[] = {s->d_ref_id, s->d_start, s->d_end, s->d_alt_off, s->d_altb, s->d_hits,
                 s->d_src, s->d_xoff, s->d_yoff, s->d_band, s->d_dist, s->d_lnp, s->d_xb, s->d_yb, s->d_yq};
    for (void* q : p) if (q) (void)hipFree(q);
    s->ctg.free();
    delete s;
}

}  // extern "C"
