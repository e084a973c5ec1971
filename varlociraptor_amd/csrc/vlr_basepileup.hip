// vlr_basepileup.hip — SNV / MNV allele supports from BAM records for gfx950 (vlr_basepileup_*, include/vlr.h): the scoring of
// vlr_basepileup.h over every record of a BAM file streamed through the device reader (vlr_bamstream.h: BGZF members inflated on the
// device, records split there), and the host driver of the session.
//
// Work mapping: one record per thread.  A short read encloses a handful of loci and its CIGAR has a few operations: a wave per record
// would leave most lanes idle, and the records of a chunk are independent.  Per chunk of split records three kernels run:
//   basepileup_count_kernel  thread i decodes and validates record i (vlr_bp::decode), finds its first locus by binary search, walks the
//                            loci its alignment encloses and scores each: cnt[i] = hits of the record (nothing is written); rejected,
//                            bad and to-be-realigned records go to integer counters (sums and a minimum: order-independent)
//   vlr_bam::scan_kernel     one workgroup: exclusive prefix sum of cnt -> off[i], the chunk's total (vlr_bamsession.h, u32 counts)
//   basepileup_fill_kernel   thread i scores record i again and writes its hits at hits[base + off[i] ...), base = hits of the chunks in
//                            front; a hit at or behind the capacity is not written
// so a hit's place is a function of the record order alone: no atomics decide a position, and how the file was cut into feeds and
// chunks (window_bytes) cannot change the array.  The hits leave the device record-major; vlr_basepileup_result puts them locus-major
// with a stable counting sort on the host (vlr_bam::locus_major: record order within a locus kept) — a permutation of 48-byte items,
// see profiles/basepileup.md for its share.  The session's common state, the wiring of a file into the device reader and the buffer
// helpers are vlr_bamsession.h's.
//
// Bounds: see vlr_basepileup.h — every byte of a record is read only after vlr_bp::decode checked its lengths against the record's end
// d_starts[i + 1]; the fill pass writes hits[k] only for k < capacity, and guard bytes behind the buffer are checked at the end.
#include <cstring>

#include "vlr_bamsession.h"

static_assert(sizeof(vlr_basepileup_hit) == 48, "hit layout");

namespace vlr_bp {

using vlr_bam::C_BAD;
using vlr_bam::C_FIRST_BAD;
using vlr_bam::C_REJECTED;
constexpr int C_NEEDS_REALIGN = vlr_bam::C_OWN;
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void basepileup_count_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                                    Tables t, Loci L, int realign, uint32_t* __restrict__ cnt,
                                                                    unsigned long long* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = starts[i], end = starts[i + 1];
    const RecResult r = record_hits(t, L, base + o, end - o, rec0 + (uint64_t)i, realign != 0, nullptr, 0);
    cnt[i] = r.n_hits;
    if (r.cls == REC_REJECTED) atomicAdd(&counters[C_REJECTED], 1ull);
    if (r.cls == REC_BAD) { atomicAdd(&counters[C_BAD], 1ull); atomicMin(&counters[C_FIRST_BAD], (unsigned long long)(rec0 + (uint64_t)i)); }
    if (r.n_needs_realign) atomicAdd(&counters[C_NEEDS_REALIGN], (unsigned long long)r.n_needs_realign);
}

__global__ __launch_bounds__(kThreads) void basepileup_fill_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                                   Tables t, Loci L, int realign, const uint32_t* __restrict__ cnt,
                                                                   const uint64_t* __restrict__ off, uint64_t hit0, uint64_t capacity,
                                                                   vlr_basepileup_hit* __restrict__ hits) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || cnt[i] == 0) return;
    const uint64_t first = hit0 + off[i];
    if (first >= capacity) return;
    const uint64_t o = starts[i], end = starts[i + 1];
    (void)record_hits(t, L, base + o, end - o, rec0 + (uint64_t)i, realign != 0, hits + first, capacity - first);
}

}  // namespace vlr_bp

struct vlr_basepileup : vlr_bam::Session {
    int realign = 0;
    int64_t n_loci = 0;
    uint64_t capacity = 0;
    vlr_bp::DeviceLoci dl;
    vlr_basepileup_hit* d_hits = nullptr;
    uint64_t n_total = 0;        // hits the input produced so far
    std::vector<vlr_basepileup_hit> hits;
    double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace vlr_bp {
using vlr_bam::bfail;
using vlr_bam::now_s;

int run_chunk(vlr_basepileup* s, vlr_dev_file* df, int64_t n, hipStream_t st) {
    const uint8_t* d_base; const uint64_t* d_starts;
    int rc = vlr_dev_file_split_view(df, &d_base, &d_starts);
    if (rc != VLR_OK || (rc = vlr_bam::reserve_records<uint32_t>(*s, n, 1, st)) != VLR_OK) return rc;
    const double t0 = now_s();
    const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
    const uint64_t rec0 = s->n_records;
    uint32_t* d_cnt = (uint32_t*)s->d_cnt;
    hipLaunchKernelGGL(basepileup_count_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->realign, d_cnt, s->d_counters);
    uint64_t total = 0;
    if ((rc = vlr_bam::scan_records<uint32_t>(*s, n, 1, &total, st)) != VLR_OK) return rc;
    if (total && s->n_total < s->capacity) {
        hipLaunchKernelGGL(basepileup_fill_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->realign, d_cnt, s->d_off,
                           s->n_total, s->capacity, s->d_hits);
        VLR_HIP_OK(hipStreamSynchronize(st));
        VLR_HIP_OK(hipGetLastError());
    }
    s->n_total += total;
    s->n_records += (uint64_t)n;
    s->t[3] += now_s() - t0;
    return VLR_OK;
}

}  // namespace vlr_bp

extern "C" {

int vlr_basepileup_tables(double call[256], double miscall[256]) {
    if (!call || !miscall) return vlr_bam::bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_basepileup_tables: null");
    vlr_bp::fill_tables(call, miscall, nullptr);
    return VLR_OK;
}

int vlr_basepileup_open(int device, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int32_t* len, const uint8_t* kind,
                        const uint8_t* ref_bases, const uint8_t* alt_bases, int realign_indel_reads, int64_t hit_capacity, int64_t window_bytes,
                        vlr_basepileup** out) {
    using namespace vlr_bp;
    if (!out || n_loci < 0 || n_loci > 0x7fffffff || hit_capacity < 0 || window_bytes < 0 ||
        (n_loci > 0 && (!ref_id || !start || !len || !kind || !ref_bases || !alt_bases)))
        return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_basepileup_open: bad argument");
    *out = nullptr;
    std::vector<uint64_t> base_off;
    int rc = check_snv_mnv_loci("vlr_basepileup_open", n_loci, ref_id, start, len, kind, base_off);
    if (rc != VLR_OK || (rc = vlr_bam::use_device(device)) != VLR_OK) return rc;
    vlr_basepileup* s = new vlr_basepileup();
    s->realign = realign_indel_reads ? 1 : 0;
    s->n_loci = n_loci;
    s->capacity = (uint64_t)hit_capacity;
    if ((rc = vlr_bam::open_session(*s, device, window_bytes, 1)) != VLR_OK || (rc = s->dl.upload(n_loci, ref_id, start, len, kind, base_off, ref_bases, alt_bases)) != VLR_OK ||
        (rc = vlr_bam::guarded(s->d_hits, (size_t)s->capacity)) != VLR_OK) {
        vlr_basepileup_close(s);
        return rc;
    }
    *out = s;
    return VLR_OK;
}

int vlr_basepileup_add_bam(vlr_basepileup* s, const char* bam_path) {
    if (!s) return vlr_bam::bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_basepileup_add_bam: null");
    return vlr_bam::add_bam(*s, bam_path, "vlr_basepileup_add_bam", {&s->t[0], &s->t[1], &s->t[2], &s->t[6], &s->t[5]}, nullptr,
                            [s](vlr_dev_file* df, int64_t n, hipStream_t st) { return vlr_bp::run_chunk(s, df, n, st); });
}

int vlr_basepileup_result(vlr_basepileup* s, vlr_basepileup_counts* r) {
    using namespace vlr_bp;
    if (!s || !r) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_basepileup_result: null");
    VLR_HIP_OK(hipSetDevice(s->device));
    if (!s->collected) {
        const double t0 = now_s();
        bool intact = true;
        int rc = vlr_bam::read_counters(*s);
        if (rc != VLR_OK || (rc = vlr_bam::guard_intact(s->d_hits, (size_t)s->capacity, &intact)) != VLR_OK) return rc;
        if (!intact) s->status |= VLR_BASEPILEUP_GUARD_DAMAGED;
        if (vlr_bam::bad_record_seen(*s)) s->status |= VLR_BASEPILEUP_BAD_RECORD;
        if (s->n_total > s->capacity) s->status |= VLR_BASEPILEUP_OVERFLOW;
        else if (s->n_total) {
            std::vector<vlr_basepileup_hit> raw((size_t)s->n_total);
            VLR_HIP_OK(hipMemcpy(raw.data(), s->d_hits, raw.size() * sizeof(vlr_basepileup_hit), hipMemcpyDeviceToHost));
            vlr_bam::locus_major(raw, s->n_loci, s->hits, nullptr);
        }
        s->t[4] += now_s() - t0;
        s->collected = true;
    }
    r->n_hits = (int64_t)s->hits.size();
    r->n_records = (int64_t)s->n_records;
    r->n_rejected = (int64_t)s->counters[C_REJECTED];
    r->n_needs_realign = (int64_t)s->counters[C_NEEDS_REALIGN];
    r->status = s->status;
    r->needed_capacity = (int64_t)s->n_total;
    r->first_bad_record = vlr_bam::first_bad_record(*s);
    for (int k = 0; k < 8; ++k) r->seconds[k] = s->t[k];
    return VLR_OK;
}

int vlr_basepileup_read(vlr_basepileup* s, vlr_basepileup_hit* hits, int64_t n) {
    using namespace vlr_bp;
    if (!s || !s->collected) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_basepileup_read: call vlr_basepileup_result first");
    if (n != (int64_t)s->hits.size() || (n > 0 && !hits)) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_basepileup_read: size differs from vlr_basepileup_result");
    if (n) memcpy(hits, s->hits.data(), (size_t)n * sizeof(vlr_basepileup_hit));
    return VLR_OK;
}

void vlr_basepileup_close(vlr_basepileup* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    vlr_bam::close_session(*s);
    s->dl.free();
    if (s->d_hits) (void)hipFree(s->d_hits);
    delete s;
}

}  // extern "C"
