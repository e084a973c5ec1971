// vlr_basepileup.hip — SNV / MNV allele supports from BAM records for gfx950 (vlr_basepileup_*, include/vlr.h): the scoring of
// vlr_basepileup.h over every record of a BAM file streamed through the device reader (vlr_bamstream.h: BGZF members inflated on the
// device, records split there), and the host driver of the session.
//
// Work mapping: one record per thread.  A short read encloses a handful of loci and its CIGAR has a few operations: a wave per record
// would leave most lanes idle, and the records of a chunk are independent.  Per chunk of split records three kernels run:
//   basepileup_count_kernel  thread i decodes and validates record i (vlr_bp::decode), finds its first locus by binary search, walks the
//                            loci its alignment encloses and scores each: cnt[i] = hits of the record (nothing is written); rejected,
//                            bad and to-be-realigned records go to integer counters (sums and a minimum: order-independent)
//   basepileup_scan_kernel   one workgroup: exclusive prefix sum of cnt -> off[i], the chunk's total
//   basepileup_fill_kernel   thread i scores record i again and writes its hits at hits[base + off[i] ...), base = hits of the chunks in
//                            front; a hit at or behind the capacity is not written
// so a hit's place is a function of the record order alone: no atomics decide a position, and how the file was cut into feeds and
// chunks (window_bytes) cannot change the array.  The hits leave the device record-major; vlr_basepileup_result puts them locus-major
// with a stable counting sort on the host (record order within a locus kept) — a permutation of 48-byte items, see
// profiles/basepileup.md for its share.
//
// Bounds: see vlr_basepileup.h — every byte of a record is read only after vlr_bp::decode checked its lengths against the record's end
// d_starts[i + 1]; the fill pass writes hits[k] only for k < capacity, and guard words behind the buffer are checked at the end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vlr.h"
#include "vlr_gpuio.h"
#include "vlr_bamstream.h"
#include "vlr_basepileup.h"

static_assert(sizeof(vlr_basepileup_hit) == 48, "hit layout");

namespace vlr_bp {

enum Counter { C_REJECTED, C_BAD, C_NEEDS_REALIGN, C_FIRST_BAD, C_N };
constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr size_t kGuardHits = 4;           // guard words behind the hit buffer: kGuardHits * sizeof(hit) bytes of kGuardByte
constexpr int kGuardByte = 0xA5;

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

// one workgroup: thread t sums the slice [t * per, (t + 1) * per) of cnt, the sums are scanned in LDS, then the slice's offsets written
__global__ __launch_bounds__(kScanThreads) void basepileup_scan_kernel(const uint32_t* __restrict__ cnt, int64_t n, uint64_t* __restrict__ off, uint64_t* __restrict__ total) {
    __shared__ uint64_t s[2][kScanThreads];
    const int t = (int)threadIdx.x;
    const int64_t per = (n + kScanThreads - 1) / kScanThreads;
    const int64_t lo = std::min<int64_t>((int64_t)t * per, n), hi = std::min<int64_t>(lo + per, n);
    uint64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += cnt[i];
    s[0][t] = sum;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kScanThreads; d <<= 1) {
        s[cur ^ 1][t] = s[cur][t] + (t >= d ? s[cur][t - d] : 0ull);
        cur ^= 1;
        __syncthreads();
    }
    uint64_t run = s[cur][t] - sum;   // exclusive
    for (int64_t i = lo; i < hi; ++i) { off[i] = run; run += cnt[i]; }
    if (t == kScanThreads - 1) *total = s[cur][t];
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

struct vlr_basepileup {
    int device = 0;
    int realign = 0;
    int64_t n_loci = 0;
    uint64_t capacity = 0;
    size_t window = (size_t)64 << 20;
    // device state
    int32_t* d_ref_id = nullptr; int64_t* d_start = nullptr; int32_t* d_len = nullptr; uint8_t* d_kind = nullptr; uint64_t* d_base_off = nullptr;
    uint8_t *d_refb = nullptr, *d_altb = nullptr;
    double* d_tables = nullptr;   // call, miscall, linear
    vlr_basepileup_hit* d_hits = nullptr;
    uint32_t* d_cnt = nullptr; uint64_t* d_off = nullptr; size_t rec_cap = 0;
    unsigned long long* d_counters = nullptr; uint64_t* d_total = nullptr;
    vlr_bp::Tables tables{};
    vlr_bp::Loci loci{};
    // host state
    uint64_t n_total = 0;        // hits the input produced so far
    uint64_t n_records = 0;      // records of the files given so far
    uint64_t status = 0;
    int64_t trunc_record = -1;   // a file ended inside this record
    std::vector<vlr_basepileup_hit> hits;
    bool collected = false;
    uint64_t counters[vlr_bp::C_N] = {0, 0, 0, ~0ull};
    double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace vlr_bp {
using vlr_bam::bfail;
using vlr_bam::now_s;

#define BP_HIP_OK(call)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) return bfail(VLR_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

template <class T> int upload(T*& d, const T* h, size_t n) {
    BP_HIP_OK(hipMalloc((void**)&d, std::max<size_t>(n, 1) * sizeof(T)));
    if (n) BP_HIP_OK(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
    return VLR_OK;
}

int run_chunk(vlr_basepileup* s, vlr_dev_file* df, int64_t n, hipStream_t st) {
    const uint8_t* d_base; const uint64_t* d_starts;
    int rc = vlr_dev_file_split_view(df, &d_base, &d_starts);
    if (rc != VLR_OK) return rc;
    if ((size_t)n > s->rec_cap) {
        BP_HIP_OK(hipStreamSynchronize(st));
        if (s->d_cnt) (void)hipFree(s->d_cnt);
        if (s->d_off) (void)hipFree(s->d_off);
        s->d_cnt = nullptr; s->d_off = nullptr; s->rec_cap = 0;
        const size_t cap = (size_t)n + (size_t)n / 4 + 1024;
        BP_HIP_OK(hipMalloc((void**)&s->d_cnt, cap * 4));
        BP_HIP_OK(hipMalloc((void**)&s->d_off, cap * 8));
        s->rec_cap = cap;
    }
    const double t0 = now_s();
    const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
    const uint64_t rec0 = s->n_records;
    hipLaunchKernelGGL(basepileup_count_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->tables, s->loci, s->realign, s->d_cnt, s->d_counters);
    hipLaunchKernelGGL(basepileup_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, s->d_cnt, n, s->d_off, s->d_total);
    uint64_t total = 0;
    BP_HIP_OK(hipMemcpyAsync(&total, s->d_total, 8, hipMemcpyDeviceToHost, st));
    BP_HIP_OK(hipStreamSynchronize(st));
    BP_HIP_OK(hipGetLastError());
    if (total && s->n_total < s->capacity) {
        hipLaunchKernelGGL(basepileup_fill_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->tables, s->loci, s->realign, s->d_cnt, s->d_off,
                           s->n_total, s->capacity, s->d_hits);
        BP_HIP_OK(hipStreamSynchronize(st));
        BP_HIP_OK(hipGetLastError());
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
    std::vector<uint64_t> base_off((size_t)n_loci + 1, 0);
    for (int64_t k = 0; k < n_loci; ++k) {
        const bool snv = kind[k] == VLR_BASEPILEUP_SNV;
        if ((!snv && kind[k] != VLR_BASEPILEUP_MNV) || ref_id[k] < 0 || start[k] < 0 || (snv ? len[k] != 1 : (len[k] < 2 || len[k] > VLR_BASEPILEUP_MAX_LEN)))
            return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_basepileup_open: locus %lld: kind %d with %d bases (an SNV has 1, an MNV 2 .. %d)", (long long)k, (int)kind[k],
                         (int)len[k], VLR_BASEPILEUP_MAX_LEN);
        if (k > 0 && (ref_id[k] < ref_id[k - 1] || (ref_id[k] == ref_id[k - 1] && start[k] < start[k - 1])))
            return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_basepileup_open: loci are not sorted by (ref_id, start) at %lld", (long long)k);
        base_off[(size_t)k + 1] = base_off[(size_t)k] + (uint64_t)len[k];
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || ndev <= device) return bfail(VLR_ERR_NO_DEVICE, "no HIP device %d (the engine has no CPU path)", device);
    BP_HIP_OK(hipSetDevice(device));
    vlr_basepileup* s = new vlr_basepileup();
    s->device = device;
    s->realign = realign_indel_reads ? 1 : 0;
    s->n_loci = n_loci;
    s->capacity = (uint64_t)hit_capacity;
    if (window_bytes > 0) s->window = (size_t)window_bytes;
    std::vector<double> tab(3 * 256);
    fill_tables(tab.data(), tab.data() + 256, tab.data() + 512);
    const size_t nb = (size_t)base_off[(size_t)n_loci];
    const size_t hit_bytes = ((size_t)s->capacity + kGuardHits) * sizeof(vlr_basepileup_hit);
    int rc = VLR_OK;
    auto step = [&](int r) { if (rc == VLR_OK) rc = r; };
    step(upload(s->d_ref_id, ref_id, (size_t)n_loci));
    step(upload(s->d_start, start, (size_t)n_loci));
    step(upload(s->d_len, len, (size_t)n_loci));
    step(upload(s->d_kind, kind, (size_t)n_loci));
    step(upload(s->d_base_off, base_off.data(), (size_t)n_loci + 1));
    step(upload(s->d_refb, ref_bases, nb));
    step(upload(s->d_altb, alt_bases, nb));
    step(upload(s->d_tables, tab.data(), tab.size()));
    step(upload(s->d_counters, (const unsigned long long*)s->counters, (size_t)C_N));
    auto hip = [&](hipError_t e, const char* what) { if (rc == VLR_OK && e != hipSuccess) rc = bfail(e == hipErrorOutOfMemory ? VLR_ERR_OUT_OF_MEMORY : VLR_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); };
    if (rc == VLR_OK) hip(hipMalloc((void**)&s->d_total, 8), "hipMalloc");
    if (rc == VLR_OK) hip(hipMalloc((void**)&s->d_hits, hit_bytes), "hipMalloc of the hit buffer");
    if (rc == VLR_OK) hip(hipMemset((void*)(s->d_hits + s->capacity), kGuardByte, kGuardHits * sizeof(vlr_basepileup_hit)), "hipMemset");
    if (rc != VLR_OK) { vlr_basepileup_close(s); return rc; }
    s->tables = Tables{s->d_tables, s->d_tables + 256, s->d_tables + 512, ln_confusion(), ln_any()};
    s->loci = Loci{n_loci, s->d_ref_id, s->d_start, s->d_len, s->d_kind, s->d_base_off, s->d_refb, s->d_altb};
    *out = s;
    return VLR_OK;
}

int vlr_basepileup_add_bam(vlr_basepileup* s, const char* bam_path) {
    using namespace vlr_bp;
    if (!s || !bam_path) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_basepileup_add_bam: null");
    if (s->collected) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_basepileup_add_bam: the result was already read");
    if (s->trunc_record >= 0) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_basepileup_add_bam: the file before ended inside a record");
    if (hipSetDevice(s->device) != hipSuccess) return bfail(VLR_ERR_HIP, "hipSetDevice(%d) failed", s->device);
    vlr_bam::BamStream b;
    b.device = s->device;
    b.window = &s->window;
    b.t_read = &s->t[0]; b.t_feed = &s->t[1]; b.t_split = &s->t[2]; b.t_inflate = &s->t[6]; b.t_total = &s->t[5];
    b.on_chunk = [s](vlr_dev_file* df, int64_t n, uint64_t, const std::vector<std::string>&, const char*, void* st) { return run_chunk(s, df, n, (hipStream_t)st); };
    // a file that ends inside a record: malformed input, reported in the status word; the records in front of it are scored
    b.on_truncated = [s](uint64_t) { s->trunc_record = (int64_t)s->n_records; return (int)VLR_OK; };
    return vlr_bam::stream_bam(b, bam_path);
}

int vlr_basepileup_result(vlr_basepileup* s, vlr_basepileup_counts* r) {
    using namespace vlr_bp;
    if (!s || !r) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_basepileup_result: null");
    BP_HIP_OK(hipSetDevice(s->device));
    if (!s->collected) {
        const double t0 = now_s();
        BP_HIP_OK(hipMemcpy(s->counters, s->d_counters, sizeof s->counters, hipMemcpyDeviceToHost));
        uint8_t guard[kGuardHits * sizeof(vlr_basepileup_hit)];
        BP_HIP_OK(hipMemcpy(guard, (const void*)(s->d_hits + s->capacity), sizeof guard, hipMemcpyDeviceToHost));
        for (uint8_t g : guard) if (g != (uint8_t)kGuardByte) s->status |= VLR_BASEPILEUP_GUARD_DAMAGED;
        if (s->counters[C_BAD] || s->trunc_record >= 0) s->status |= VLR_BASEPILEUP_BAD_RECORD;
        if (s->n_total > s->capacity) s->status |= VLR_BASEPILEUP_OVERFLOW;
        else if (s->n_total) {
            // record-major on the device -> locus-major, record order kept within a locus: a stable counting sort
            std::vector<vlr_basepileup_hit> raw((size_t)s->n_total);
            BP_HIP_OK(hipMemcpy(raw.data(), s->d_hits, raw.size() * sizeof(vlr_basepileup_hit), hipMemcpyDeviceToHost));
            std::vector<uint64_t> first((size_t)s->n_loci + 1, 0);
            for (const auto& h : raw) if ((int64_t)h.locus < s->n_loci) ++first[(size_t)h.locus + 1];
            for (size_t k = 0; k < (size_t)s->n_loci; ++k) first[k + 1] += first[k];
            s->hits.resize(raw.size());
            for (const auto& h : raw) if ((int64_t)h.locus < s->n_loci) s->hits[(size_t)first[h.locus]++] = h;
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
    r->first_bad_record = s->counters[C_BAD] ? (int64_t)s->counters[C_FIRST_BAD] : -1;
    if (s->trunc_record >= 0 && (r->first_bad_record < 0 || s->trunc_record < r->first_bad_record)) r->first_bad_record = s->trunc_record;
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
    void* p[] = {s->d_ref_id, s->d_start, s->d_len, s->d_kind, s->d_base_off, s->d_refb, s->d_altb, s->d_tables, s->d_hits, s->d_cnt, s->d_off, s->d_counters, s->d_total};
    for (void* q : p) if (q) (void)hipFree(q);
    delete s;
}

}  // extern "C"
