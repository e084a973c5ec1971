// vlr_bamsession.h — what the device sessions over BAM records have in common (vlr_basepileup.hip, vlr_indelpileup.hip,
// vlr_fragpileup.hip; the error macro, the buffer helpers and the contig loader also serve vlr_bamstats.hip): the error macro, the
// device buffer helpers and the owner of a session's or a pass's buffers, the one-workgroup prefix sum, the state every session keeps, the wiring of a file into the device reader
// (vlr_bamstream.h), the bad-record rule, the host's locus-major sort and the SNV / MNV loci on the device.  Structs and free
// functions; every session keeps its own kernels, the body of its run_chunk and its open / result / read.  Internal to those .hip files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "../../include/vlr.h"
#include "vlr_gpuio.h"
#include "vlr_bamstream.h"
#include "vlr_basepileup.h"

// a failed HIP call ends the function with the engine's code for it: out of device memory has its own
#define VLR_HIP_OK(call)                                                                                                                                     \
    do {                                                                                                                                                     \
        hipError_t e_ = (call);                                                                                                                              \
        if (e_ != hipSuccess) return vlr_bam::bfail(e_ == hipErrorOutOfMemory ? VLR_ERR_OUT_OF_MEMORY : VLR_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

namespace vlr_bam {

constexpr int kScanThreads = 1024;
constexpr size_t kGuardBytes = 256;   // behind every capacity-bounded buffer: kGuardBytes of kGuardByte, looked at when the session ends
constexpr int kGuardByte = 0xA5;

template <class T> int upload(T*& d, const T* h, size_t n) {
    VLR_HIP_OK(hipMalloc((void**)&d, std::max<size_t>(n, 1) * sizeof(T)));
    if (n) VLR_HIP_OK(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
    return VLR_OK;
}
template <class T> int zeros(T*& d, size_t n) {
    VLR_HIP_OK(hipMalloc((void**)&d, std::max<size_t>(n, 1) * sizeof(T)));
    VLR_HIP_OK(hipMemset((void*)d, 0, std::max<size_t>(n, 1) * sizeof(T)));
    return VLR_OK;
}
// device buffers only grow (the stream is idle when this runs: the callers synchronise first)
template <class T> int grow(T*& p, size_t& cap, size_t need) {
    if (need <= cap) return VLR_OK;
    if (p) (void)hipFree((void*)p);
    p = nullptr; cap = 0;
    const size_t ncap = need + need / 4 + 1024;
    VLR_HIP_OK(hipMalloc((void**)&p, ncap * sizeof(T)));
    cap = ncap;
    return VLR_OK;
}
// a buffer of n items with guard bytes behind it
template <class T> int guarded(T*& d, size_t n) {
    VLR_HIP_OK(hipMalloc((void**)&d, n * sizeof(T) + kGuardBytes));
    VLR_HIP_OK(hipMemset((void*)((uint8_t*)d + n * sizeof(T)), kGuardByte, kGuardBytes));
    return VLR_OK;
}
template <class T> int guard_intact(const T* d, size_t n, bool* ok) {
    uint8_t g[kGuardBytes];
    VLR_HIP_OK(hipMemcpy(g, (const uint8_t*)d + n * sizeof(T), kGuardBytes, hipMemcpyDeviceToHost));
    for (uint8_t b : g) if (b != (uint8_t)kGuardByte) *ok = false;
    return VLR_OK;
}

// The device buffers of a session, or the scratch of one pass: handed out here and remembered here, the guarded ones with the bytes in
// front of their guard, so that the check of the guards and the release name no buffer and no size again.
struct Buffers {
    struct Buf { void* p; size_t bytes; bool guard; };
    std::vector<Buf> bufs;
    template <class T> int upload(T*& d, const T* h, size_t n) { const int rc = vlr_bam::upload(d, h, n); keep(d, 0, false); return rc; }
    template <class T> int zeros(T*& d, size_t n) { const int rc = vlr_bam::zeros(d, n); keep(d, 0, false); return rc; }
    template <class T> int guarded(T*& d, size_t n) { const int rc = vlr_bam::guarded(d, n); keep(d, n * sizeof(T), true); return rc; }
    // *ok = false when the guard bytes behind any guarded buffer changed; the first HIP error ends the check
    int guards_intact(bool* ok) const {
        for (const Buf& b : bufs) {
            const int rc = b.guard ? guard_intact((const uint8_t*)b.p, b.bytes, ok) : VLR_OK;
            if (rc != VLR_OK) return rc;
        }
        return VLR_OK;
    }
    void free() {
        for (const Buf& b : bufs) (void)hipFree(b.p);
        bufs.clear();
    }
    void keep(void* p, size_t bytes, bool guard) { if (p) bufs.push_back(Buf{p, bytes, guard}); }   // (a failed step may have allocated: it is released too)
};

inline int use_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || ndev <= device) return bfail(VLR_ERR_NO_DEVICE, "no HIP device %d (the engine has no CPU path)", device);
    VLR_HIP_OK(hipSetDevice(device));
    return VLR_OK;
}

// Exclusive prefix sums: workgroup b scans count array b (cnt_all + b * stride -> off_all + b * stride, its sum to total[b]).  Thread t
// sums the slice [t * per, (t + 1) * per), the sums are scanned in LDS, then the slice's offsets written.
template <class Count>
__global__ __launch_bounds__(kScanThreads) void scan_kernel(const Count* __restrict__ cnt_all, int64_t n, int64_t stride, uint64_t* __restrict__ off_all,
                                                            uint64_t* __restrict__ total) {
    __shared__ uint64_t s[2][kScanThreads];
    const Count* cnt = cnt_all + (int64_t)blockIdx.x * stride;
    uint64_t* off = off_all + (int64_t)blockIdx.x * stride;
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
    if (t == kScanThreads - 1) total[blockIdx.x] = s[cur][t];
}

// counters of the records a session saw (device: sums and a minimum, order-independent); C_OWN is the session's to name
enum Counter { C_REJECTED, C_BAD, C_FIRST_BAD, C_OWN, C_N };

// the state every session keeps; the session structs derive from it
struct Session {
    int device = 0;
    size_t window_bytes = (size_t)64 << 20;   // inflated bytes per split of the device reader
    uint64_t n_records = 0;             // records of the files given so far
    int64_t trunc_record = -1;          // a file ended inside this record
    bool collected = false;
    uint64_t status = 0;
    uint64_t counters[C_N] = {0, 0, ~0ull, 0};
    unsigned long long* d_counters = nullptr;
    uint64_t* d_total = nullptr;        // [arrays]
    // per record of a chunk: `arrays` count arrays (u32 or u64, the session's choice) and their scanned offsets, [arrays][rec_cap]
    void* d_cnt = nullptr; uint64_t* d_off = nullptr; size_t rec_cap = 0;
};

inline int open_session(Session& b, int device, int64_t window_bytes, int arrays) {
    b.device = device;
    if (window_bytes > 0) b.window_bytes = (size_t)window_bytes;
    int rc = upload(b.d_counters, (const unsigned long long*)b.counters, (size_t)C_N);
    return rc != VLR_OK ? rc : zeros(b.d_total, (size_t)arrays);
}

inline void close_session(Session& b) {
    void* p[] = {b.d_counters, b.d_total, b.d_cnt, b.d_off};
    for (void* q : p) if (q) (void)hipFree(q);
}

// room for the n records of a chunk in the count and offset arrays
template <class Count> int reserve_records(Session& b, int64_t n, int arrays, hipStream_t st) {
    if ((size_t)n <= b.rec_cap) return VLR_OK;
    VLR_HIP_OK(hipStreamSynchronize(st));
    if (b.d_cnt) (void)hipFree(b.d_cnt);
    if (b.d_off) (void)hipFree(b.d_off);
    b.d_cnt = nullptr; b.d_off = nullptr; b.rec_cap = 0;
    const size_t cap = (size_t)n + (size_t)n / 4 + 1024;
    VLR_HIP_OK(hipMalloc(&b.d_cnt, (size_t)arrays * cap * sizeof(Count)));
    VLR_HIP_OK(hipMalloc((void**)&b.d_off, (size_t)arrays * cap * 8));
    b.rec_cap = cap;
    return VLR_OK;
}

// the counts of the chunk's n records scanned into their offsets, the sums on the host; the stream is idle afterwards
template <class Count> int scan_records(Session& b, int64_t n, int arrays, uint64_t* total, hipStream_t st) {
    hipLaunchKernelGGL(scan_kernel<Count>, dim3((unsigned)arrays), dim3(kScanThreads), 0, st, (const Count*)b.d_cnt, n, (int64_t)b.rec_cap, b.d_off, b.d_total);
    VLR_HIP_OK(hipMemcpyAsync(total, b.d_total, (size_t)arrays * 8, hipMemcpyDeviceToHost, st));
    VLR_HIP_OK(hipStreamSynchronize(st));
    VLR_HIP_OK(hipGetLastError());
    return VLR_OK;
}

struct Timers { double *read, *feed, *split, *inflate, *total; };   // seconds of the device reader, see BamStream

// One more BAM file for a session.  run_chunk gets the split records of a chunk (it adds them to n_records); on_header may be empty.
inline int add_bam(Session& b, const char* path, const char* api_name, const Timers& t, std::function<int(const std::vector<std::string>& names)> on_header,
                   std::function<int(vlr_dev_file* df, int64_t n, hipStream_t st)> run_chunk) {
    if (!path) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: null", api_name);
    if (b.collected) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: the result was already read", api_name);
    if (b.trunc_record >= 0) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: the file before ended inside a record", api_name);
    if (hipSetDevice(b.device) != hipSuccess) return bfail(VLR_ERR_HIP, "hipSetDevice(%d) failed", b.device);
    BamStream bs;
    bs.device = b.device;
    bs.window = &b.window_bytes;
    bs.t_read = t.read; bs.t_feed = t.feed; bs.t_split = t.split; bs.t_inflate = t.inflate; bs.t_total = t.total;
    bs.on_header = std::move(on_header);
    bs.on_chunk = [&run_chunk](vlr_dev_file* df, int64_t n, uint64_t, const std::vector<std::string>&, const char*, void* st) { return run_chunk(df, n, (hipStream_t)st); };
    // a file that ends inside a record: malformed input, reported in the status word; the records in front of it count
    bs.on_truncated = [&b](uint64_t) { b.trunc_record = (int64_t)b.n_records; return (int)VLR_OK; };
    return stream_bam(bs, path);
}

// the counters back on the host, when the session ends
inline int read_counters(Session& b) {
    VLR_HIP_OK(hipMemcpy(b.counters, b.d_counters, sizeof b.counters, hipMemcpyDeviceToHost));
    return VLR_OK;
}
// a record the decode refused, or a file that ended inside one: the BAD_RECORD bit of the status word, and the first such record (-1: none)
inline bool bad_record_seen(const Session& b) { return b.counters[C_BAD] != 0 || b.trunc_record >= 0; }
inline int64_t first_bad_record(const Session& b) {
    const int64_t r = b.counters[C_BAD] ? (int64_t)b.counters[C_FIRST_BAD] : -1;
    return b.trunc_record >= 0 && (r < 0 || b.trunc_record < r) ? b.trunc_record : r;
}

// record-major hits -> locus-major, record order kept within a locus: a stable counting sort.  out[k] = raw[perm[k]] when perm is given.
template <class Hit> void locus_major(const std::vector<Hit>& raw, int64_t n_loci, std::vector<Hit>& out, std::vector<uint64_t>* perm) {
    std::vector<uint64_t> first((size_t)n_loci + 1, 0);
    for (const auto& h : raw) if ((int64_t)h.locus < n_loci) ++first[(size_t)h.locus + 1];
    for (size_t k = 0; k < (size_t)n_loci; ++k) first[k + 1] += first[k];
    out.resize((size_t)first[(size_t)n_loci]);
    if (perm) perm->resize(out.size());
    for (size_t k = 0; k < raw.size(); ++k) {
        const auto& h = raw[k];
        if ((int64_t)h.locus >= n_loci) continue;
        const size_t at = (size_t)first[h.locus]++;
        out[at] = h;
        if (perm) (*perm)[at] = k;
    }
}

}  // namespace vlr_bam

namespace vlr_bp {

// the SNV / MNV loci of an open call: kind and length of each, the order, and base_off[n_loci + 1] = where a locus' alleles start
inline int check_snv_mnv_loci(const char* api_name, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int32_t* len, const uint8_t* kind,
                              std::vector<uint64_t>& base_off) {
    base_off.assign((size_t)n_loci + 1, 0);
    for (int64_t k = 0; k < n_loci; ++k) {
        const bool snv = kind[k] == VLR_BASEPILEUP_SNV;
        if ((!snv && kind[k] != VLR_BASEPILEUP_MNV) || ref_id[k] < 0 || start[k] < 0 || (snv ? len[k] != 1 : (len[k] < 2 || len[k] > VLR_BASEPILEUP_MAX_LEN)))
            return vlr_bam::bfail(VLR_ERR_INVALID_ARGUMENT, "%s: locus %lld: kind %d with %d bases (an SNV has 1, an MNV 2 .. %d)", api_name, (long long)k, (int)kind[k],
                                  (int)len[k], VLR_BASEPILEUP_MAX_LEN);
        if (k > 0 && (ref_id[k] < ref_id[k - 1] || (ref_id[k] == ref_id[k - 1] && start[k] < start[k - 1])))
            return vlr_bam::bfail(VLR_ERR_INVALID_ARGUMENT, "%s: loci are not sorted by (ref_id, start) at %lld", api_name, (long long)k);
        base_off[(size_t)k + 1] = base_off[(size_t)k] + (uint64_t)len[k];
    }
    return VLR_OK;
}

// the checked loci and the quality tables on the device
struct DeviceLoci {
    int32_t* d_ref_id = nullptr; int64_t* d_start = nullptr; int32_t* d_len = nullptr; uint8_t* d_kind = nullptr; uint64_t* d_base_off = nullptr;
    uint8_t *d_refb = nullptr, *d_altb = nullptr;
    double* d_tables = nullptr;   // call, miscall, linear
    Tables tables{};
    Loci loci{};

    int upload(int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int32_t* len, const uint8_t* kind, const std::vector<uint64_t>& base_off,
               const uint8_t* ref_bases, const uint8_t* alt_bases) {
        using vlr_bam::upload;
        std::vector<double> tab(3 * 256);
        fill_tables(tab.data(), tab.data() + 256, tab.data() + 512);
        const size_t nl = (size_t)n_loci, nb = (size_t)base_off[nl];
        int rc;
        if ((rc = upload(d_ref_id, ref_id, nl)) != VLR_OK || (rc = upload(d_start, start, nl)) != VLR_OK || (rc = upload(d_len, len, nl)) != VLR_OK ||
            (rc = upload(d_kind, kind, nl)) != VLR_OK || (rc = upload(d_base_off, base_off.data(), nl + 1)) != VLR_OK || (rc = upload(d_refb, ref_bases, nb)) != VLR_OK ||
            (rc = upload(d_altb, alt_bases, nb)) != VLR_OK || (rc = upload(d_tables, tab.data(), tab.size())) != VLR_OK)
            return rc;
        tables = Tables{d_tables, d_tables + 256, d_tables + 512, ln_confusion(), ln_any()};
        loci = Loci{n_loci, d_ref_id, d_start, d_len, d_kind, d_base_off, d_refb, d_altb};
        return VLR_OK;
    }
    void free() {
        void* p[] = {d_ref_id, d_start, d_len, d_kind, d_base_off, d_refb, d_altb, d_tables};
        for (void* q : p) if (q) (void)hipFree(q);
    }
};

}  // namespace vlr_bp
