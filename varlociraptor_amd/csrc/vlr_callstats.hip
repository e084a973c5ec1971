// vlr_callstats.hip — gfx950 kernels of the two downstream consumers of a calls file:
//   `filter-calls posterior-odds`   (filtration/posterior_odds.rs:62-79): one Kass-Raftery decision per allele;
//   `estimate mutational-burden`    (estimation/mutational_burden.rs:186-190, 214-346): ln_sum_exp of the allele probabilities
//                                   per (VAF range, group) cell.
// Contracts and conventions: include/vlr.h (vlr_posterior_odds_keep, vlr_range_group_lse).  The record I/O of both commands is
// csrc/vlr_ingest.cpp (vlr_calls_filter_odds, vlr_calls_mutational_burden); the numpy restatements the tests compare with are
// varlociraptor_amd/odds.py and varlociraptor_amd/burden.py.
//
// vlr_range_group_lse.  n entries (vaf, ln_prob, group), R half-open ranges [lo_r, hi_r), G groups; cell (r, g) holds the
// entries of group g with lo_r <= vaf < hi_r (two f64 comparisons with the tabulated bounds, nothing derived from vaf), and
//   out[r * G + g] = m + ln1p((c - 1) + S),   m = the cell's maximum ln_prob, c = the number of entries equal to m,
//                                             S = sum of e^(ln_prob - m) over the entries below m
// which is bio's ln_sum_exp (the maximum apart, ln1p of the others; an entry equal to the maximum
// contributes e^0 = 1 exactly).  Two passes over the entries, both with the same geometry:
//   pass 1: the maximum of every cell (order-free: a maximum does not depend on the order it is taken in);
//   pass 2: c (an integer) and S.
// SUMMATION ORDER OF S (fixed): the entries in chunks of VLR_LSE_CHUNK consecutive ones; within a chunk the terms of one cell
//   are added sequentially in entry order starting from 0.0; the chunk sums of a cell are then added sequentially in chunk
//   order starting from 0.0.  The order depends on nothing but the entry order: not on the launch geometry, the scheduling,
//   the group tiling, the number of chunks per launch or on how the entries were uploaded.  No floating-point atomics
//   (no atomics at all): the same input gives the same bits.
// Geometry: one workgroup (256 threads, wave64) per chunk.  A thread owns range r = t % R and the groups g with g % K == t / R
//   (K = a power of two <= 256 / R), so every cell of the workgroup has exactly one owner, which walks the chunk's entries in
//   order.  All lanes read the same entry (a uniform address: the loads are scalar or broadcast), test their own range in
//   registers and update their own row of the workgroup's cell table in LDS: maximum (f64), S (f64), c (u32) = 20 bytes per
//   cell, rows padded to an odd number of f64 so that the lanes of a wave (consecutive r, same g) fall on different banks.
//   R = 100, G = 14 is 30 kB.  When R x G does not fit 64 kB the groups are tiled and a workgroup skips the entries outside
//   its tile.  Per-chunk partials go to a slab [chunk][R x G]; a second kernel adds them per cell in chunk order.  The slab
//   is bounded (kSlabBytes): longer inputs are processed in batches of chunks, each batch's partials added onto the running
//   totals, which is the same sequence of additions.
// NaN / inf: a NaN vaf is in no range.  A NaN ln_prob makes its cells NaN (the maximum becomes NaN and stays).  A cell without
//   entries, or whose entries are all -inf, is -inf.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/vlr.h"
#include "vlr_callstats.h"

extern "C" void vlr_set_error(const char* msg);  // vlr_host.cpp: the text behind vlr_last_error()

namespace vlr_callstats {

constexpr int kChunk = VLR_LSE_CHUNK;
constexpr int kThreads = 256;
constexpr int kLdsBytes = 64 * 1024;             // cell table of one workgroup (static + dynamic LDS without opting in)
constexpr size_t kSlabBytes = (size_t)256 << 20;  // per-chunk partials of one batch
constexpr int kCellBytes = 20;                    // maximum, S, c

__device__ __forceinline__ double fold_max(double m, double p) {  // NaN-sticky maximum
    return (m == m && !(p <= m)) ? p : m;
}

// PASS 1: part_a[chunk][cell] = maximum; PASS 2: part_a = S, part_c = c (cell_max: [R * G] from pass 1)
template <int PASS>
__global__ void __launch_bounds__(kThreads) lse_chunk_pass(long long n, long long chunk0, const double* __restrict__ vaf, const double* __restrict__ lp,
                                                           const int* __restrict__ grp, int R, const double* __restrict__ lo, const double* __restrict__ hi,
                                                           int G, int g0, int gt, int gp, int K, const double* __restrict__ cell_max,
                                                           double* __restrict__ part_a, unsigned* __restrict__ part_c) {
    extern __shared__ double lds[];
    const int cells_lds = R * gp;
    double* mx = lds;
    double* sum = lds + cells_lds;
    unsigned* cnt = (unsigned*)(lds + 2 * cells_lds);
    const int t = threadIdx.x;
    for (int i = t; i < cells_lds; i += kThreads) {
        const int ri = i / gp, gi = i - ri * gp;
        if (PASS == 1) mx[i] = -__builtin_huge_val();
        else {
            mx[i] = gi < gt ? cell_max[(long long)ri * G + g0 + gi] : -__builtin_huge_val();
            sum[i] = 0.0;
            cnt[i] = 0u;
        }
    }
    __syncthreads();
    const int r = t % R, k = t / R;
    const long long e0 = (chunk0 + blockIdx.x) * (long long)kChunk;
    const long long e1 = e0 + kChunk < n ? e0 + kChunk : n;
    if (k < K) {
        const double lo_r = lo[r], hi_r = hi[r];
        const int row = r * gp;
        for (long long e = e0; e < e1; ++e) {
            const int g = grp[e] - g0;
            if ((unsigned)g >= (unsigned)gt || (g & (K - 1)) != k) continue;
            const double v = vaf[e];
            if (!(lo_r <= v && v < hi_r)) continue;
            const double p = lp[e];
            const int idx = row + g;
            const double m = mx[idx];
            if (PASS == 1) mx[idx] = fold_max(m, p);
            else if (p == m) cnt[idx] += 1u;
            else sum[idx] += exp(p - m);
        }
    }
    __syncthreads();
    const long long base = (long long)blockIdx.x * R * G;
    for (int i = t; i < R * gt; i += kThreads) {
        const int ri = i / gt, gi = i - ri * gt;
        const long long c = base + (long long)ri * G + g0 + gi;
        if (PASS == 1) part_a[c] = mx[ri * gp + gi];
        else { part_a[c] = sum[ri * gp + gi]; part_c[c] = cnt[ri * gp + gi]; }
    }
}

// the partials of one batch onto the running totals, per cell in chunk order
template <int PASS>
__global__ void __launch_bounds__(kThreads) lse_combine(int cells, long long nb, int first, const double* __restrict__ part_a, const unsigned* __restrict__ part_c,
                                                        double* __restrict__ tot_a, unsigned long long* __restrict__ tot_c) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= cells) return;
    if (PASS == 1) {
        double m = first ? -__builtin_huge_val() : tot_a[c];
        for (long long b = 0; b < nb; ++b) m = fold_max(m, part_a[b * cells + c]);
        tot_a[c] = m;
    } else {
        double s = first ? 0.0 : tot_a[c];
        unsigned long long k = first ? 0ull : tot_c[c];
        for (long long b = 0; b < nb; ++b) { s += part_a[b * cells + c]; k += part_c[b * cells + c]; }
        tot_a[c] = s;
        tot_c[c] = k;
    }
}

__global__ void __launch_bounds__(kThreads) lse_finish(int cells, const double* __restrict__ cell_max, const double* __restrict__ tot_s,
                                                       const unsigned long long* __restrict__ tot_c, double* __restrict__ out) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= cells) return;
    const double m = cell_max[c];
    out[c] = (m == -__builtin_huge_val()) ? m : m + log1p(((double)tot_c[c] - 1.0) + tot_s[c]);
}

// BayesFactor::new(other, target) = e^(other - target), evidence_kass_raftery, kept while below min_level.
// Decided in log space on d = other - target.  k <= 1: a correctly rounded e^d is <= 1 exactly when d < 2^-53 (e^d = 1 + d + d^2/2 + ...
// lies below the midpoint 1 + 2^-53 of 1 and its successor for every double d < 2^-53, and above it at d = 2^-53), so d == 0 is NONE
// exactly and so is a positive d that the reference's exp rounds away.  k <= 3, 20, 150: d <= ln 3, ln 20, ln 150 (tabulated by the
// host), which can differ from the reference's e^d <= b only where d is within rounding of ln b.  A NaN d fails every comparison.
__global__ void __launch_bounds__(kThreads) odds_keep(long long n, const double* __restrict__ ln_target, const double* __restrict__ ln_other,
                                                      const uint8_t* __restrict__ valid, int min_level, double ln3, double ln20, double ln150,
                                                      uint8_t* __restrict__ keep) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const double d = ln_other[i] - ln_target[i];
        const int level = d < 0x1p-53 ? 0 : d <= ln3 ? 1 : d <= ln20 ? 2 : d <= ln150 ? 3 : 4;
        keep[i] = (uint8_t)(((valid[i] & 3) == 3) && level < min_level);
    }
}

// device time of the kernels of the last call of each entry point (hipEvent pair around the launches), for vlr_callstats_last_kernel_ms
thread_local double g_last_ms[2] = {0.0, 0.0};
struct KernelTimer {
    hipEvent_t a = nullptr, b = nullptr;
    void start() { if (hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) (void)hipEventRecord(a, 0); }
    double stop() {  // milliseconds; 0 when the events could not be made
        float ms = 0.0f;
        if (a && b && hipEventRecord(b, 0) == hipSuccess && hipEventSynchronize(b) == hipSuccess) (void)hipEventElapsedTime(&ms, a, b);
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        a = b = nullptr;
        return (double)ms;
    }
};

int cfail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    vlr_set_error(buf);
    return code;
}

int pick_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || ndev <= device)
        return cfail(VLR_ERR_NO_DEVICE, "no HIP device %d (the engine has no CPU path)", device);
    if (hipSetDevice(device) != hipSuccess) return cfail(VLR_ERR_HIP, "hipSetDevice(%d) failed", device);
    return VLR_OK;
}

}  // namespace vlr_callstats

extern "C" int vlr_launch_range_group_lse(int device, int64_t n, const double* vaf, const double* ln_prob, const int32_t* group, int n_ranges,
                                          const double* lo, const double* hi, int n_groups, int64_t piece, double* out) {
    using namespace vlr_callstats;
    const int R = n_ranges, G = n_groups;
    if (n < 0 || R < 1 || R > VLR_LSE_MAX_RANGES || G < 1 || G > VLR_LSE_MAX_GROUPS || !lo || !hi || !out || (n > 0 && (!vaf || !ln_prob || !group)))
        return cfail(VLR_ERR_INVALID_ARGUMENT, "vlr_range_group_lse: null argument, n < 0, n_ranges outside [1, %d] or n_groups outside [1, %d]",
                     VLR_LSE_MAX_RANGES, VLR_LSE_MAX_GROUPS);
    // the kernels index the cell tables through the groups: they are checked here, before anything reaches the device
    for (int64_t i = 0; i < n; ++i)
        if (group[i] < 0 || group[i] >= G) return cfail(VLR_ERR_INVALID_ARGUMENT, "vlr_range_group_lse: group %d of entry %lld outside [0, %d)", group[i], (long long)i, G);
    const int cells = R * G;
    if (n == 0) {
        for (int c = 0; c < cells; ++c) out[c] = -std::numeric_limits<double>::infinity();
        return VLR_OK;
    }
    if (int rc = pick_device(device)) return rc;
    // group tile: the widest (odd-padded) row such that R rows of 20-byte cells fit the LDS budget
    int gt = std::min(G, kLdsBytes / (kCellBytes * R));
    if (gt > 1 && !(gt & 1) && R * (gt + 1) * kCellBytes > kLdsBytes) --gt;
    const int gp = gt | 1;
    int K = 1;
    while (K * 2 <= gt && K * 2 * R <= kThreads) K *= 2;
    const size_t lds_bytes = (size_t)R * gp * kCellBytes;
    const int64_t n_chunks = (n + kChunk - 1) / kChunk;
    const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(n_chunks, (int64_t)(kSlabBytes / ((size_t)cells * 12))));
    // one allocation: vaf | ln_prob | bounds | maxima | S totals | c totals | out | partial S | group | partial c
    const size_t w8 = 2 * (size_t)n + 2 * (size_t)R + 4 * (size_t)cells + (size_t)batch * cells;
    const size_t bytes = w8 * 8 + ((size_t)n + (size_t)batch * cells) * 4;
    char* d = nullptr;
    if (hipMalloc((void**)&d, bytes) != hipSuccess) { (void)hipGetLastError(); return cfail(VLR_ERR_OUT_OF_MEMORY, "hipMalloc(%zu)", bytes); }
    double* d_vaf = (double*)d;
    double* d_lp = d_vaf + n;
    double* d_lo = d_lp + n;
    double* d_hi = d_lo + R;
    double* d_max = d_hi + R;
    double* d_sum = d_max + cells;
    unsigned long long* d_cnt = (unsigned long long*)(d_sum + cells);
    double* d_out = (double*)(d_cnt + cells);
    double* d_pa = d_out + cells;
    int* d_grp = (int*)(d_pa + (size_t)batch * cells);
    unsigned* d_pc = (unsigned*)(d_grp + n);
    int rc = VLR_OK;
    do {
        const int64_t step = piece > 0 ? piece : n;
        bool ok = hipMemcpy(d_lo, lo, (size_t)R * 8, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_hi, hi, (size_t)R * 8, hipMemcpyHostToDevice) == hipSuccess;
        for (int64_t b = 0; ok && b < n; b += step) {
            const size_t m = (size_t)std::min<int64_t>(step, n - b);
            ok = hipMemcpy(d_vaf + b, vaf + b, m * 8, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_lp + b, ln_prob + b, m * 8, hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(d_grp + b, group + b, m * 4, hipMemcpyHostToDevice) == hipSuccess;
        }
        if (!ok) { rc = cfail(VLR_ERR_HIP, "staging copy failed"); break; }
        const dim3 cgrid((unsigned)((cells + kThreads - 1) / kThreads));
        KernelTimer timer;
        timer.start();
        for (int pass = 1; pass <= 2; ++pass) {
            for (int64_t c0 = 0; c0 < n_chunks; c0 += batch) {
                const int64_t nb = std::min<int64_t>(batch, n_chunks - c0);
                for (int g0 = 0; g0 < G; g0 += gt) {
                    const int w = std::min(gt, G - g0);
                    if (pass == 1) hipLaunchKernelGGL(lse_chunk_pass<1>, dim3((unsigned)nb), dim3(kThreads), lds_bytes, 0, (long long)n, (long long)c0, d_vaf, d_lp, d_grp, R, d_lo, d_hi, G, g0, w, gp, K, d_max, d_pa, d_pc);
                    else hipLaunchKernelGGL(lse_chunk_pass<2>, dim3((unsigned)nb), dim3(kThreads), lds_bytes, 0, (long long)n, (long long)c0, d_vaf, d_lp, d_grp, R, d_lo, d_hi, G, g0, w, gp, K, d_max, d_pa, d_pc);
                }
                if (pass == 1) hipLaunchKernelGGL(lse_combine<1>, cgrid, dim3(kThreads), 0, 0, cells, (long long)nb, (int)(c0 == 0), d_pa, d_pc, d_max, d_cnt);
                else hipLaunchKernelGGL(lse_combine<2>, cgrid, dim3(kThreads), 0, 0, cells, (long long)nb, (int)(c0 == 0), d_pa, d_pc, d_sum, d_cnt);
            }
        }
        hipLaunchKernelGGL(lse_finish, cgrid, dim3(kThreads), 0, 0, cells, d_max, d_sum, d_cnt, d_out);
        g_last_ms[0] = timer.stop();
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { rc = cfail(VLR_ERR_HIP, "range/group kernels: %s", hipGetErrorString(e)); break; }
        if (hipMemcpy(out, d_out, (size_t)cells * 8, hipMemcpyDeviceToHost) != hipSuccess) { rc = cfail(VLR_ERR_HIP, "result copy failed"); break; }
    } while (0);
    (void)hipFree(d);
    return rc;
}

extern "C" int vlr_range_group_lse(int device, int64_t n, const double* vaf, const double* ln_prob, const int32_t* group, int n_ranges, const double* lo,
                                   const double* hi, int n_groups, double* out) {
    return vlr_launch_range_group_lse(device, n, vaf, ln_prob, group, n_ranges, lo, hi, n_groups, 0, out);
}

extern "C" int vlr_posterior_odds_keep(int device, int64_t n, const double* ln_target, const double* ln_other, const uint8_t* valid, int min_level, uint8_t* keep) {
    using namespace vlr_callstats;
    if (n < 0 || min_level < VLR_ODDS_NONE || min_level > VLR_ODDS_VERY_STRONG || (n > 0 && (!ln_target || !ln_other || !valid || !keep)))
        return cfail(VLR_ERR_INVALID_ARGUMENT, "vlr_posterior_odds_keep: null argument, n < 0 or min_level outside [0, 4]");
    if (n == 0) return VLR_OK;
    if (int rc = pick_device(device)) return rc;
    const size_t nn = (size_t)n;
    char* d = nullptr;
    if (hipMalloc((void**)&d, nn * 18) != hipSuccess) { (void)hipGetLastError(); return cfail(VLR_ERR_OUT_OF_MEMORY, "hipMalloc(%zu)", nn * 18); }
    double* d_t = (double*)d;
    double* d_o = d_t + nn;
    uint8_t* d_v = (uint8_t*)(d_o + nn);
    uint8_t* d_k = d_v + nn;
    int rc = VLR_OK;
    do {
        if (hipMemcpy(d_t, ln_target, nn * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_o, ln_other, nn * 8, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_v, valid, nn, hipMemcpyHostToDevice) != hipSuccess) { rc = cfail(VLR_ERR_HIP, "staging copy failed"); break; }
        const unsigned grid = (unsigned)std::min<size_t>((nn + kThreads - 1) / kThreads, 2048);
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(odds_keep, dim3(grid), dim3(kThreads), 0, 0, (long long)n, d_t, d_o, d_v, min_level, std::log(3.0), std::log(20.0), std::log(150.0), d_k);
        g_last_ms[1] = timer.stop();
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { rc = cfail(VLR_ERR_HIP, "posterior-odds kernel: %s", hipGetErrorString(e)); break; }
        if (hipMemcpy(keep, d_k, nn, hipMemcpyDeviceToHost) != hipSuccess) { rc = cfail(VLR_ERR_HIP, "result copy failed"); break; }
    } while (0);
    (void)hipFree(d);
    return rc;
}

extern "C" int vlr_callstats_last_kernel_ms(double* range_group_lse_ms, double* posterior_odds_ms) {
    if (range_group_lse_ms) *range_group_lse_ms = vlr_callstats::g_last_ms[0];
    if (posterior_odds_ms) *posterior_odds_ms = vlr_callstats::g_last_ms[1];
    return VLR_OK;
}
