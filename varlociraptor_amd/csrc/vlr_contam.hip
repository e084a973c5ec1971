// vlr_contam.hip — the posterior grid of `estimate contamination` (estimation/contamination.rs:160-224) for gfx950.
//
// 4 x 101 events (maximum somatic VAF x contamination); the likelihood of an event is the sum over the kept de-novo SNVs of
// one interpolated allele-frequency density (the call's FORMAT/AFD list).  One workgroup owns VLR_CONTAM_BLOCK consecutive
// observations and one lane owns one event (seven wave64s, lanes 404..447 idle): the lane walks the block's observations in
// record order and adds its term, so every partial sum has one fixed order whatever the grid.  The per-observation values
// (offsets, MAP VAF, P(denovo)) are uniform over the workgroup; the lists are read directly (they are a few hundred bytes,
// every lane of the workgroup searches the same one at the same time).  A second kernel adds the block sums of an event
// sequentially in block order.  f64 throughout, no atomics; the Simpson / ln_sum_exp epilogue over the 404 joints runs on
// the host.  Contract and conventions: include/vlr.h (vlr_contamination_posterior).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/vlr.h"

extern "C" void vlr_set_error(const char* msg);  // vlr_host.cpp: the text behind vlr_last_error()

namespace vlr_contam {

constexpr int kBlock = VLR_CONTAM_BLOCK;
constexpr int kNC = VLR_CONTAM_N_C;
constexpr int kNMV = VLR_CONTAM_N_MV;
constexpr int kEvents = kNC * kNMV;                 // 404
constexpr int kThreads = ((kEvents + 63) / 64) * 64;  // 448: seven waves
constexpr int kReduceThreads = 64;

__device__ __forceinline__ double ln_add_exp(double a, double b) {  // bio LogProb::ln_add_exp
    if (b > a) { const double t = a; a = b; b = t; }
    if (a == -__builtin_huge_val()) return a;
    return a + log1p(exp(b - a));
}

__device__ __forceinline__ double ln_one_minus_exp(double p) {  // bio LogProb::ln_one_minus_exp
    if (p < -0.693) return log1p(-exp(p));
    return log(-expm1(p));
}

// VariantObservation::pdf (contamination.rs:84-117) over one list sorted by VAF, with the falling-segment decision of vlr.h
__device__ __forceinline__ double pdf(const double* __restrict__ v, const double* __restrict__ p, int n, double x) {
    int lo = 0, len = n;  // lower bound: first key >= x (a NaN x never compares: lo stays 0)
    while (len > 0) {
        const int half = len >> 1;
        if (v[lo + half] < x) { lo += half + 1; len -= half + 1; }
        else len = half;
    }
    if (lo < n && v[lo] == x) return p[lo];                     // case 1: exact key
    if (lo == 0 || lo == n) return -__builtin_huge_val();       // cases 3-5: outside the list, empty list
    const double xa = v[lo - 1], xb = v[lo], a = p[lo - 1], b = p[lo];
    const double ea = exp(a), eb = exp(b);
    const double ldx = log(x - xa);
    if (eb >= ea) return ln_add_exp(a, log((eb - ea) / (xb - xa)) + ldx);  // rising / flat: the reference's formula
    const double s = log((ea - eb) / (xb - xa)) + ldx;                    // falling: a.ln_sub_exp(ln|slope| + ln(x - xa))
    if (s >= a) return b;
    return a + ln_one_minus_exp(s - a);
}

__global__ void __launch_bounds__(kThreads) contam_block_sums(long long n_obs, const long long* __restrict__ off, const double* __restrict__ lv,
                                                              const double* __restrict__ lp, const double* __restrict__ map_vaf,
                                                              const double* __restrict__ ln_denovo, double max_vaf, double* __restrict__ partial) {
    const int e = threadIdx.x;
    if (e >= kEvents) return;
    const int m = e / kNC, i = e - m * kNC;
    const double mv = 0.25 * (double)(m + 1);                          // 0.25, 0.5, 0.75, 1.0 (exact)
    const double step = (1.0 - 0.0) / (double)(kNC - 1);               // itertools_num::linspace(0.0, 1.0, 101)
    const double c = 0.0 + step * (double)i;
    const double purity = 1.0 - c;
    const double mvp = mv * purity;
    const long long o0 = (long long)blockIdx.x * kBlock;
    const long long o1 = o0 + kBlock < n_obs ? o0 + kBlock : n_obs;
    double acc = 0.0;
    for (long long o = o0; o < o1; ++o) {
        double t;
        if (purity == 0.0) {
            t = ln_one_minus_exp(ln_denovo[o]);                           // no de-novo somatic mutation without tumour cells
        } else {
            const double x = mvp * (map_vaf[o] / max_vaf);              // VAFDist::get_expected_vaf, left to right
            const long long b = off[o];
            t = pdf(lv + b, lp + b, (int)(off[o + 1] - b), x);
        }
        acc += t;
    }
    partial[blockIdx.x * (long long)kEvents + e] = acc;
}

__global__ void __launch_bounds__(kReduceThreads) contam_event_sums(long long nb, const double* __restrict__ partial, double* __restrict__ total) {
    const int e = blockIdx.x * kReduceThreads + threadIdx.x;
    if (e >= kEvents) return;
    double acc = 0.0;
    for (long long b = 0; b < nb; ++b) acc += partial[b * kEvents + e];
    total[e] = acc;
}

// bio LogProb::ln_sum_exp: max m (first index), m + ln1p(sum over the others of e^(v - m)); NaN in, NaN out
double host_ln_sum_exp(const double* v, int n) {
    const double ninf = -std::numeric_limits<double>::infinity();
    int im = -1;
    for (int k = 0; k < n; ++k) {
        if (v[k] != v[k]) return v[k];
        if (im < 0 || v[k] > v[im]) im = k;
    }
    if (im < 0 || v[im] == ninf) return ninf;
    double s = 0.0;
    for (int k = 0; k < n; ++k)
        if (k != im && v[k] != ninf) s += std::exp(v[k] - v[im]);
    return v[im] + std::log1p(s);
}

int cfail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    vlr_set_error(buf);
    return code;
}

}  // namespace vlr_contam

extern "C" int vlr_contamination_posterior(int device, int64_t n_obs, const int64_t* list_offset, const double* list_vaf, const double* list_lnprob,
                                           const double* map_vaf, const double* ln_prob_denovo, double max_vaf, const double* ln_prior,
                                           double* ln_joint, double* ln_marginal) {
    using namespace vlr_contam;
    if (n_obs < 0 || !list_offset || !ln_prior || !ln_joint || !ln_marginal || (n_obs > 0 && (!map_vaf || !ln_prob_denovo)))
        return cfail(VLR_ERR_INVALID_ARGUMENT, "vlr_contamination_posterior: null argument or n_obs < 0");
    // the kernel indexes the lists through the offsets: they are checked here, before anything reaches the device
    if (list_offset[0] != 0) return cfail(VLR_ERR_INVALID_ARGUMENT, "list_offset[0] = %lld, not 0", (long long)list_offset[0]);
    for (int64_t o = 0; o < n_obs; ++o) {
        const int64_t b = list_offset[o], e = list_offset[o + 1];
        if (e < b || e - b > (int64_t)0x7fffffff) return cfail(VLR_ERR_INVALID_ARGUMENT, "list_offset decreases or spans too much at %lld", (long long)o);
        for (int64_t k = b; k < e; ++k) {
            if (list_vaf[k] != list_vaf[k] || (k > b && !(list_vaf[k - 1] < list_vaf[k])))
                return cfail(VLR_ERR_INVALID_ARGUMENT, "list %lld: VAF keys not strictly ascending (or NaN) at entry %lld", (long long)o, (long long)(k - b));
        }
    }
    const int64_t n_ent = list_offset[n_obs];
    if (n_ent > 0 && (!list_vaf || !list_lnprob)) return cfail(VLR_ERR_INVALID_ARGUMENT, "vlr_contamination_posterior: null list");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || ndev <= device)
        return cfail(VLR_ERR_NO_DEVICE, "no HIP device %d (the engine has no CPU path)", device);
    if (hipSetDevice(device) != hipSuccess) return cfail(VLR_ERR_HIP, "hipSetDevice(%d) failed", device);
    const int64_t nb = (n_obs + kBlock - 1) / kBlock;
    std::vector<double> total((size_t)kEvents, 0.0);
    if (nb > 0) {
        // one allocation: offsets | list VAFs | list values | MAP VAFs | P(denovo) | block sums | event sums
        const size_t w_off = (size_t)n_obs + 1, w_ent = (size_t)(n_ent > 0 ? n_ent : 1);
        const size_t words = w_off + 2 * w_ent + 2 * (size_t)n_obs + (size_t)nb * kEvents + kEvents;
        char* d = nullptr;
        if (hipMalloc((void**)&d, words * 8) != hipSuccess) { (void)hipGetLastError(); return cfail(VLR_ERR_OUT_OF_MEMORY, "hipMalloc(%zu)", words * 8); }
        long long* d_off = (long long*)d;
        double* d_lv = (double*)(d_off + w_off);
        double* d_lp = d_lv + w_ent;
        double* d_map = d_lp + w_ent;
        double* d_den = d_map + n_obs;
        double* d_part = d_den + n_obs;
        double* d_tot = d_part + (size_t)nb * kEvents;
        int rc = VLR_OK;
        do {
            if (hipMemcpy(d_off, list_offset, w_off * 8, hipMemcpyHostToDevice) != hipSuccess ||
                (n_ent > 0 && hipMemcpy(d_lv, list_vaf, (size_t)n_ent * 8, hipMemcpyHostToDevice) != hipSuccess) ||
                (n_ent > 0 && hipMemcpy(d_lp, list_lnprob, (size_t)n_ent * 8, hipMemcpyHostToDevice) != hipSuccess) ||
                hipMemcpy(d_map, map_vaf, (size_t)n_obs * 8, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(d_den, ln_prob_denovo, (size_t)n_obs * 8, hipMemcpyHostToDevice) != hipSuccess) { rc = cfail(VLR_ERR_HIP, "staging copy failed"); break; }
            hipLaunchKernelGGL(contam_block_sums, dim3((unsigned)nb), dim3(kThreads), 0, 0, (long long)n_obs, d_off, d_lv, d_lp, d_map, d_den, max_vaf, d_part);
            hipLaunchKernelGGL(contam_event_sums, dim3((kEvents + kReduceThreads - 1) / kReduceThreads), dim3(kReduceThreads), 0, 0, (long long)nb, d_part, d_tot);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) { rc = cfail(VLR_ERR_HIP, "contamination kernels: %s", hipGetErrorString(e)); break; }
            if (hipMemcpy(total.data(), d_tot, kEvents * 8, hipMemcpyDeviceToHost) != hipSuccess) { rc = cfail(VLR_ERR_HIP, "result copy failed"); break; }
        } while (0);
        (void)hipFree(d);
        if (rc != VLR_OK) return rc;
    }
    for (int e = 0; e < kEvents; ++e) ln_joint[e] = ln_prior[e % kNC] + total[(size_t)e];
    // Marginal (contamination.rs:196-224): Simpson over the 101 contaminations per maximum somatic VAF, weights and terms in the
    // order of the call path's Simpson (interior points, then both ends), then ln_sum_exp of the four integrals
    double integral[kNMV];
    std::vector<double> terms((size_t)kNC);
    for (int m = 0; m < kNMV; ++m) {
        const double* f = ln_joint + m * kNC;
        int k = 0;
        for (int i = 1; i < kNC - 1; ++i) terms[(size_t)k++] = f[i] + std::log((double)(2 + (i % 2) * 2));
        terms[(size_t)k++] = f[0];
        terms[(size_t)k++] = f[kNC - 1];
        integral[m] = host_ln_sum_exp(terms.data(), kNC) + std::log(1.0 - 0.0) - std::log((double)(kNC - 1)) - std::log(3.0);
    }
    *ln_marginal = host_ln_sum_exp(integral, kNMV);
    return VLR_OK;
}
