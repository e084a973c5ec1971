// vlr_fragpileup.hip — fragment observations of SNV / MNV candidates from BAM records for gfx950 (vlr_fragpileup_*, include/vlr.h): the
// text of vlr_fragpileup.h over every record of the BAM files streamed through the device reader (vlr_bamstream.h), and the host driver
// of the session.
//
// Member pass, per chunk of split records (one record per thread, as in vlr_basepileup.hip):
//   frag_count_kernel    thread i decodes record i, finds the loci whose window holds its start: cnt[i] = members, and when it is a member
//                        of any locus nbytes[i] = bytes of its QNAME, nxa[i] = alt-locus keys of its XA:Z tag; rejected and bad records go
//                        to integer counters
//   vlr_bam::scan_kernel one workgroup per count array (cnt, nbytes, nxa; vlr_bamsession.h, u32 counts): exclusive prefix sums
//   frag_fill_kernel     thread i builds the members of record i again and writes them at members[base + off[i] ...), its name at
//                        names[name_base + noff[i] ...), its keys at keys[key_base + xoff[i] ...); what would lie behind a capacity is
//                        not written.  It adds the record's members
//                        to the per-locus counters (sums: order-independent)
// so the places of members, names and keys are functions of the record order alone.
// Fragment pass, at vlr_fragpileup_result:
//   vlr_bam::scan_kernel per-locus member counts -> the loci's first slots
//   frag_scatter_kernel  member m takes the next free slot of its locus (an atomic cursor: the placement within a locus is not stable and
//                        need not be, the sort below is on a total key)
//   frag_locus_kernel    one workgroup per locus: the member indices go to LDS, a bitonic sort orders them by (QNAME bytes, record ordinal),
//                        the thread at the first member of each run of equal names forms the fragment's observation (vlr_fp::run_obs), a
//                        prefix sum over the flags of the runs that gave one ranks them in name order, the read positions that count for
//                        major_read_position are sorted in the same LDS array and thread 0 takes their mode; then the indices of the
//                        alt-locus keys of all observations are laid out by a second prefix sum, sorted in that array by (contig hash,
//                        bucket), and thread 0 takes major_alt_locus
//   vlr_bam::scan_kernel per-locus observation counts -> the loci's offsets
//   frag_gather_kernel   one workgroup per locus writes its observations at the offset, in rank order, with VLR_FRAGPILEUP_READPOS_MAJOR
//                        and the alt_locus class (vlr_fp::alt_locus_class)
// No atomic decides a place or an order that reaches the output: the cursors only fill the sort's input.
//
// LDS of frag_locus_kernel: 4 B index + 2 B rank per member + 2 KiB of scan cells = 26 KiB at VLR_FRAGPILEUP_MAX_MEMBERS = 4096, six
// workgroups per CU by LDS.
// Bounds: a record is read only after vlr_bp::decode checked it; members[k] is written for k < member capacity, names[k] for
// k < name capacity, keys[k] for k < key capacity; perm / tmp / rank / the pair arrays are sized by the member count and every index into
// them is below a locus' count, which sums to it; the output is sized by the scanned observation count; guard bytes behind every one of
// these buffers are checked at the end (vlr_bam::guarded / guard_intact).  The session's common state, the wiring of a file into the
// device reader and the SNV / MNV loci on the device are vlr_bamsession.h's.
#include <cstring>

#include "vlr_bamsession.h"
#include "vlr_fragpileup.h"

static_assert(sizeof(vlr_fragpileup_obs) == 56, "observation layout");
static_assert(sizeof(vlr_fragpileup_locus) == 24, "locus record layout");
static_assert(sizeof(vlr_fp::Member) == 72, "member layout");
static_assert(sizeof(vlr_fp::AltKey) == 16, "key layout");

namespace vlr_fp {

using vlr_bam::C_BAD;
using vlr_bam::C_FIRST_BAD;
using vlr_bam::C_REJECTED;
using vlr_bam::kScanThreads;
enum { K_MEMBERS = 0, K_NAME = 1, K_XA = 2, K_N = 3 };   // the three counts of a record
constexpr int kThreads = 256;
constexpr int kLocusThreads = 256;
constexpr uint32_t kMax = VLR_FRAGPILEUP_MAX_MEMBERS;
constexpr uint32_t kSentinel = 0xffffffffu;
constexpr uint16_t kNoRank = 0xffffu;

__global__ __launch_bounds__(kThreads) void frag_count_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                              vlr_bp::Tables t, vlr_bp::Loci L, int realign, int64_t window, uint64_t coeff,
                                                              uint32_t* __restrict__ cnt, uint32_t* __restrict__ nbytes, uint32_t* __restrict__ nxa,
                                                              unsigned long long* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = starts[i], end = starts[i + 1];
    const RecMembers r = record_members(t, L, base + o, end - o, rec0 + (uint64_t)i, realign != 0, window, coeff, nullptr, 0, 0, nullptr, 0, nullptr, 0);
    cnt[i] = r.n_members;
    nbytes[i] = r.name_bytes;
    nxa[i] = r.n_xa;
    if (r.cls == vlr_bp::REC_REJECTED) atomicAdd(&counters[C_REJECTED], 1ull);
    if (r.cls == vlr_bp::REC_BAD) { atomicAdd(&counters[C_BAD], 1ull); atomicMin(&counters[C_FIRST_BAD], (unsigned long long)(rec0 + (uint64_t)i)); }
}

__global__ __launch_bounds__(kThreads) void frag_fill_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                             vlr_bp::Tables t, vlr_bp::Loci L, int realign, int64_t window, uint64_t coeff,
                                                             const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ nbytes, const uint64_t* __restrict__ off,
                                                             const uint64_t* __restrict__ noff, const uint64_t* __restrict__ xoff, uint64_t member0, uint64_t member_cap,
                                                             uint64_t name0, uint64_t name_cap, uint64_t key0, uint64_t key_cap, Member* __restrict__ members,
                                                             uint8_t* __restrict__ names, AltKey* __restrict__ keys, uint32_t* __restrict__ locus_cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || cnt[i] == 0) return;
    const uint64_t first = member0 + off[i];
    if (first >= member_cap) return;
    const uint64_t room = member_cap - first;
    const uint64_t name_at = name0 + noff[i];
    uint8_t* name_dst = name_at + (uint64_t)nbytes[i] <= name_cap ? names + name_at : nullptr;
    const uint64_t key_at = key0 + xoff[i];
    const uint64_t key_room = key_at < key_cap ? key_cap - key_at : 0;
    const uint64_t o = starts[i], end = starts[i + 1];
    const RecMembers r = record_members(t, L, base + o, end - o, rec0 + (uint64_t)i, realign != 0, window, coeff, members + first, room, name_at, name_dst, key_at,
                                        key_room ? keys + key_at : nullptr, key_room);
    const uint64_t written = std::min<uint64_t>(r.n_members, room);
    for (uint64_t k = 0; k < written; ++k) {
        const uint32_t li = members[first + k].locus;
        if ((int64_t)li < L.n) atomicAdd(&locus_cnt[li], 1u);
    }
}

__global__ __launch_bounds__(kThreads) void frag_scatter_kernel(const Member* __restrict__ members, uint64_t n_members, int64_t n_loci, const uint64_t* __restrict__ locus_off,
                                                                const uint32_t* __restrict__ locus_cnt, uint32_t* __restrict__ cursor, uint32_t* __restrict__ perm) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_members) return;
    const uint32_t li = members[m].locus;
    if ((int64_t)li >= n_loci) return;
    const uint32_t k = atomicAdd(&cursor[li], 1u);
    const uint64_t slot = locus_off[li] + k;
    if (k < locus_cnt[li] && slot < n_members) perm[slot] = (uint32_t)m;
}

// a <= b in the sort's order; the sentinel is the greatest element
__device__ inline bool idx_less(const Member* __restrict__ M, const uint8_t* __restrict__ names, uint32_t a, uint32_t b) {
    if (a == kSentinel) return false;
    if (b == kSentinel) return true;
    return member_less(names, M[a], M[b]);
}

// bitonic sort of v[0 .. P), P a power of two, ascending by `less`
template <class Less>
__device__ inline void bitonic(uint32_t* v, uint32_t P, Less less) {
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += kLocusThreads) {
                const uint32_t x = i ^ j;
                if (x > i) {
                    const uint32_t a = v[i], b = v[x];
                    const bool up = (i & k) == 0;
                    if (up ? less(b, a) : less(a, b)) { v[i] = b; v[x] = a; }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kLocusThreads) void frag_locus_kernel(const Member* __restrict__ M, const uint8_t* __restrict__ names, const AltKey* __restrict__ keys,
                                                                   const uint32_t* __restrict__ perm, const uint64_t* __restrict__ locus_off,
                                                                   const uint32_t* __restrict__ locus_cnt, uint32_t max_mapq, vlr_fragpileup_obs* tmp, uint32_t* pair_left,
                                                                   uint32_t* pair_right, uint16_t* __restrict__ rank_out, uint32_t* __restrict__ n_obs,
                                                                   uint32_t* __restrict__ major, AltKey* __restrict__ major_key, uint32_t* __restrict__ have_major_key,
                                                                   uint32_t* __restrict__ lstatus) {
    __shared__ uint32_t idx[kMax];
    __shared__ uint16_t rnk[kMax];
    __shared__ uint32_t part[2][kLocusThreads];
    const uint32_t l = blockIdx.x, t = threadIdx.x;
    const uint32_t n = locus_cnt[l];
    const uint64_t base = locus_off[l];
    if (n == 0 || n > kMax) {   // (uniform over the workgroup)
        if (t == 0) {
            n_obs[l] = 0; major[l] = VLR_BASEPILEUP_NO_READ_POSITION; have_major_key[l] = 0;
            lstatus[l] = n > kMax ? VLR_FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS : 0u;
        }
        return;
    }
    uint32_t P = 1;
    while (P < n) P <<= 1;
    for (uint32_t i = t; i < P; i += kLocusThreads) idx[i] = i < n ? perm[base + i] : kSentinel;
    __syncthreads();
    bitonic(idx, P, [&](uint32_t a, uint32_t b) { return idx_less(M, names, a, b); });
    // the fragment of every run of equal names
    for (uint32_t i = t; i < n; i += kLocusThreads) {
        uint16_t flag = 0;
        if (i == 0 || compare_names(names, M[idx[i - 1]], M[idx[i]]) != 0) {
            vlr_fragpileup_obs o;
            uint32_t ml, mr;
            if (run_obs(M, names, idx, i, n, max_mapq, o, &ml, &mr)) { tmp[base + i] = o; pair_left[base + i] = ml; pair_right[base + i] = mr; flag = 1; }
        }
        rnk[i] = flag;
    }
    __syncthreads();
    // ranks in name order: exclusive prefix sum of the flags
    const uint32_t per = (n + kLocusThreads - 1) / kLocusThreads;
    const uint32_t lo = std::min(t * per, n), hi = std::min(lo + per, n);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += rnk[i];
    part[0][t] = sum;
    __syncthreads();
    int cur = 0;
    for (uint32_t d = 1; d < (uint32_t)kLocusThreads; d <<= 1) {
        part[cur ^ 1][t] = part[cur][t] + (t >= d ? part[cur][t - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    uint32_t run = part[cur][t] - sum;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint16_t f = rnk[i];
        rnk[i] = f ? (uint16_t)run : kNoRank;
        run += f;
    }
    const uint32_t total = part[cur][kLocusThreads - 1];
    __syncthreads();
    // major_read_position: the read positions that count, sorted; the others are sentinels behind them
    for (uint32_t i = t; i < P; i += kLocusThreads) {
        uint32_t key = kSentinel;
        if (i < n) {
            rank_out[base + i] = rnk[i];
            if (rnk[i] != kNoRank && counts_for_major(tmp[base + i])) key = tmp[base + i].read_position;
        }
        idx[i] = key;
    }
    __syncthreads();
    bitonic(idx, P, [](uint32_t a, uint32_t b) { return a < b; });
    uint32_t major_pos = VLR_BASEPILEUP_NO_READ_POSITION;
    if (t == 0) {
        uint32_t m = 0;
        while (m < n && idx[m] != kSentinel) ++m;
        bool found = false;
        const uint32_t v = major_of_sorted(idx, m, &found);
        if (found) major_pos = v;
    }
    __syncthreads();
    // major_alt_locus: the pool indices of the keys of all observations, laid out in name order by a prefix sum, sorted by key
    uint32_t ksum = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        if (rnk[i] == kNoRank) continue;
        const uint32_t mr = pair_right[base + i];
        ksum = std::min(ksum + M[pair_left[base + i]].xa_n, kMax + 1u);
        if (mr != kSentinel) ksum = std::min(ksum + M[mr].xa_n, kMax + 1u);
    }
    part[0][t] = ksum;
    __syncthreads();
    cur = 0;
    for (uint32_t d = 1; d < (uint32_t)kLocusThreads; d <<= 1) {
        part[cur ^ 1][t] = part[cur][t] + (t >= d ? part[cur][t - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    const uint32_t n_keys = part[cur][kLocusThreads - 1];   // (every slice sum is capped at kMax + 1: no overflow, and exact up to kMax)
    if (n_keys > kMax) {   // (uniform)
        if (t == 0) { n_obs[l] = 0; major[l] = VLR_BASEPILEUP_NO_READ_POSITION; have_major_key[l] = 0; lstatus[l] = VLR_FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI; }
        return;
    }
    uint32_t PK = 1;
    while (PK < n_keys) PK <<= 1;
    for (uint32_t i = t; i < PK; i += kLocusThreads) idx[i] = kSentinel;
    __syncthreads();
    uint32_t at = part[cur][t] - ksum;
    for (uint32_t i = lo; i < hi; ++i) {
        if (rnk[i] == kNoRank) continue;
        const Member& ml = M[pair_left[base + i]];
        for (uint32_t k = 0; k < ml.xa_n && at < kMax; ++k) idx[at++] = (uint32_t)(ml.xa_off + k);
        const uint32_t mr = pair_right[base + i];
        if (mr != kSentinel) for (uint32_t k = 0; k < M[mr].xa_n && at < kMax; ++k) idx[at++] = (uint32_t)(M[mr].xa_off + k);
    }
    __syncthreads();
    bitonic(idx, PK, [&](uint32_t a, uint32_t b) { return a != kSentinel && (b == kSentinel || key_less(keys[a], keys[b])); });
    if (t == 0) {
        const int64_t at_major = major_key_of_sorted(keys, idx, n_keys);
        n_obs[l] = total;
        major[l] = major_pos;
        if (at_major >= 0) major_key[l] = keys[idx[at_major]];
        have_major_key[l] = at_major >= 0 ? 1u : 0u;
        lstatus[l] = 0;
    }
}

__global__ __launch_bounds__(kLocusThreads) void frag_gather_kernel(const Member* __restrict__ M, const AltKey* __restrict__ keys, const vlr_fragpileup_obs* __restrict__ tmp,
                                                                    const uint32_t* __restrict__ pair_left, const uint32_t* __restrict__ pair_right,
                                                                    const uint16_t* __restrict__ rank, const uint64_t* __restrict__ locus_off,
                                                                    const uint32_t* __restrict__ locus_cnt, const uint32_t* __restrict__ n_obs, const uint64_t* __restrict__ obs_off,
                                                                    const uint32_t* __restrict__ major, const AltKey* __restrict__ major_key,
                                                                    const uint32_t* __restrict__ have_major_key, uint64_t out_cap, vlr_fragpileup_obs* __restrict__ out) {
    const uint32_t l = blockIdx.x;
    const uint32_t n = locus_cnt[l];
    if (n == 0 || n > kMax || n_obs[l] == 0) return;
    const uint64_t base = locus_off[l], at = obs_off[l];
    const uint32_t mj = major[l];
    const bool have = have_major_key[l] != 0;
    const AltKey mk = major_key[l];
    for (uint32_t i = threadIdx.x; i < n; i += kLocusThreads) {
        const uint16_t r = rank[base + i];
        if (r == kNoRank || (uint32_t)r >= n_obs[l] || at + r >= out_cap) continue;
        vlr_fragpileup_obs o = tmp[base + i];
        // ReadObservation::process: Major where the observation has a read position equal to the major one
        if (mj != VLR_BASEPILEUP_NO_READ_POSITION && o.status == 0 && o.read_position == mj) o.bits |= VLR_FRAGPILEUP_READPOS_MAJOR;
        const uint32_t mr = pair_right[base + i];
        o.alt_locus = alt_locus_class(keys, M[pair_left[base + i]], mr != kSentinel ? &M[mr] : nullptr, have, mk);
        out[at + r] = o;
    }
}

}  // namespace vlr_fp

struct vlr_fragpileup : vlr_bam::Session {
    int realign = 0;
    int64_t n_loci = 0;
    int64_t win = 0;
    uint32_t max_mapq = 0;
    uint64_t member_cap = 0, name_cap = 0, key_cap = 0, coeff = 1;
    // device state (the record arrays of the base: [K_N][rec_cap] u32 counts and their offsets; d_total[K_N])
    vlr_bp::DeviceLoci dl;
    vlr_fp::Member* d_members = nullptr;
    uint8_t* d_names = nullptr;
    vlr_fp::AltKey *d_keys = nullptr, *d_major_key = nullptr;
    uint32_t* d_have_key = nullptr;
    uint32_t *d_lcnt = nullptr, *d_cursor = nullptr, *d_nobs = nullptr, *d_major = nullptr, *d_lstatus = nullptr;
    uint64_t *d_loff = nullptr, *d_obsoff = nullptr;
    // host state
    uint64_t n_members = 0, n_name_bytes = 0, n_keys = 0;
    std::vector<vlr_fragpileup_obs> obs;
    std::vector<vlr_fragpileup_locus> locus_rec;
    int64_t n_too_deep = 0;
    double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace vlr_fp {
using vlr_bam::bfail;
using vlr_bam::guard_intact;
using vlr_bam::guarded;
using vlr_bam::now_s;
using vlr_bam::zeros;

int run_chunk(vlr_fragpileup* s, vlr_dev_file* df, int64_t n, hipStream_t st) {
    const uint8_t* d_base; const uint64_t* d_starts;
    int rc = vlr_dev_file_split_view(df, &d_base, &d_starts);
    if (rc != VLR_OK || (rc = vlr_bam::reserve_records<uint32_t>(*s, n, K_N, st)) != VLR_OK) return rc;
    const double t0 = now_s();
    const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
    const uint64_t rec0 = s->n_records;
    const size_t stride = s->rec_cap;
    uint32_t *d_cnt = (uint32_t*)s->d_cnt, *d_nbytes = d_cnt + K_NAME * stride, *d_nxa = d_cnt + K_XA * stride;
    hipLaunchKernelGGL(frag_count_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->realign, s->win, s->coeff, d_cnt, d_nbytes,
                       d_nxa, s->d_counters);
    uint64_t total[K_N] = {0, 0, 0};
    if ((rc = vlr_bam::scan_records<uint32_t>(*s, n, K_N, total, st)) != VLR_OK) return rc;
    // once a buffer has overflowed nothing more is written: the session only counts on
    const bool fits = s->n_members <= s->member_cap && s->n_name_bytes <= s->name_cap && s->n_keys <= s->key_cap;
    if (total[K_MEMBERS] && fits && s->n_members < s->member_cap) {
        hipLaunchKernelGGL(frag_fill_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->realign, s->win, s->coeff, d_cnt, d_nbytes,
                           s->d_off, s->d_off + K_NAME * stride, s->d_off + K_XA * stride, s->n_members, s->member_cap, s->n_name_bytes, s->name_cap, s->n_keys, s->key_cap,
                           s->d_members, s->d_names, s->d_keys, s->d_lcnt);
        VLR_HIP_OK(hipStreamSynchronize(st));
        VLR_HIP_OK(hipGetLastError());
    }
    s->n_members += total[K_MEMBERS];
    s->n_name_bytes += total[K_NAME];
    s->n_keys += total[K_XA];
    s->n_records += (uint64_t)n;
    s->t[3] += now_s() - t0;
    return VLR_OK;
}


int fragment_pass(vlr_fragpileup* s) {
    const size_t nm = (size_t)s->n_members, nl = (size_t)s->n_loci;
    uint32_t *d_perm = nullptr, *d_left = nullptr, *d_right = nullptr; uint16_t* d_rank = nullptr; vlr_fragpileup_obs *d_tmp = nullptr, *d_out = nullptr;
    int rc = VLR_OK;
    auto step = [&](int r) { if (rc == VLR_OK) rc = r; };
    step(guarded(d_perm, nm));
    step(guarded(d_rank, nm));
    step(guarded(d_left, nm));
    step(guarded(d_right, nm));
    step(guarded(d_tmp, nm));
    auto body = [&]() -> int {
        uint64_t total_obs = 0;
        hipLaunchKernelGGL(vlr_bam::scan_kernel<uint32_t>, dim3(1), dim3(kScanThreads), 0, 0, s->d_lcnt, (int64_t)nl, (int64_t)0, s->d_loff, s->d_total);
        hipLaunchKernelGGL(frag_scatter_kernel, dim3((unsigned)((nm + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, s->d_members, (uint64_t)nm, s->n_loci, s->d_loff,
                           s->d_lcnt, s->d_cursor, d_perm);
        hipLaunchKernelGGL(frag_locus_kernel, dim3((unsigned)nl), dim3(kLocusThreads), 0, 0, s->d_members, s->d_names, s->d_keys, d_perm, s->d_loff, s->d_lcnt, s->max_mapq,
                           d_tmp, d_left, d_right, d_rank, s->d_nobs, s->d_major, s->d_major_key, s->d_have_key, s->d_lstatus);
        hipLaunchKernelGGL(vlr_bam::scan_kernel<uint32_t>, dim3(1), dim3(kScanThreads), 0, 0, s->d_nobs, (int64_t)nl, (int64_t)0, s->d_obsoff, s->d_total + 1);
        VLR_HIP_OK(hipDeviceSynchronize());
        VLR_HIP_OK(hipGetLastError());
        VLR_HIP_OK(hipMemcpy(&total_obs, s->d_total + 1, 8, hipMemcpyDeviceToHost));
        if (total_obs > nm) return bfail(VLR_ERR_HIP, "vlr_fragpileup_result: more observations than members");
        // the output is sized by the observations, not by the members
        int r = guarded(d_out, (size_t)total_obs);
        if (r != VLR_OK) return r;
        hipLaunchKernelGGL(frag_gather_kernel, dim3((unsigned)nl), dim3(kLocusThreads), 0, 0, s->d_members, s->d_keys, d_tmp, d_left, d_right, d_rank, s->d_loff, s->d_lcnt,
                           s->d_nobs, s->d_obsoff, s->d_major, s->d_major_key, s->d_have_key, total_obs, d_out);
        VLR_HIP_OK(hipDeviceSynchronize());
        VLR_HIP_OK(hipGetLastError());
        bool ok = true;
        r = guard_intact(d_perm, nm, &ok);
        if (r == VLR_OK) r = guard_intact(d_rank, nm, &ok);
        if (r == VLR_OK) r = guard_intact(d_left, nm, &ok);
        if (r == VLR_OK) r = guard_intact(d_right, nm, &ok);
        if (r == VLR_OK) r = guard_intact(d_tmp, nm, &ok);
        if (r == VLR_OK) r = guard_intact(d_out, (size_t)total_obs, &ok);
        if (r != VLR_OK) return r;
        if (!ok) s->status |= VLR_FRAGPILEUP_GUARD_DAMAGED;
        const double t1 = now_s();
        s->obs.resize((size_t)total_obs);
        if (total_obs) VLR_HIP_OK(hipMemcpy(s->obs.data(), d_out, (size_t)total_obs * sizeof(vlr_fragpileup_obs), hipMemcpyDeviceToHost));
        std::vector<uint32_t> lcnt(nl), nobs(nl), major(nl), lst(nl);
        std::vector<uint64_t> ooff(nl);
        VLR_HIP_OK(hipMemcpy(lcnt.data(), s->d_lcnt, nl * 4, hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(nobs.data(), s->d_nobs, nl * 4, hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(major.data(), s->d_major, nl * 4, hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(lst.data(), s->d_lstatus, nl * 4, hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(ooff.data(), s->d_obsoff, nl * 8, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < nl; ++k) {
            s->locus_rec[k] = vlr_fragpileup_locus{(int64_t)ooff[k], lcnt[k], nobs[k], major[k], lst[k]};
            if (lst[k]) ++s->n_too_deep;
        }
        s->t[7] += now_s() - t1;
        return VLR_OK;
    };
    if (rc == VLR_OK) rc = body();
    void* p[] = {d_perm, d_rank, d_left, d_right, d_tmp, d_out};
    for (void* q : p) if (q) (void)hipFree(q);
    return rc;
}

}  // namespace vlr_fp

extern "C" {

int vlr_fragpileup_open(int device, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int32_t* len, const uint8_t* kind,
                        const uint8_t* ref_bases, const uint8_t* alt_bases, int realign_indel_reads, int64_t window, int max_mapq, int max_read_len,
                        int64_t member_capacity, int64_t name_capacity, int64_t key_capacity, int64_t window_bytes, vlr_fragpileup** out) {
    using namespace vlr_fp;
    if (!out || n_loci < 0 || n_loci > 0x7fffffff || member_capacity < 0 || member_capacity > 0x7fffffff || name_capacity < 0 || key_capacity < 0 || key_capacity > 0x7fffffff ||
        window_bytes < 0 || window < 0 ||
        window > ((int64_t)1 << 40) || max_mapq < 0 || max_mapq > 255 || (n_loci > 0 && (!ref_id || !start || !len || !kind || !ref_bases || !alt_bases)))
        return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_open: bad argument");
    if (max_read_len <= 0) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_open: max_read_len must be positive");
    *out = nullptr;
    std::vector<uint64_t> base_off;
    int rc = vlr_bp::check_snv_mnv_loci("vlr_fragpileup_open", n_loci, ref_id, start, len, kind, base_off);
    if (rc != VLR_OK || (rc = vlr_bam::use_device(device)) != VLR_OK) return rc;
    vlr_fragpileup* s = new vlr_fragpileup();
    s->realign = realign_indel_reads ? 1 : 0;
    s->n_loci = n_loci;
    s->win = window;
    s->max_mapq = (uint32_t)max_mapq;
    s->member_cap = (uint64_t)member_capacity;
    s->name_cap = (uint64_t)name_capacity;
    s->key_cap = (uint64_t)key_capacity;
    s->coeff = 10ull * (uint64_t)max_read_len;
    s->locus_rec.assign((size_t)n_loci, vlr_fragpileup_locus{0, 0, 0, VLR_BASEPILEUP_NO_READ_POSITION, 0});
    const size_t nl = (size_t)n_loci;
    auto step = [&](int r) { if (rc == VLR_OK) rc = r; };
    step(vlr_bam::open_session(*s, device, window_bytes, K_N));
    step(s->dl.upload(n_loci, ref_id, start, len, kind, base_off, ref_bases, alt_bases));
    step(zeros(s->d_major_key, nl)); step(zeros(s->d_have_key, nl));
    step(zeros(s->d_lcnt, nl)); step(zeros(s->d_cursor, nl)); step(zeros(s->d_nobs, nl)); step(zeros(s->d_major, nl)); step(zeros(s->d_lstatus, nl));
    step(zeros(s->d_loff, nl)); step(zeros(s->d_obsoff, nl));
    step(guarded(s->d_members, (size_t)s->member_cap));
    step(guarded(s->d_names, (size_t)s->name_cap));
    step(guarded(s->d_keys, (size_t)s->key_cap));
    if (rc != VLR_OK) { vlr_fragpileup_close(s); return rc; }
    *out = s;
    return VLR_OK;
}

int vlr_fragpileup_add_bam(vlr_fragpileup* s, const char* bam_path) {
    if (!s) return vlr_bam::bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_add_bam: null");
    return vlr_bam::add_bam(*s, bam_path, "vlr_fragpileup_add_bam", {&s->t[0], &s->t[1], &s->t[2], &s->t[6], &s->t[5]}, nullptr,
                            [s](vlr_dev_file* df, int64_t n, hipStream_t st) { return vlr_fp::run_chunk(s, df, n, st); });
}

int vlr_fragpileup_result(vlr_fragpileup* s, vlr_fragpileup_counts* r) {
    using namespace vlr_fp;
    if (!s || !r) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_result: null");
    VLR_HIP_OK(hipSetDevice(s->device));
    if (!s->collected) {
        bool ok = true;
        int rc = vlr_bam::read_counters(*s);
        if (rc == VLR_OK) rc = guard_intact(s->d_members, (size_t)s->member_cap, &ok);
        if (rc == VLR_OK) rc = guard_intact(s->d_names, (size_t)s->name_cap, &ok);
        if (rc == VLR_OK) rc = guard_intact(s->d_keys, (size_t)s->key_cap, &ok);
        if (rc != VLR_OK) return rc;
        if (!ok) s->status |= VLR_FRAGPILEUP_GUARD_DAMAGED;
        if (vlr_bam::bad_record_seen(*s)) s->status |= VLR_FRAGPILEUP_BAD_RECORD;
        if (s->n_members > s->member_cap) s->status |= VLR_FRAGPILEUP_MEMBER_OVERFLOW;
        if (s->n_name_bytes > s->name_cap) s->status |= VLR_FRAGPILEUP_NAME_OVERFLOW;
        if (s->n_keys > s->key_cap) s->status |= VLR_FRAGPILEUP_KEY_OVERFLOW;
        if (!(s->status & (VLR_FRAGPILEUP_MEMBER_OVERFLOW | VLR_FRAGPILEUP_NAME_OVERFLOW | VLR_FRAGPILEUP_KEY_OVERFLOW | VLR_FRAGPILEUP_GUARD_DAMAGED)) && s->n_members && s->n_loci) {
            const double t0 = now_s();
            rc = fragment_pass(s);
            if (rc != VLR_OK) return rc;
            s->t[4] += now_s() - t0 - s->t[7];
        }
        s->collected = true;
    }
    const bool over = (s->status & (VLR_FRAGPILEUP_MEMBER_OVERFLOW | VLR_FRAGPILEUP_NAME_OVERFLOW | VLR_FRAGPILEUP_KEY_OVERFLOW)) != 0;
    r->n_obs = (int64_t)s->obs.size();
    r->n_members = over ? 0 : (int64_t)s->n_members;
    r->n_records = (int64_t)s->n_records;
    r->n_rejected = (int64_t)s->counters[C_REJECTED];
    r->n_loci_too_deep = s->n_too_deep;
    r->status = s->status;
    r->needed_members = (int64_t)s->n_members;
    r->needed_name_bytes = (int64_t)s->n_name_bytes;
    r->needed_keys = (int64_t)s->n_keys;
    r->first_bad_record = vlr_bam::first_bad_record(*s);
    for (int k = 0; k < 8; ++k) r->seconds[k] = s->t[k];
    return VLR_OK;
}

int vlr_fragpileup_read(vlr_fragpileup* s, vlr_fragpileup_obs* obs, int64_t n_obs, vlr_fragpileup_locus* loci, int64_t n_loci) {
    using namespace vlr_fp;
    if (!s || !s->collected) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_read: call vlr_fragpileup_result first");
    if (n_obs != (int64_t)s->obs.size() || n_loci != s->n_loci || (n_obs > 0 && !obs) || (n_loci > 0 && !loci))
        return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_read: sizes differ from vlr_fragpileup_result and the loci given at open");
    if (n_obs) memcpy(obs, s->obs.data(), (size_t)n_obs * sizeof(vlr_fragpileup_obs));
    if (n_loci) memcpy(loci, s->locus_rec.data(), (size_t)n_loci * sizeof(vlr_fragpileup_locus));
    return VLR_OK;
}

void vlr_fragpileup_close(vlr_fragpileup* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    vlr_bam::close_session(*s);
    s->dl.free();
    void* p[] = {s->d_members, s->d_names, s->d_keys, s->d_major_key, s->d_have_key, s->d_lcnt, s->d_cursor, s->d_nobs, s->d_major, s->d_lstatus, s->d_loff, s->d_obsoff};
    for (void* q : p) if (q) (void)hipFree(q);
    delete s;
}

}  // extern "C"

