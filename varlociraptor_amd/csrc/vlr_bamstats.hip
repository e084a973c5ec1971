// vlr_bamstats.hip — the per-record pass of `estimate alignment-properties` (estimation/alignment_properties.rs:148-463, cigar_stats
// :693-861) for gfx950, and its host driver (vlr_bamstats_*, include/vlr.h).
//
// Streaming: each BAM goes through the device front door of the observation reader — the BGZF member index (here, from the file read
// in bounded pieces), the inflate kernel behind vlr_dev_file_feed, the header skipped, the BAM record split (vlr_dev_file_split_bam:
// the BCF split's anchor / verified walk / serial fallback over the 32-byte BAM head) and vlr_dev_file_consume.  Device memory is the
// reader's window (about kWindow inflated bytes, more only for one record longer than that), the per-chunk record arrays, the contigs
// the taken records lie on and the fixed-size counters.
//
// Per chunk of split records three kernels run:
//   bam_take_kernel   one lane per record: the fixed head checked against block_size; the skip rule (:286-292) -> take[i]
//                     (0 skipped, 1 taken, 2 malformed: counts as taken, so that the cap decides whether the reference would reach it)
//   bam_select_kernel one workgroup: exclusive prefix sum of the taken flags -> the record index the cap (--num-records) applies to;
//                     sel[i] = 1 for the analysed records, the skipped records in front of the cap counted, the contigs used marked
//   bam_stats_kernel  one wave per analysed record (grid-stride): lane 0 walks the CIGAR and the indels serially, the lanes of the wave
//                     take the bases of an M/=/X operation side by side (transitions of neighbouring reference bases, (rbase, qbase)
//                     runs); maxima, flag counters and one insert size per record
// Integer counts only: the 16 x 16 transition counts (u64) and the dense hop counters (u32: raw base in ACGTacgt, both keys < 32) in
// LDS, flushed with 64-bit atomics; other hop keys go to an exact global hash table (64-bit CAS / add).  Sums of integers in any
// order: the results do not depend on the launch geometry or on how records fall into chunks.
//
// Bounds: every access of a record stays inside [start, start + 4 + block_size) (head checked by the take kernel, aux walked with
// its lengths checked), every reference access inside the contig; a CIGAR that runs past its contig or its read, a malformed record,
// a reference id out of range or a hop key past 2^28 come back as an error naming the file and the record.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <zlib.h>

#include "vlr_bamsession.h"

extern "C" void vlr_set_error(const char* msg);  // vlr_host.cpp: the text behind vlr_last_error()

namespace vlr_bam {

constexpr int kWaves = 4;                   // waves per workgroup of the stats kernel
constexpr int kThreads = 64 * kWaves;
constexpr int kDenseK = 32;                 // hop keys k0, k1 below this with a base in ACGTacgt: dense LDS counters
constexpr int kDense = 8 * kDenseK * kDenseK;
constexpr uint32_t kHashSlots = 1u << 20;   // exact spill of the other hop keys
constexpr uint64_t kEmpty = ~0ull;
constexpr uint32_t kKeyMax = (1u << 28) - 1;
constexpr size_t kWindow = (size_t)64 << 20;      // inflated bytes fed per split
constexpr uint64_t kSplitRecords = 1u << 18;     // records per split at most
constexpr size_t kReadPiece = (size_t)32 << 20;   // compressed bytes read from the file at a time

enum Err : uint32_t { E_MALFORMED = 1, E_CIGAR_RANGE = 2, E_TID = 4, E_KEY = 8, E_HASH_FULL = 16 };
// misc counters (u64, global): maxima are kept as value + 1 (0 = none)
enum Misc { M_MAX_DEL, M_MAX_INS, M_FRAC, M_READ_LEN, M_MAPQ, M_NOT_USABLE, M_SOFT, M_NOT_PAIRED, M_NOT_FIRST, M_MATE_UNMAPPED, M_TID_MISMATCH,
            M_ERR_CODE, M_ERR_REC, M_N };

__device__ __forceinline__ uint32_t ld16(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint32_t upper(uint32_t c) { return (c >= 97 && c <= 122) ? c - 32 : c; }
__device__ __forceinline__ int st_match(uint32_t c) {
    c = upper(c);
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 14;
}
__device__ __forceinline__ int st_hop(uint32_t c, int y) { const int m = st_match(c); return m == 14 ? 14 : 6 + 2 * m + y; }
__device__ __forceinline__ uint32_t qbase(const uint8_t* seq, uint32_t i) {
    const uint32_t b = seq[i >> 1];
    return (uint32_t)"=ACMGRSVTWYHKDBN"[(i & 1) ? (b & 15u) : (b >> 4)];
}
__device__ __forceinline__ int dense_slot(uint32_t base) {
    switch (base) {
        case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3;
        case 'a': return 4; case 'c': return 5; case 'g': return 6; case 't': return 7;
        default: return -1;
    }
}
__device__ __forceinline__ void fail(uint64_t* misc, uint32_t code, uint64_t rec) {
    atomicOr((unsigned long long*)&misc[M_ERR_CODE], (unsigned long long)code);
    atomicMin((unsigned long long*)&misc[M_ERR_REC], (unsigned long long)rec);
}

struct Sink {
    unsigned long long* trans;   // LDS [256]
    uint32_t* dense;             // LDS [kDense]
    uint64_t* hkeys;
    uint64_t* hvals;
    uint64_t* misc;
};

__device__ void hop(const Sink& s, uint32_t base, uint64_t k0, uint64_t k1, uint64_t rec) {
    const int slot = dense_slot(base);
    if (slot >= 0 && k0 < (uint64_t)kDenseK && k1 < (uint64_t)kDenseK) {
        atomicAdd(&s.dense[(slot * kDenseK + (int)k0) * kDenseK + (int)k1], 1u);
        return;
    }
    if (k0 >= kKeyMax || k1 >= kKeyMax) { fail(s.misc, E_KEY, rec); return; }
    const uint64_t key = ((uint64_t)(base & 0xffu) << 56) | (k0 << 28) | k1;
    uint64_t h = key * 0x9E3779B97F4A7C15ull;
    uint32_t i = (uint32_t)(h >> 40) & (kHashSlots - 1);
    for (uint32_t probe = 0; probe < kHashSlots; ++probe) {
        const unsigned long long prev = atomicCAS((unsigned long long*)&s.hkeys[i], (unsigned long long)kEmpty, (unsigned long long)key);
        if (prev == kEmpty || prev == key) { atomicAdd((unsigned long long*)&s.hvals[i], 1ull); return; }
        i = (i + 1) & (kHashSlots - 1);
    }
    fail(s.misc, E_HASH_FULL, rec);
}
__device__ __forceinline__ void tr(const Sink& s, int a, int b, uint64_t v) { if (v) atomicAdd(&s.trans[a * 16 + b], (unsigned long long)v); }

// one lane per record of the chunk
__global__ void bam_take_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint8_t* __restrict__ take) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = starts[i], end = starts[i + 1];
    const uint8_t* p = base + o;
    uint8_t t = 2;
    if (end - o >= 36) {
        const uint32_t bs = ld32(p);
        const uint32_t l_rn = p[12], mapq = p[13], n_cig = ld16(p + 16), flag = ld16(p + 18);
        const int32_t l_seq = (int32_t)ld32(p + 20);
        if ((uint64_t)bs + 4 == end - o && l_seq >= 0 && l_rn >= 1 &&
            32ull + l_rn + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq <= bs)
            t = (mapq == 0 || (flag & 0x400u) || (flag & 0x200u) || (flag & 0x4u) || l_seq == 0) ? 0 : 1;
    }
    take[i] = t;
}

// one workgroup of 1024: sel[i] = take[i] for the records the reference reaches before its cap, 0 behind; out[0] += analysed,
// out[1] += skipped in front of the cap; used[tid] = 1 for the analysed records' contigs; the first malformed one reached -> misc
constexpr int kSelThreads = 1024;
__global__ __launch_bounds__(kSelThreads) void bam_select_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n,
                                                                 const uint8_t* __restrict__ take, uint64_t remaining, int n_refs, uint64_t rec0,
                                                                 uint8_t* __restrict__ sel, uint8_t* __restrict__ used, uint64_t* __restrict__ out,
                                                                 uint64_t* __restrict__ misc) {
    __shared__ uint64_t part[kSelThreads];
    const int t = (int)threadIdx.x;
    const int64_t per = (n + kSelThreads - 1) / kSelThreads;
    const int64_t a = (int64_t)t * per, b = a + per < n ? a + per : n;
    uint64_t c = 0;
    for (int64_t i = a; i < b; ++i) c += take[i] != 0;
    part[t] = c;
    __syncthreads();
    for (int off = 1; off < kSelThreads; off <<= 1) {   // inclusive scan (Hillis-Steele)
        const uint64_t v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t idx = part[t] - c;   // taken records in front of this thread's range
    uint64_t n_sel = 0, n_skip = 0;
    for (int64_t i = a; i < b; ++i) {
        const uint8_t k = take[i];
        const bool reached = idx < remaining;
        uint8_t s = 0;
        if (k == 0) {
            n_skip += reached;
        } else {
            if (reached) {
                if (k == 2) {
                    fail(misc, E_MALFORMED, rec0 + (uint64_t)i);
                } else {
                    const int32_t tid = (int32_t)ld32(base + starts[i] + 4);
                    if (tid < 0 || tid >= n_refs) fail(misc, E_TID, rec0 + (uint64_t)i);
                    else { used[tid] = 1; s = 1; }
                }
                n_sel += 1;
            }
            idx += 1;
        }
        sel[i] = s;
    }
    if (n_sel) atomicAdd((unsigned long long*)&out[0], (unsigned long long)n_sel);
    if (n_skip) atomicAdd((unsigned long long*)&out[1], (unsigned long long)n_skip);
}

// EF aux tag (utils/mod.rs:61-71): the first EF of an integer type equals 1; the walk stops at the first field that does not fit
__device__ bool aux_ef(const uint8_t* p, uint64_t q, uint64_t end) {
    while (q + 3 <= end) {
        const uint32_t t0 = p[q], t1 = p[q + 1], ty = p[q + 2];
        uint64_t v = q + 3, len;
        if (ty == 'A' || ty == 'c' || ty == 'C') len = 1;
        else if (ty == 's' || ty == 'S') len = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') len = 4;
        else if (ty == 'Z' || ty == 'H') {
            uint64_t z = v;
            while (z < end && p[z] != 0) ++z;
            if (z >= end) return false;
            len = z + 1 - v;
        } else if (ty == 'B') {
            if (v + 5 > end) return false;
            const uint32_t sub = p[v];
            const uint64_t cnt = ld32(p + v + 1);
            const uint64_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
            if (es == 0) return false;
            len = 5 + cnt * es;
        } else {
            return false;
        }
        if (v + len > end) return false;
        if (t0 == 'E' && t1 == 'F') {
            int64_t x;
            if (ty == 'c') x = (int8_t)p[v];
            else if (ty == 'C') x = p[v];
            else if (ty == 's') x = (int16_t)ld16(p + v);
            else if (ty == 'S') x = ld16(p + v);
            else if (ty == 'i') x = (int32_t)ld32(p + v);
            else if (ty == 'I') x = ld32(p + v);
            else return false;
            return x == 1;
        }
        q = v + len;
    }
    return false;
}

__global__ __launch_bounds__(kThreads) void bam_stats_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n,
                                                            const uint8_t* __restrict__ sel, const uint8_t* const* __restrict__ ctg,
                                                            const uint64_t* __restrict__ ctg_len, uint64_t rec0, uint64_t* __restrict__ g_trans,
                                                            uint64_t* __restrict__ g_dense, uint64_t* __restrict__ hkeys, uint64_t* __restrict__ hvals,
                                                            uint64_t* __restrict__ misc, int64_t* __restrict__ tlen_out) {
    __shared__ unsigned long long s_trans[256];
    __shared__ uint32_t s_dense[kDense];
    __shared__ unsigned long long s_misc[M_ERR_CODE];
    for (int k = (int)threadIdx.x; k < 256; k += kThreads) s_trans[k] = 0;
    for (int k = (int)threadIdx.x; k < kDense; k += kThreads) s_dense[k] = 0;
    for (int k = (int)threadIdx.x; k < M_ERR_CODE; k += kThreads) s_misc[k] = 0;
    __syncthreads();
    const Sink S{s_trans, s_dense, hkeys, hvals, misc};
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave0 = (int64_t)blockIdx.x * kWaves + (int64_t)(threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * kWaves;
    for (int64_t r = wave0; r < n; r += n_waves) {
        if (lane == 0) tlen_out[r] = -1;
        if (sel[r] != 1) continue;
        const uint64_t rec = rec0 + (uint64_t)r;
        const uint8_t* p = base + starts[r];
        const uint64_t end = 4 + (uint64_t)ld32(p);                  // record bytes [0, end) (checked by the take kernel)
        const int32_t tid = (int32_t)ld32(p + 4);
        const int64_t pos = (int32_t)ld32(p + 8);
        const uint32_t l_rn = p[12], mapq = p[13], n_cig = ld16(p + 16), flag = ld16(p + 18);
        const uint64_t l_seq = ld32(p + 20);
        const int32_t mtid = (int32_t)ld32(p + 24), tlen = (int32_t)ld32(p + 32);
        const uint8_t* cig = p + 36 + l_rn;
        const uint8_t* seq = cig + 4 * (uint64_t)n_cig;
        const uint64_t aux0 = 36 + l_rn + 4 * (uint64_t)n_cig + (l_seq + 1) / 2 + l_seq;
        const uint8_t* ref = ctg[tid];
        const uint64_t L = ctg_len[tid];
        bool bad = pos < 0;
        uint64_t rpos = pos < 0 ? 0 : (uint64_t)pos, qpos = 0;
        bool irregular = false, soft = false, malformed = false;
        uint64_t max_del = 0, max_ins = 0, fbits = 0;   // value + 1
        for (uint32_t j = 0; j < n_cig && !bad && !malformed; ++j) {
            const uint32_t v = ld32(cig + 4 * j);
            const uint32_t op = v & 15u;
            const uint64_t l = v >> 4;
            if (op > 8) { if (lane == 0) fail(misc, E_MALFORMED, rec); malformed = true; break; }
            if (op == 2) {                                                     // D (:730-786)
                max_del = max_del > l + 1 ? max_del : l + 1;
                irregular = true;
                if (l < 32767) {
                    if (l == 0 || rpos + l > L) { bad = true; break; }
                    if (lane == 0) {
                        const uint32_t b = ref[rpos], bu = upper(b);
                        bool hom = true;
                        for (uint64_t k = 1; k < l && hom; ++k) hom = upper(ref[rpos + k]) == bu;
                        if (hom) {
                            uint64_t len = l;
                            for (uint64_t k = rpos + l; k < L && upper(ref[k]) == bu; ++k) ++len;
                            if (rpos > 1)                                          // ref[..rpos - 1] reversed: base rpos - 1 skipped
                                for (uint64_t k = rpos - 1; k-- > 0 && upper(ref[k]) == bu;) ++len;
                            if (len >= 2) {
                                const int ms = st_match(b), hs = st_hop(b, 0);
                                tr(S, ms, ms, l);
                                tr(S, ms, hs, 1);
                                const uint64_t lm2 = l >= 2 ? l - 2 : 0;
                                tr(S, hs, hs, len >= lm2 ? len - lm2 : 0);
                                if (rpos + len + 1 < L) tr(S, hs, st_match(ref[rpos + len + 1]), 1);
                                hop(S, b, len, len - l, rec);
                            }
                        }
                        if (!hom || l == 1) {
                            tr(S, st_match(b), 4, 1);
                            tr(S, 4, 4, l >= 2 ? l - 2 : 0);
                            if (rpos + l + 1 < L) tr(S, 4, st_match(ref[rpos + l + 1]), 1);
                        }
                    }
                }
                rpos += l;
            } else if (op == 1) {                                              // I (:787-834)
                max_ins = max_ins > l + 1 ? max_ins : l + 1;
                irregular = true;
                if (l < 32767) {
                    if (rpos >= L || qpos + (l > 0 ? l : 1) > l_seq) { bad = true; break; }
                    if (lane == 0) {
                        const uint32_t q0 = qbase(seq, (uint32_t)qpos), q0u = upper(q0);
                        const uint32_t b = upper(ref[rpos]) == q0 ? ref[rpos] : q0;
                        bool hom = true;
                        for (uint64_t k = 1; k < l && hom; ++k) hom = upper(qbase(seq, (uint32_t)(qpos + k))) == q0u;
                        if (hom) {
                            uint64_t len = l;
                            for (uint64_t k = rpos; k < L && upper(ref[k]) == q0u; ++k) ++len;
                            if (rpos > 0)
                                for (uint64_t k = rpos; k-- > 0 && upper(ref[k]) == q0u;) ++len;
                            if (len >= 2) {
                                const int ms = st_match(b), hs = st_hop(b, 1);
                                tr(S, ms, ms, l);
                                tr(S, ms, hs, 1);
                                const uint64_t lm2 = l >= 2 ? l - 2 : 0;
                                tr(S, hs, hs, len >= lm2 ? len - lm2 : 0);
                                if (rpos + 1 < L) tr(S, hs, st_match(ref[rpos + 1]), 1);
                                hop(S, b, len - l, l, rec);
                            }
                        }
                        if (!hom || l == 1) {
                            tr(S, st_match(b), 5, 1);
                            tr(S, 5, 5, l >= 2 ? l - 2 : 0);
                            if (rpos + l + 1 < L) tr(S, 5, st_match(ref[rpos + l + 1]), 1);
                        }
                    }
                }
                qpos += l;
            } else if (op == 0 || op == 7 || op == 8) {                        // M = X (:835-859): the wave takes the bases
                if (rpos + l > L || qpos + l > l_seq) { bad = true; break; }
                const uint8_t* rr = ref + rpos;
                for (uint64_t k = (uint64_t)lane; k < l; k += 64) {
                    const uint32_t rb = rr[k], qb = qbase(seq, (uint32_t)(qpos + k));
                    if (k + 1 < l) tr(S, st_match(rb), st_match(rr[k + 1]), 1);
                    // a run of equal raw (rbase, qbase) pairs starts here: its first lane measures it
                    if (k == 0 || rr[k - 1] != rb || qbase(seq, (uint32_t)(qpos + k - 1)) != qb) {
                        uint64_t e = k + 1;
                        while (e < l && rr[e] == rb && qbase(seq, (uint32_t)(qpos + e)) == qb) ++e;
                        if (upper(rb) == qb && e - k >= 2) hop(S, rb, e - k, e - k, rec);
                    }
                }
                qpos += l;
                rpos += l;
            } else if (op == 4) {                                              // S
                const double s = (double)l / (double)l_seq;
                uint64_t b;
                __builtin_memcpy(&b, &s, 8);
                fbits = fbits > b + 1 ? fbits : b + 1;
                irregular = soft = true;
                qpos += l;
            } else if (op == 3) {                                              // N
                rpos += l;
            } else if (op == 5) {                                              // H: irregular (omit_insert_size = false)
                irregular = true;
            }
        }
        if (malformed) continue;
        if (bad) { if (lane == 0) fail(misc, E_CIGAR_RANGE, rec); continue; }
        if (lane == 0) {
            if (max_del) atomicMax(&s_misc[M_MAX_DEL], (unsigned long long)max_del);
            if (max_ins) atomicMax(&s_misc[M_MAX_INS], (unsigned long long)max_ins);
            if (fbits) atomicMax(&s_misc[M_FRAC], (unsigned long long)fbits);
            atomicMax(&s_misc[M_READ_LEN], (unsigned long long)l_seq + 1);
            atomicMax(&s_misc[M_MAPQ], (unsigned long long)mapq + 1);
            if (irregular) atomicAdd(&s_misc[M_NOT_USABLE], 1ull);
            if (soft) atomicAdd(&s_misc[M_SOFT], 1ull);
            if (!(flag & 0x1u)) atomicAdd(&s_misc[M_NOT_PAIRED], 1ull);
            if (!(flag & 0x40u)) atomicAdd(&s_misc[M_NOT_FIRST], 1ull);
            if (flag & 0x8u) atomicAdd(&s_misc[M_MATE_UNMAPPED], 1ull);
            if (tid != mtid) atomicAdd(&s_misc[M_TID_MISMATCH], 1ull);
            int64_t isz = -1;
            if (!irregular) {
                if (flag & 0x1u) {
                    if ((flag & 0x40u) && tid == mtid && !(flag & 0x8u)) isz = tlen < 0 ? -(int64_t)tlen : (int64_t)tlen;
                } else if (aux_ef(p, aux0, end)) {
                    isz = (int64_t)rpos - pos;
                }
            }
            tlen_out[r] = isz;
        }
    }
    __syncthreads();
    for (int k = (int)threadIdx.x; k < 256; k += kThreads)
        if (s_trans[k]) atomicAdd((unsigned long long*)&g_trans[k], s_trans[k]);
    for (int k = (int)threadIdx.x; k < kDense; k += kThreads)
        if (s_dense[k]) atomicAdd((unsigned long long*)&g_dense[k], (unsigned long long)s_dense[k]);
    for (int k = (int)threadIdx.x; k < M_ERR_CODE; k += kThreads) {
        if (!s_misc[k]) continue;
        if (k <= M_MAPQ) atomicMax((unsigned long long*)&misc[k], s_misc[k]);
        else atomicAdd((unsigned long long*)&misc[k], s_misc[k]);
    }
}

int bfail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    vlr_set_error(buf);
    return code;
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace vlr_bam

struct vlr_bamstats {
    int device = 0;
    std::string fasta;
    vlr_bam::Fai fai;
    int64_t cap = 0;             // records to analyse in all (--num-records or the default count)
    size_t window = vlr_bam::kWindow;
    uint64_t n_taken = 0, n_skipped = 0;
    // device state
    uint64_t *d_trans = nullptr, *d_dense = nullptr, *d_hkeys = nullptr, *d_hvals = nullptr, *d_misc = nullptr, *d_out = nullptr;
    uint8_t *d_take = nullptr, *d_sel = nullptr, *d_used = nullptr;
    int64_t* d_tlen = nullptr;
    size_t rec_cap = 0, used_cap = 0;
    const uint8_t** d_ctg = nullptr; uint64_t* d_ctg_len = nullptr; size_t ctg_cap = 0;
    vlr_bam::Contigs contigs;   // uploaded contigs by name
    std::vector<int64_t> tlens;
    std::vector<uint64_t> hop_keys, hop_vals;
    bool collected = false;
    double t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

namespace vlr_bam {

int read_fai(const std::string& fasta, Fai& fai) {
    const std::string path = fasta + ".fai";
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: no .fai index (index the reference with samtools faidx)", fasta.c_str());
    char line[4096];
    while (fgets(line, sizeof line, f)) {
        char name[2048];
        unsigned long long a, b, c, d;
        if (sscanf(line, "%2047[^\t]\t%llu\t%llu\t%llu\t%llu", name, &a, &b, &c, &d) == 5 && c > 0 && d >= c) fai[name] = {a, b, c, d};
    }
    fclose(f);
    return VLR_OK;
}

// the bases of one contig through the .fai, on the device (see vlr_bamstream.h)
int load_contig(const std::string& fasta, const Fai& fai, Contigs& cache, const std::string& name, const char* bam, bool upper_case, std::pair<uint8_t*, uint64_t>& out) {
    auto it = cache.find(name);
    if (it != cache.end()) { out = it->second; return VLR_OK; }
    auto e = fai.find(name);
    if (e == fai.end()) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: contig %s (of %s) is missing from the reference", fasta.c_str(), name.c_str(), bam);
    const FaiEntry& x = e->second;
    std::vector<uint8_t> seq(x.len);
    if (x.len) {
        const uint64_t nlines = (x.len - 1) / x.lb + 1;
        const uint64_t raw_n = (nlines - 1) * x.lw + (x.len - (nlines - 1) * x.lb);
        std::vector<uint8_t> raw(raw_n);
        FILE* f = fopen(fasta.c_str(), "rb");
        if (!f) return bfail(VLR_ERR_INVALID_ARGUMENT, "cannot open %s", fasta.c_str());
        const bool ok = fseeko(f, (off_t)x.off, SEEK_SET) == 0 && fread(raw.data(), 1, raw_n, f) == raw_n;
        fclose(f);
        if (!ok) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: contig %s shorter than its .fai entry", fasta.c_str(), name.c_str());
        for (uint64_t l = 0, k = 0; l < nlines; ++l) {
            const uint64_t m = std::min<uint64_t>(x.lb, x.len - k);
            memcpy(seq.data() + k, raw.data() + l * x.lw, m);
            k += m;
        }
        if (upper_case) for (auto& c : seq) if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
    }
    uint8_t* d = nullptr;
    VLR_HIP_OK(hipMalloc(&d, x.len + 1));
    if (x.len) VLR_HIP_OK(hipMemcpy(d, seq.data(), x.len, hipMemcpyHostToDevice));
    out = cache[name] = {d, x.len};
    return VLR_OK;
}

struct Member { uint64_t off, clen; uint32_t isize, crc; };

// BGZF members of buf[0, n) that are complete; *used = bytes they cover (SAM spec 4.1).  false: not BGZF
bool index_members(const uint8_t* b, size_t n, std::vector<Member>& out, size_t* used) {
    size_t p = 0;
    while (p + 18 <= n) {
        if (b[p] != 0x1f || b[p + 1] != 0x8b || b[p + 2] != 8 || !(b[p + 3] & 4)) return false;
        const size_t xlen = b[p + 10] | (b[p + 11] << 8);
        size_t q = p + 12;
        const size_t xend = q + xlen;
        if (xend > n) break;
        long bsize = -1;
        while (q + 4 <= xend) {
            const size_t slen = b[q + 2] | (b[q + 3] << 8);
            if (b[q] == 'B' && b[q + 1] == 'C' && slen == 2 && q + 6 <= xend) bsize = (b[q + 4] | (b[q + 5] << 8)) + 1;
            q += 4 + slen;
        }
        if (bsize < 0 || (size_t)bsize < xlen + 20) return false;
        if (p + (size_t)bsize > n) break;
        const size_t cend = p + (size_t)bsize - 8;
        Member m;
        m.off = xend; m.clen = cend - xend;
        m.crc = b[cend] | (b[cend + 1] << 8) | (b[cend + 2] << 16) | ((uint32_t)b[cend + 3] << 24);
        m.isize = b[cend + 4] | (b[cend + 5] << 8) | (b[cend + 6] << 16) | ((uint32_t)b[cend + 7] << 24);
        if (m.isize > 65536) return false;
        out.push_back(m);
        p += (size_t)bsize;
    }
    *used = p;
    return true;
}

int alloc_state(vlr_bamstats* s) {
    VLR_HIP_OK(hipMalloc(&s->d_trans, 256 * 8));
    VLR_HIP_OK(hipMalloc(&s->d_dense, kDense * 8));
    VLR_HIP_OK(hipMalloc(&s->d_hkeys, (size_t)kHashSlots * 8));
    VLR_HIP_OK(hipMalloc(&s->d_hvals, (size_t)kHashSlots * 8));
    VLR_HIP_OK(hipMalloc(&s->d_misc, M_N * 8));
    VLR_HIP_OK(hipMalloc(&s->d_out, 2 * 8));
    VLR_HIP_OK(hipMemset(s->d_trans, 0, 256 * 8));
    VLR_HIP_OK(hipMemset(s->d_dense, 0, kDense * 8));
    VLR_HIP_OK(hipMemset(s->d_hkeys, 0xff, (size_t)kHashSlots * 8));
    VLR_HIP_OK(hipMemset(s->d_hvals, 0, (size_t)kHashSlots * 8));
    VLR_HIP_OK(hipMemset(s->d_misc, 0, M_N * 8));
    const uint64_t none = ~0ull;
    VLR_HIP_OK(hipMemcpy(s->d_misc + M_ERR_REC, &none, 8, hipMemcpyHostToDevice));
    return VLR_OK;
}

// one chunk of split records: take, select (the cap), contigs, statistics; insert sizes back to the host
int run_chunk(vlr_bamstats* s, vlr_dev_file* df, int64_t n, uint64_t rec0, const std::vector<std::string>& names, const char* path, hipStream_t st) {
    const uint8_t* d_base; const uint64_t* d_starts;
    int rc = vlr_dev_file_split_view(df, &d_base, &d_starts);
    if (rc != VLR_OK) return rc;
    size_t c1 = s->rec_cap, c2 = s->rec_cap, c3 = s->rec_cap;
    if ((size_t)n > s->rec_cap) {
        VLR_HIP_OK(hipStreamSynchronize(st));
        if ((rc = grow(s->d_take, c1, (size_t)n)) || (rc = grow(s->d_sel, c2, (size_t)n)) || (rc = grow(s->d_tlen, c3, (size_t)n))) return rc;
        s->rec_cap = c1;
    }
    const size_t n_refs = names.size();
    double t0 = now_s();
    hipLaunchKernelGGL(bam_take_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_base, d_starts, n, s->d_take);
    VLR_HIP_OK(hipMemsetAsync(s->d_used, 0, n_refs ? n_refs : 1, st));
    VLR_HIP_OK(hipMemsetAsync(s->d_out, 0, 16, st));
    const uint64_t remaining = (uint64_t)s->cap - s->n_taken;
    hipLaunchKernelGGL(bam_select_kernel, dim3(1), dim3(kSelThreads), 0, st, d_base, d_starts, n, s->d_take, remaining, (int)n_refs, rec0, s->d_sel,
                       s->d_used, s->d_out, s->d_misc);
    uint64_t out[2], err[2];
    std::vector<uint8_t> used(n_refs ? n_refs : 1);
    VLR_HIP_OK(hipMemcpyAsync(out, s->d_out, 16, hipMemcpyDeviceToHost, st));
    VLR_HIP_OK(hipMemcpyAsync(err, s->d_misc + M_ERR_CODE, 16, hipMemcpyDeviceToHost, st));
    VLR_HIP_OK(hipMemcpyAsync(used.data(), s->d_used, used.size(), hipMemcpyDeviceToHost, st));
    VLR_HIP_OK(hipStreamSynchronize(st));
    VLR_HIP_OK(hipGetLastError());
    s->t[3] += now_s() - t0;
    if (err[0]) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: record %llu: %s", path, (unsigned long long)err[1],
                             (err[0] & E_MALFORMED) ? "malformed record (fields overrun block_size)" : "reference id out of range");
    if (out[0] == 0) { s->n_skipped += out[1]; return VLR_OK; }
    // the contigs the analysed records lie on
    t0 = now_s();
    std::vector<const uint8_t*> ptr(n_refs);
    std::vector<uint64_t> len(n_refs);
    for (size_t k = 0; k < n_refs; ++k) {
        std::pair<uint8_t*, uint64_t> c{nullptr, 0};
        auto it = s->contigs.find(names[k]);
        if (it != s->contigs.end()) c = it->second;
        else if (used[k] && (rc = load_contig(s->fasta, s->fai, s->contigs, names[k], path, false, c)) != VLR_OK) return rc;
        ptr[k] = c.first; len[k] = c.second;
    }
    if (n_refs) {
        VLR_HIP_OK(hipMemcpyAsync((void*)s->d_ctg, ptr.data(), n_refs * sizeof(void*), hipMemcpyHostToDevice, st));
        VLR_HIP_OK(hipMemcpyAsync(s->d_ctg_len, len.data(), n_refs * 8, hipMemcpyHostToDevice, st));
    }
    VLR_HIP_OK(hipStreamSynchronize(st));
    s->t[4] += now_s() - t0;
    t0 = now_s();
    const int64_t blocks = std::min<int64_t>((n + kWaves - 1) / kWaves, 1024);
    hipLaunchKernelGGL(bam_stats_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, d_base, d_starts, n, s->d_sel, s->d_ctg, s->d_ctg_len, rec0,
                       s->d_trans, s->d_dense, s->d_hkeys, s->d_hvals, s->d_misc, s->d_tlen);
    VLR_HIP_OK(hipMemcpyAsync(err, s->d_misc + M_ERR_CODE, 16, hipMemcpyDeviceToHost, st));
    VLR_HIP_OK(hipStreamSynchronize(st));
    VLR_HIP_OK(hipGetLastError());
    s->t[5] += now_s() - t0;
    if (err[0]) {
        const char* what = (err[0] & E_CIGAR_RANGE) ? "CIGAR runs past the contig or the read" : (err[0] & E_MALFORMED) ? "malformed record (unknown CIGAR operation)"
                           : (err[0] & E_KEY) ? "homopolymer run longer than 2^28 - 2" : "hop counter table full";
        return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: record %llu: %s", path, (unsigned long long)err[1], what);
    }
    t0 = now_s();
    std::vector<int64_t> tl((size_t)n);
    VLR_HIP_OK(hipMemcpyAsync(tl.data(), s->d_tlen, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    VLR_HIP_OK(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i) if (tl[(size_t)i] >= 0) s->tlens.push_back(tl[(size_t)i]);
    s->t[6] += now_s() - t0;
    s->n_taken += out[0];
    s->n_skipped += out[1];
    return VLR_OK;
}

// One BAM file through the device reader: the BGZF member index from the file read in bounded pieces, the feeds up to the window, the
// header skipped, the record split, and per split the caller's chunk pass (vlr_bamstream.h)
int stream_bam(const BamStream& b, const char* path) {
    const double t_all = now_s();
    double sink = 0.0;
    auto T = [&](double* p) -> double& { return p ? *p : sink; };
    size_t& window = *b.window;
    FILE* f = fopen(path, "rb");
    if (!f) return bfail(VLR_ERR_INVALID_ARGUMENT, "cannot open %s", path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
    vlr_dev_file* df = nullptr;
    int rc = vlr_dev_file_create(b.device, &df);
    if (rc != VLR_OK) return rc;
    struct Destroyer { vlr_dev_file* d; ~Destroyer() { vlr_dev_file_destroy(d); } } destroyer{df};
    hipStream_t st = (hipStream_t)vlr_dev_file_stream(df);
    std::vector<uint8_t> buf;          // compressed bytes not yet fed: [0, have)
    size_t have = 0;
    bool eof = false;
    std::vector<Member> members;
    std::vector<vlr::InflateBlock> ib;
    // header: inflated on the host from the first members (the device skips the same bytes)
    std::vector<uint8_t> head;
    size_t head_need = 0;              // 0: not known yet
    std::vector<std::string> names;
    bool header_skipped = false;
    uint64_t rec0 = 0;                 // records of this file in front of the current chunk
    double t0;
    auto read_more = [&]() -> int {
        t0 = now_s();
        if (buf.size() < have + kReadPiece) buf.resize(have + kReadPiece);
        const size_t got = fread(buf.data() + have, 1, kReadPiece, f);
        have += got;
        if (got < kReadPiece) eof = true;
        T(b.t_read) += now_s() - t0;
        return VLR_OK;
    };
    auto parse_header = [&]() -> int {   // from `head` (host-inflated); sets head_need and names when complete
        if (head.size() < 12) return VLR_OK;
        if (memcmp(head.data(), "BAM\1", 4) != 0) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: not a BAM file", path);
        int32_t l_text; memcpy(&l_text, head.data() + 4, 4);
        if (l_text < 0) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: malformed BAM header", path);
        size_t o = 8 + (size_t)l_text;
        if (head.size() < o + 4) return VLR_OK;
        int32_t n_ref; memcpy(&n_ref, head.data() + o, 4);
        if (n_ref < 0) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: malformed BAM header", path);
        o += 4;
        std::vector<std::string> nm;
        for (int32_t k = 0; k < n_ref; ++k) {
            if (head.size() < o + 4) return VLR_OK;
            int32_t l_name; memcpy(&l_name, head.data() + o, 4);
            if (l_name < 1) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: malformed BAM header", path);
            if (head.size() < o + 8 + (size_t)l_name) return VLR_OK;
            nm.emplace_back((const char*)head.data() + o + 4, (size_t)l_name - 1);
            o += 8 + (size_t)l_name;
        }
        names = nm;
        head_need = o;
        return VLR_OK;
    };
    size_t fed_members_bytes = 0;      // compressed bytes consumed from buf by feeds
    while (true) {
        if (b.done && b.done()) break;
        // feed up to the window
        while (vlr_dev_file_buffered(df) < window + (header_skipped ? 0 : head_need)) {
            members.clear();
            size_t used = 0;
            if (!index_members(buf.data() + fed_members_bytes, have - fed_members_bytes, members, &used))
                return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: not a BGZF file, or a corrupt BGZF member", path);
            if (members.empty()) {
                if (eof) {
                    if (have > fed_members_bytes) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: truncated BGZF member at the end of the file", path);
                    break;
                }
                // compact and read on
                memmove(buf.data(), buf.data() + fed_members_bytes, have - fed_members_bytes);
                have -= fed_members_bytes; fed_members_bytes = 0;
                read_more();
                continue;
            }
            // a feed of members up to the window
            ib.clear();
            uint64_t add = 0;
            size_t k = 0;
            const uint64_t goal = window + (header_skipped ? 0 : (head_need ? head_need : window));
            for (; k < members.size() && (k == 0 || vlr_dev_file_buffered(df) + add < goal) && k < (1u << 16); ++k) {
                vlr::InflateBlock x;
                x.src = members[k].off - members[0].off; x.dst = add; x.clen = (uint32_t)members[k].clen; x.isize = members[k].isize; x.crc = members[k].crc; x.pad = 0;
                ib.push_back(x);
                add += members[k].isize;
            }
            const uint8_t* mb = buf.data() + fed_members_bytes;
            if (head_need == 0) {   // header members inflated on the host as well
                for (size_t j = 0; j < k && head_need == 0; ++j) {
                    const size_t old = head.size();
                    head.resize(old + members[j].isize);
                    z_stream z; memset(&z, 0, sizeof z);
                    if (inflateInit2(&z, -15) != Z_OK) return bfail(VLR_ERR_HIP, "zlib init failed");
                    z.next_in = (Bytef*)(mb + members[j].off); z.avail_in = (uInt)members[j].clen;
                    z.next_out = head.data() + old; z.avail_out = members[j].isize;
                    const int zr = inflate(&z, Z_FINISH);
                    inflateEnd(&z);
                    if (zr != Z_STREAM_END || z.avail_out != 0) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: corrupt BGZF member in the header", path);
                    if ((rc = parse_header()) != VLR_OK) return rc;
                }
            }
            const size_t comp_bytes = (members[k - 1].off + members[k - 1].clen) - members[0].off;
            t0 = now_s();
            rc = vlr_dev_file_feed(df, mb + members[0].off, comp_bytes, ib.data(), (int)ib.size(), add);
            if (rc == VLR_OK) rc = vlr_dev_file_feed_wait(df);   // (the compressed bytes stay valid until here)
            T(b.t_feed) += now_s() - t0;
            if (rc != VLR_OK) return rc;
            // everything in front of the end of member k - 1 is consumed (the member headers in between included)
            const size_t consumed_to = fed_members_bytes + (members[k - 1].off + members[k - 1].clen + 8);
            fed_members_bytes = consumed_to;
            if (!header_skipped && head_need && vlr_dev_file_buffered(df) >= head_need) {
                if ((rc = vlr_dev_file_skip(df, head_need)) != VLR_OK) return rc;
                header_skipped = true;
                if (b.on_header && (rc = b.on_header(names)) != VLR_OK) return rc;
            }
        }
        if (!header_skipped) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: truncated BAM header", path);
        t0 = now_s();
        int64_t n = 0;
        int serial = 0;
        const uint64_t buffered = vlr_dev_file_buffered(df);
        if (buffered == 0) break;
        // (at most kSplitRecords per split: the reader's record arrays are sized by it)
        rc = vlr_dev_file_split_bam(df, (int64_t)std::min<uint64_t>(buffered / 36 + 1, kSplitRecords), (int)names.size(), &n, &serial);
        T(b.t_split) += now_s() - t0;
        if (rc != VLR_OK) return rc;
        T(b.n_serial) += serial;
        if (n == 0) {
            const bool more = !eof || fed_members_bytes < have;
            if (!more) {
                if (b.on_truncated) { rc = b.on_truncated(rec0); break; }
                return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: record %llu: truncated (the file ends inside it)", path, (unsigned long long)rec0);
            }
            window = std::max<size_t>(window, (size_t)buffered * 2);   // a record longer than the window: grow it for this record
            continue;
        }
        if ((rc = b.on_chunk(df, n, rec0, names, path, (void*)st)) != VLR_OK) return rc;
        if ((rc = vlr_dev_file_consume(df, n)) != VLR_OK) return rc;
        rec0 += (uint64_t)n;
    }
    T(b.t_inflate) += vlr_dev_file_inflate_seconds(df, 1);
    T(b.t_total) += now_s() - t_all;
    return rc;
}

// the statistics pass over one BAM file
int add_bam(vlr_bamstats* s, const char* path) {
    BamStream b;
    b.device = s->device;
    b.window = &s->window;
    b.t_read = &s->t[0]; b.t_feed = &s->t[1]; b.t_split = &s->t[2]; b.t_inflate = &s->t[8]; b.t_total = &s->t[7]; b.n_serial = &s->t[9];
    b.done = [s]() { return s->n_taken >= (uint64_t)s->cap; };
    b.on_header = [s](const std::vector<std::string>& names) -> int {
        int rc;
        size_t uc = s->used_cap;
        if ((rc = grow(s->d_used, uc, names.size() + 1)) != VLR_OK) return rc;
        s->used_cap = uc;
        if (names.size() + 1 > s->ctg_cap) {
            size_t c1 = s->ctg_cap, c2 = s->ctg_cap;
            if ((rc = grow(s->d_ctg, c1, names.size() + 1)) || (rc = grow(s->d_ctg_len, c2, names.size() + 1))) return rc;
            s->ctg_cap = c1;
        }
        return VLR_OK;
    };
    b.on_chunk = [s](vlr_dev_file* df, int64_t n, uint64_t rec0, const std::vector<std::string>& names, const char* path, void* st) {
        return run_chunk(s, df, n, rec0, names, path, (hipStream_t)st);
    };
    return stream_bam(b, path);
}

}  // namespace vlr_bam

extern "C" {

int vlr_bamstats_open(int device, const char* fasta_path, int64_t max_records, int64_t window_bytes, vlr_bamstats** out) {
    using namespace vlr_bam;
    if (!out || !fasta_path || max_records < 0 || window_bytes < 0) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_bamstats_open: bad argument");
    *out = nullptr;
    int rc = use_device(device);
    if (rc != VLR_OK) return rc;
    vlr_bamstats* s = new vlr_bamstats();
    s->device = device;
    s->fasta = fasta_path;
    s->cap = max_records;
    if (window_bytes > 0) s->window = (size_t)window_bytes;
    rc = read_fai(s->fasta, s->fai);
    if (rc == VLR_OK) rc = alloc_state(s);
    if (rc != VLR_OK) { vlr_bamstats_close(s); return rc; }
    *out = s;
    return VLR_OK;
}

int vlr_bamstats_add_bam(vlr_bamstats* s, const char* bam_path) {
    if (!s || !bam_path) return vlr_bam::bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_bamstats_add_bam: null");
    if (s->collected) return vlr_bam::bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_bamstats_add_bam: the result was already read");
    if (hipSetDevice(s->device) != hipSuccess) return vlr_bam::bfail(VLR_ERR_HIP, "hipSetDevice(%d) failed", s->device);
    return vlr_bam::add_bam(s, bam_path);
}

int vlr_bamstats_result(vlr_bamstats* s, vlr_bamstats_counts* r) {
    using namespace vlr_bam;
    if (!s || !r) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_bamstats_result: null");
    VLR_HIP_OK(hipSetDevice(s->device));
    if (!s->collected) {
        std::vector<uint64_t> dense(kDense), hk(kHashSlots), hv(kHashSlots);
        VLR_HIP_OK(hipMemcpy(dense.data(), s->d_dense, kDense * 8, hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(hk.data(), s->d_hkeys, (size_t)kHashSlots * 8, hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(hv.data(), s->d_hvals, (size_t)kHashSlots * 8, hipMemcpyDeviceToHost));
        std::map<uint64_t, uint64_t> all;
        static const char kBase[8] = {'A', 'C', 'G', 'T', 'a', 'c', 'g', 't'};
        for (int b = 0; b < 8; ++b)
            for (int k0 = 0; k0 < kDenseK; ++k0)
                for (int k1 = 0; k1 < kDenseK; ++k1) {
                    const uint64_t v = dense[(size_t)(b * kDenseK + k0) * kDenseK + k1];
                    if (v) all[((uint64_t)(uint8_t)kBase[b] << 56) | ((uint64_t)k0 << 28) | (uint64_t)k1] += v;
                }
        for (uint32_t i = 0; i < kHashSlots; ++i)
            if (hk[i] != kEmpty) all[hk[i]] += hv[i];
        s->hop_keys.clear(); s->hop_vals.clear();
        for (auto& kv : all) { s->hop_keys.push_back(kv.first); s->hop_vals.push_back(kv.second); }
        s->collected = true;
    }
    uint64_t misc[M_N];
    VLR_HIP_OK(hipMemcpy(r->transitions, s->d_trans, 256 * 8, hipMemcpyDeviceToHost));
    VLR_HIP_OK(hipMemcpy(misc, s->d_misc, M_N * 8, hipMemcpyDeviceToHost));
    r->n_taken = (int64_t)s->n_taken; r->n_skipped = (int64_t)s->n_skipped;
    r->n_not_usable = (int64_t)misc[M_NOT_USABLE]; r->n_softclips = (int64_t)misc[M_SOFT];
    r->n_not_paired = (int64_t)misc[M_NOT_PAIRED]; r->n_not_first = (int64_t)misc[M_NOT_FIRST];
    r->n_mate_unmapped = (int64_t)misc[M_MATE_UNMAPPED]; r->n_tid_mismatch = (int64_t)misc[M_TID_MISMATCH];
    r->max_del = (int64_t)misc[M_MAX_DEL] - 1; r->max_ins = (int64_t)misc[M_MAX_INS] - 1;
    r->has_softclip = misc[M_FRAC] ? 1 : 0;
    r->frac_max_softclip = 0.0;
    if (misc[M_FRAC]) { const uint64_t b = misc[M_FRAC] - 1; memcpy(&r->frac_max_softclip, &b, 8); }
    r->max_read_len = misc[M_READ_LEN] ? (int64_t)misc[M_READ_LEN] - 1 : 0;
    r->max_mapq = misc[M_MAPQ] ? (int64_t)misc[M_MAPQ] - 1 : 0;
    r->n_hop_keys = (int64_t)s->hop_keys.size();
    r->n_insert_sizes = (int64_t)s->tlens.size();
    for (int k = 0; k < 10; ++k) r->seconds[k] = s->t[k];
    return VLR_OK;
}

int vlr_bamstats_read(vlr_bamstats* s, uint64_t* hop_keys, uint64_t* hop_counts, int64_t n_hop, int64_t* insert_sizes, int64_t n_insert) {
    if (!s || !s->collected) return vlr_bam::bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_bamstats_read: call vlr_bamstats_result first");
    if (n_hop != (int64_t)s->hop_keys.size() || n_insert != (int64_t)s->tlens.size())
        return vlr_bam::bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_bamstats_read: sizes differ from vlr_bamstats_result");
    if (n_hop) { memcpy(hop_keys, s->hop_keys.data(), (size_t)n_hop * 8); memcpy(hop_counts, s->hop_vals.data(), (size_t)n_hop * 8); }
    if (n_insert) memcpy(insert_sizes, s->tlens.data(), (size_t)n_insert * 8);
    return VLR_OK;
}

void vlr_bamstats_close(vlr_bamstats* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    void* p[] = {s->d_trans, s->d_dense, s->d_hkeys, s->d_hvals, s->d_misc, s->d_out, s->d_take, s->d_sel, s->d_used, s->d_tlen, (void*)s->d_ctg, s->d_ctg_len};
    for (void* q : p) if (q) (void)hipFree(q);
    for (auto& kv : s->contigs) if (kv.second.first) (void)hipFree(kv.second.first);
    delete s;
}

}  // extern "C"
