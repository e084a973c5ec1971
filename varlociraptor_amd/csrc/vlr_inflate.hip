// BGZF members inflated on the device: one wave64 (= one workgroup) per member.
//
// What it replaces: htslib's bgzf_read / libdeflate behind rust-htslib's bcf::Reader, which the reference opens per sample in
// `call variants` (reference src/calling/variants/calling.rs:297-316, ObservationBcfs; preprocessing/mod.rs:818-919 reads the
// records).  On the 16-CPU box the host inflate of the observation files is 3.4 CPU-seconds per 200 000 tumor-normal records — the
// whole budget of 1 M records/s — while the compressed bytes are 1/11 of the inflated ones: they cross PCIe, and the
// inflated stream is born in HBM where the record decoder (vlr_decode.hip) reads it.
//
// DEFLATE (RFC 1951) is a serial bit stream: symbol k+1 starts where symbol k ends.  The wave runs it as ONE decoder whose state
// (bit buffer, output position, current symbol) is wave-uniform, and uses the 64 lanes for everything that is parallel around it:
//   * the compressed bytes reach the bit buffer through a 64-dword window held one dword per lane (one coalesced load per 256
//     bytes, prefetched one window ahead); the decoder takes dword i with a lane read — no memory latency on the serial path;
//   * the last 4 KiB of the inflated member live in an LDS ring, so a match is one LDS read and one LDS write of up to 64 bytes per
//     instruction pair, with the period trick for overlapping matches (source index = i mod distance), and literals are single LDS
//     byte stores; the one match in ten that reaches further back than the ring (DEFLATE's window is 32 KiB) reads the member's own
//     flushed output from HBM instead.  11 kB of LDS per wave = fourteen members in flight per CU (round 4: a 32 KiB ring, 39 kB,
//     four members — one wave per SIMD, whose ~70 dependent instructions per symbol set the pace with nothing to hide them behind);
//   * symbols are decoded in speculative batches: lane i decodes the symbol that WOULD start at bit i of the next 64 stream bits
//     (literal/length lookup, extra bits, distance lookup, extra bits — two LDS round trips for 64 candidates at once) and leaves a
//     32-bit token with the bits it takes; the wave then follows the chain of real symbol starts through the tokens with lane reads
//     and executes them in order (about six symbols per batch in the observation files).  Codes longer than the table index are
//     decoded bit by bit where the chain reaches them.  The first version of the loop — one symbol at a time, the table entry of the
//     next symbol fetched before the bytes of the current match are copied — is kept (VLR_INFLATE_BATCH=0): the tests run both;
//   * Huffman tables are built by all lanes (canonical codes from per-length ballots) into single-lookup tables whose entries
//     already carry the length / distance base and extra-bit count; codes longer than the table index fall back to the canonical
//     bit-serial walk;
//   * finished 8 KiB pieces of the ring go to HBM in 16-byte lanes (ring positions are shifted by the low 4 bits of the destination
//     so both sides of the copy are aligned).
// The CRC32 of every member is checked against its trailer by vlr_crc_kernel, launched behind the inflate kernel (below).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "vlr_gpuio.h"

namespace vlr {
namespace {

#ifndef VLR_INFL_LIT_BITS   // (sweep builds: tools/inflate_sweep.sh)
#define VLR_INFL_LIT_BITS 10
#endif
#ifndef VLR_INFL_DIST_BITS
#define VLR_INFL_DIST_BITS 9
#endif
#ifndef VLR_INFL_RING
#define VLR_INFL_RING 4096
#endif
constexpr int kLitBits = VLR_INFL_LIT_BITS, kDistBits = VLR_INFL_DIST_BITS, kClBits = 7;
constexpr bool kInflateBatchDefault = true;   // speculative batches (VLR_INFLATE_BATCH=0: one symbol at a time, the cross-check)
// a corrupt stream is noticed at the next position check (every 8.7 KiB of output at most = 16.3 KiB of input at 15 bits per symbol):
// the compressed bytes handed to the kernel must be readable this far beyond the last member (vlr_gpuio.h kInflateInputSlack)
// The ring holds the last 4 KiB of the inflated member, not DEFLATE's whole 32 KiB window: 86 % of the matches of an observation file
// reach back less than 1 KiB, 10 % between 8 and 16 KiB (the same INFO vector of the previous record) whatever the ring below 8 KiB — a
// match that reaches beyond the ring (dist + len > kRing) takes its bytes from the member's flushed output in HBM (L2-resident: written
// microseconds ago by this wave).  11 kB of LDS per wave instead of 39: fourteen members per CU instead of four, which is what a
// decoder bound by the issue rate and latencies of ONE wave needs.  Everything below kRing - (kFlush + 512 + 2 x 258) behind the
// position is in HBM when a far match asks for it: kRing >= kFlush + 1286.
constexpr uint32_t kRing = VLR_INFL_RING, kRingMask = kRing - 1, kFlush = 1024;   // flushed to HBM in 1 KiB pieces, each before the ring wraps onto it
static_assert(kRing >= kFlush + 1286, "far matches read flushed bytes only");
constexpr uint32_t kBadDistance = 1u, kBadSymbol = 2u, kBadOutput = 4u, kBadInput = 8u;   // the symbol loops' `bad`

struct InflLds {
    uint8_t out[kRing];              // ring over the last kRing bytes of the inflated member, position shifted by (HBM destination & 15)
    uint32_t lit[1 << kLitBits];     // code length (4) | kind (2: literal, length, end of block, invalid) @4 | value or length base (9) @8 | extra bits (3) @20
    uint32_t dist[1 << kDistBits];   // code length (4) | extra bits (4; 15 = invalid symbol) @4 | base (16) @8.  Also the code-length code's table.
    uint16_t lsym[288], dsym[32];    // symbols in canonical order (bit-serial fallback)
    uint16_t lcount[16], dcount[16];
    uint8_t lens[328];
};

struct Bits {
    const uint32_t* g;   // dword-aligned base of the stream
    uint32_t cur, nxt;   // per lane: dwords 64 wi + lane and 64 (wi + 1) + lane
    uint32_t w;          // next dword to take
    uint64_t buf;
    int cnt;
};
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t take32(Bits& b, int lane) {
    const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)b.cur, (int)uni(b.w & 63u));
    b.w += 1;
    if ((b.w & 63u) == 0) { b.cur = b.nxt; b.nxt = b.g[b.w + 64 + lane]; }
    return v;
}
__device__ __forceinline__ void refill(Bits& b, int lane) {  // afterwards at least 33 bits are buffered
    if (b.cnt <= 32) { b.buf |= (uint64_t)take32(b, lane) << b.cnt; b.cnt += 32; }
}
__device__ __forceinline__ uint32_t peek(const Bits& b, int n) { return (uint32_t)b.buf & ((1u << n) - 1u); }
__device__ __forceinline__ void drop(Bits& b, int n) { b.buf >>= n; b.cnt -= n; }
__device__ __forceinline__ void bits_open(Bits& b, const uint8_t* p, int lane) {
    const uintptr_t a = (uintptr_t)p;
    b.g = (const uint32_t*)(a & ~(uintptr_t)3);
    b.w = 0; b.buf = 0; b.cnt = 0;
    b.cur = b.g[lane]; b.nxt = b.g[64 + lane];
    refill(b, lane);
    drop(b, (int)(a & 3) * 8);
}
__device__ __forceinline__ const uint8_t* bits_byte_pos(const Bits& b) {  // (only at a byte boundary)
    return (const uint8_t*)b.g + (((uint64_t)b.w * 32 - (uint64_t)b.cnt) >> 3);
}
__device__ __forceinline__ const uint8_t* bits_used_end(const Bits& b) {  // first byte no consumed bit lies in
    return (const uint8_t*)b.g + (((uint64_t)b.w * 32 - (uint64_t)b.cnt + 7) >> 3);
}

template <int KIND>
__device__ __forceinline__ uint32_t make_entry(uint32_t s) {
    if (KIND == 0) {
        if (s < 256) return s << 8;
        if (s == 256) return 2u << 4;
        if (s > 285) return 3u << 4;
        const uint32_t k = s - 257;
        uint32_t xb = 0, base = 3 + k;
        if (k == 28) base = 258;
        else if (k >= 8) { xb = (k >> 2) - 1; base = 3 + ((4 + (k & 3)) << xb); }
        return (1u << 4) | (base << 8) | (xb << 20);
    }
    if (KIND == 1) {
        if (s >= 30) return 15u << 4;
        uint32_t xb = 0, base = 1 + s;
        if (s >= 4) { xb = (s >> 1) - 1; base = 1 + ((2 + (s & 1)) << xb); }
        return (xb << 4) | (base << 8);
    }
    return s << 8;
}

// canonical Huffman code of `n` symbols with lengths lens[0..n) -> single-lookup table of 2^TB entries (longer codes: entry 0),
// symbols in canonical order and per-length counts for the bit-serial fallback.  false: over-subscribed set of lengths.
template <int KIND, int TB>
__device__ __forceinline__ bool build_table(const uint8_t* lens, int n, uint32_t* table, uint16_t* symorder, uint16_t* count, int lane) {
    for (int i = lane; i < (1 << TB); i += 64) table[i] = 0;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t mycnt = 0;  // lane L: symbols of length L
    const int nch = (n + 63) >> 6;
    for (int c = 0; c < nch; ++c) {
        const int s = c * 64 + lane;
        const int l = s < n ? lens[s] : 0;
        for (int L = 1; L <= 15; ++L) {
            const unsigned long long m = __ballot(l == L);
            if (lane == L) mycnt += (uint32_t)__popcll(m);
        }
    }
    if (lane < 16) count[lane] = (uint16_t)mycnt;
    uint32_t mybase = 0, myoff = 0;
    {
        uint32_t code = 0, off = 0, prev = 0;
        int left = 1;
        for (int L = 1; L <= 15; ++L) {
            const uint32_t cL = (uint32_t)__builtin_amdgcn_readlane((int)mycnt, L);
            left = (left << 1) - (int)cL;
            if (left < 0) return false;
            code = (code + prev) << 1;
            if (lane == L) { mybase = code; myoff = off; }
            off += cL; prev = cL;
        }
    }
    for (int c = 0; c < nch; ++c) {
        const int s = c * 64 + lane;
        const int l = s < n ? lens[s] : 0;
        uint32_t code_s = 0, idx_s = 0;
        for (int L = 1; L <= 15; ++L) {
            const unsigned long long m = __ballot(l == L);
            if (m == 0) continue;
            const uint32_t bL = (uint32_t)__builtin_amdgcn_readlane((int)mybase, L), oL = (uint32_t)__builtin_amdgcn_readlane((int)myoff, L);
            const uint32_t rank = (uint32_t)__popcll(m & lt), pc = (uint32_t)__popcll(m);
            if (l == L) { code_s = bL + rank; idx_s = oL + rank; }
            if (lane == L) { mybase += pc; myoff += pc; }
        }
        if (l > 0) {
            symorder[idx_s] = (uint16_t)s;
            if (l <= TB) {
                const uint32_t rev = __brev(code_s) >> (32 - l);
                const uint32_t e = make_entry<KIND>((uint32_t)s) | (uint32_t)l;
                for (uint32_t k = rev; k < (1u << TB); k += 1u << l) table[k] = e;
            }
        }
    }
    return true;
}

// bit-serial canonical decode (codes longer than the table index); needs 15 buffered bits.  -1: no such code
__device__ __forceinline__ int slow_symbol(Bits& b, const uint16_t* count, const uint16_t* symorder) {
    const uint32_t v = (uint32_t)b.buf;
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)((v >> (len - 1)) & 1u);
        const int c = (int)uni(count[len]);
        if (code - c < first) {
            const int sym = (int)uni(symorder[index + (code - first)]);
            drop(b, len);
            return sym;
        }
        index += c; first += c;
        first <<= 1; code <<= 1;
    }
    return -1;
}

// the same walk on a value (the low 15 bits of v are the next stream bits)
// (returns symbol | code length << 16, or -1)
__device__ __forceinline__ int slow_symbol_v(uint32_t v, const uint16_t* count, const uint16_t* symorder) {
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)((v >> (len - 1)) & 1u);
        const int c = (int)uni(count[len]);
        if (code - c < first) return (int)uni(symorder[index + (code - first)]) | (len << 16);
        index += c; first += c;
        first <<= 1; code <<= 1;
    }
    return -1;
}
// 32 stream bits at bit offset q (< 128) of the five dwords S0..S4
// (five values, not an array: a select chain over an array in memory turns into an indexed scratch load)
__device__ __forceinline__ uint32_t window_bits(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t s4, uint32_t q) {
    const bool b0 = (q & 32u) != 0, b1 = (q & 64u) != 0;
    const uint32_t lo = b1 ? (b0 ? s3 : s2) : (b0 ? s1 : s0);
    const uint32_t hi = b1 ? (b0 ? s4 : s3) : (b0 ? s2 : s1);
    return __builtin_amdgcn_alignbit(hi, lo, q & 31u);
}
// token of one symbol: kind (2: 0 literal, 1 match, 2 end of block, 3 invalid) | stream bits it takes (6; 0 = not decodable by table
// lookups alone) @2 | literal byte or match length (9) @8 | distance - 1 (15) @17
__device__ __forceinline__ uint32_t make_token(uint32_t kind, uint32_t adv, uint32_t val, uint32_t dist) { return kind | (adv << 2) | (val << 8) | ((dist - 1u) << 17); }

// ring position P (= shift + byte offset in the member) -> HBM: pieces [from, to) with from a multiple of 16 except at the member's start
__device__ __forceinline__ void flush_ring(const InflLds& L, uint8_t* gbase, uint32_t from, uint32_t to, int lane) {
    for (uint32_t k = (from & ~15u) + 16u * (uint32_t)lane; k < to; k += 1024u) {
        if (k >= from && k + 16 <= to) *reinterpret_cast<uint4*>(gbase + k) = *reinterpret_cast<const uint4*>(&L.out[k & kRingMask]);
        else
            for (uint32_t j = k < from ? from : k; j < k + 16 && j < to; ++j) gbase[j] = L.out[j & kRingMask];
    }
}

// the len bytes of a match at distance dist, appended at ring position pos (all wave-uniform).  Near matches: one LDS read and one LDS
// write of up to 64 bytes per instruction pair, byte k of the match repeats with period dist (k mod dist, = k when dist >= len; an
// approximate reciprocal with two corrections is exact for k < 512).  Far matches (beyond the ring): the bytes come from the member's
// own output in HBM, which the flushes have written (kRing >= kFlush + 1286: every byte that far back is flushed) — loads at agent
// scope (past the vector L1, which may hold a line of the flush frontier from an earlier far match), after the flush stores of
// this wave have completed.  `ok`: the distance lies inside the member (a corrupt stream's does not: nothing is read then).
__device__ __forceinline__ void copy_match(InflLds& L, const uint8_t* gbase, uint32_t pos, uint32_t dist, uint32_t len, bool ok, int lane) {
    const uint32_t from = pos - dist;
    if (__builtin_expect(dist + len > kRing, 0)) {
        if (!ok) return;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        for (uint32_t k = (uint32_t)lane; k < len; k += 64) {
            const uintptr_t a = (uintptr_t)(gbase + from + k);
            const uint32_t w = __hip_atomic_load((const uint32_t*)(a & ~(uintptr_t)3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            L.out[(pos + k) & kRingMask] = (uint8_t)(w >> (8u * (uint32_t)(a & 3)));
        }
        return;
    }
    const float rd = __builtin_amdgcn_rcpf((float)(dist | (uint32_t)(dist == 0)));
    if (len <= 64) {
        const uint32_t k = (uint32_t)lane;
        int r = (int)k - (int)((float)k * rd) * (int)dist;
        r = r < 0 ? r + (int)dist : r;
        r = r >= (int)dist ? r - (int)dist : r;
        const uint8_t v = L.out[(from + (uint32_t)r) & kRingMask];
        if (k < len) L.out[(pos + k) & kRingMask] = v;
    } else {
        for (uint32_t k = (uint32_t)lane; k < len; k += 64) {
            int r = (int)k - (int)((float)k * rd) * (int)dist;
            r = r < 0 ? r + (int)dist : r;
            r = r >= (int)dist ? r - (int)dist : r;
            L.out[(pos + k) & kRingMask] = L.out[(from + (uint32_t)r) & kRingMask];
        }
    }
}

template <bool BATCH>
__global__ __launch_bounds__(64) void vlr_inflate_kernel(const uint8_t* __restrict__ comp, const InflateBlock* __restrict__ blocks, int n_blocks,
                                                        uint8_t* __restrict__ out, int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) InflLds L;
    const int lane = (int)threadIdx.x;
    const int blk = (int)blockIdx.x;
    if (blk >= n_blocks) return;
    const uint64_t src = blocks[blk].src, dst = blocks[blk].dst;
    const uint32_t clen = uni(blocks[blk].clen), isize = uni(blocks[blk].isize);
    const uint32_t sh = uni((uint32_t)(((uintptr_t)out + dst) & 15));  // ring positions are shifted so that LDS and HBM addresses agree mod 16
    const uint8_t* in_end = comp + src + clen;
    uint8_t* gbase = out + dst - sh;  // 16-byte aligned: ring position P goes to gbase[P]
    int err = INFL_OK;
    uint32_t pos = sh;                // ring position of the next byte
    uint32_t flushed = sh;            // ring positions below are in HBM
    const uint32_t lim = sh + isize;
    if (isize > 65536u) err = INFL_SIZE_MISMATCH;
    Bits b;
    bits_open(b, comp + src, lane);
    bool last = (isize == 0 && clen == 0);
    while (!last && err == INFL_OK) {
        refill(b, lane);
        last = (peek(b, 1) != 0);
        const uint32_t type = (peek(b, 3) >> 1);
        drop(b, 3);
        if (type == 0) {  // stored
            drop(b, b.cnt & 7);
            refill(b, lane);
            const uint32_t len = peek(b, 16);
            drop(b, 16);
            refill(b, lane);
            const uint32_t nlen = peek(b, 16);
            drop(b, 16);
            const uint8_t* p = bits_byte_pos(b);
            if ((len ^ 0xffffu) != nlen) { err = INFL_BAD_STORED; break; }
            if (pos + len > lim) { err = INFL_OUTPUT_OVERRUN; break; }
            if (p + len > in_end) { err = INFL_INPUT_OVERRUN; break; }
            for (uint32_t done = 0; done < len;) {   // through the ring in pieces the flush keeps up with
                const uint32_t piece = len - done < kFlush ? len - done : kFlush;
                for (uint32_t k = (uint32_t)lane; k < piece; k += 64) L.out[(pos + k) & kRingMask] = p[done + k];
                pos += piece; done += piece;
                if (pos - flushed >= kFlush) { const uint32_t to = pos & ~(kFlush - 1); flush_ring(L, gbase, flushed, to, lane); flushed = to; }
            }
            bits_open(b, p + len, lane);
            continue;
        }
        if (type == 3) { err = INFL_BAD_BLOCK_TYPE; break; }
        if (type == 1) {  // fixed code (RFC 1951 3.2.6)
            for (int s = lane; s < 288; s += 64) L.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            if (lane < 32) L.lens[288 + lane] = 5;
            build_table<0, kLitBits>(L.lens, 288, L.lit, L.lsym, L.lcount, lane);
            build_table<1, kDistBits>(L.lens + 288, 32, L.dist, L.dsym, L.dcount, lane);
        } else {  // dynamic code
            refill(b, lane);
            const int hlit = (int)peek(b, 5) + 257;
            drop(b, 5);
            const int hdist = (int)peek(b, 5) + 1;
            drop(b, 5);
            const int hclen = (int)peek(b, 4) + 4;
            drop(b, 4);
            if (hlit > 286 || hdist > 30) { err = INFL_BAD_CODE_LENGTHS; break; }
            if (lane < 19) L.lens[lane] = 0;
            // order of the code-length code lengths (RFC 1951 3.2.7)
            static constexpr unsigned char order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            for (int i = 0; i < hclen; ++i) {
                refill(b, lane);
                const uint32_t v = peek(b, 3);
                drop(b, 3);
                if (lane == 0) L.lens[order[i]] = (uint8_t)v;
            }
            if (!build_table<2, kClBits>(L.lens, 19, L.dist, L.dsym, L.dcount, lane)) { err = INFL_OVERSUBSCRIBED; break; }
            const int total = hlit + hdist;
            int i = 0;
            uint32_t prev = 0;
            while (i < total) {
                refill(b, lane);
                const uint32_t e = uni(L.dist[peek(b, kClBits)]);
                int sym;
                if ((e & 15u) == 0) {
                    sym = slow_symbol(b, L.dcount, L.dsym);
                    if (sym < 0) { err = INFL_BAD_CODE_LENGTHS; break; }
                } else { sym = (int)(e >> 8); drop(b, (int)(e & 15u)); }
                if (sym < 16) { if (lane == 0) L.lens[i] = (uint8_t)sym; prev = (uint32_t)sym; i += 1; continue; }
                int rep;
                uint32_t val = 0;
                if (sym == 16) {
                    if (i == 0) { err = INFL_BAD_CODE_LENGTHS; break; }
                    rep = 3 + (int)peek(b, 2); drop(b, 2); val = prev;
                } else if (sym == 17) { rep = 3 + (int)peek(b, 3); drop(b, 3); prev = 0; }
                else { rep = 11 + (int)peek(b, 7); drop(b, 7); prev = 0; }
                if (i + rep > total) { err = INFL_BAD_CODE_LENGTHS; break; }
                for (int k = lane; k < rep; k += 64) L.lens[i + k] = (uint8_t)val;
                i += rep;
            }
            if (err != INFL_OK) break;
            if (uni(L.lens[256]) == 0) { err = INFL_BAD_CODE_LENGTHS; break; }
            // (the distance lengths are copied behind the 288 literal/length slots before the tables are built: build_table reads them
            // while it writes the tables, and L.dist still holds the code-length table until then)
            const uint8_t dl = lane < hdist ? L.lens[hlit + lane] : (uint8_t)0;
            __builtin_amdgcn_wave_barrier();
            if (lane < 32) L.lens[288 + lane] = dl;
            if (!build_table<0, kLitBits>(L.lens, hlit, L.lit, L.lsym, L.lcount, lane)) { err = INFL_OVERSUBSCRIBED; break; }
            if (!build_table<1, kDistBits>(L.lens + 288, hdist, L.dist, L.dsym, L.dcount, lane)) { err = INFL_OVERSUBSCRIBED; break; }
        }
        // ---- symbols of the block.  `e` is the table entry at the current bit position, fetched one symbol ahead.  Checks that only
        // guard against a corrupt stream (bad distance code, distance beyond the output) are collected in `bad` without a branch:
        // the ring mask keeps every LDS access in range, and the output bound — the one check the HBM copy depends on — stays exact.
        // (One loop exit — every early exit of a multi-exit loop costs the structurised control flow a flag test per iteration — and one
        // rare branch: the position is compared with `next_stop`, the nearer of the next flush point and the member's end; a corrupt
        // stream that runs past the end is caught there, before anything beyond the member's bytes could go to HBM.)
        // `bad` has one bit per reason, and the reason reported is the one that can only have come first: a bad distance does not end
        // the loop (what follows it may be garbage: a bad symbol, an overrun), a bad symbol and an overrun do.  (The INFL_ values
        // themselves were OR-ed here once: a distance symbol without a code in the batch loop gave 6 | 5 = 7, an output overrun.)
        uint32_t bad = 0;
        bool done = false;
        uint32_t next_stop = flushed + kFlush + 512 < lim + 1 ? flushed + kFlush + 512 : lim + 1;
        if (BATCH) {
            // ---- speculative batches: lane i decodes the symbol that WOULD start at bit i of the next 64 stream bits — literal/length
            // lookup, extra bits, distance lookup, extra bits: two LDS round trips for 64 candidates at once — and leaves a token with the
            // bits it takes; then the wave follows the chain of real symbol starts through the tokens with lane reads (no memory latency
            // on the serial path) and executes them in order.  A batch covers ~6 symbols of these files.
            uint32_t bp = b.w * 32u - (uint32_t)b.cnt;   // bit position of the next symbol from b.g
            uint32_t gi = bp >> 11;                        // 64-dword group of the window registers
            uint32_t wcur = b.g[64u * gi + (uint32_t)lane], wnxt = b.g[64u * (gi + 1) + (uint32_t)lane];
            do {
                const uint32_t base = bp >> 5;
                while ((base >> 6) != gi) { wcur = wnxt; gi += 1; wnxt = b.g[64u * (gi + 1) + (uint32_t)lane]; }
                const uint32_t j0 = base - 64u * gi;   // 0 .. 63; dwords j0 .. j0 + 4 of the two window registers
                auto dw = [&](uint32_t j) {
                    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)wcur, (int)uni(j & 63u)), c = (uint32_t)__builtin_amdgcn_readlane((int)wnxt, (int)uni(j & 63u));
                    return j < 64 ? a : c;
                };
                const uint32_t s0 = dw(j0), s1 = dw(j0 + 1), s2 = dw(j0 + 2), s3 = dw(j0 + 3), s4 = dw(j0 + 4);
                const uint32_t q0 = bp & 31u;
                uint32_t tok;
                {
                    const uint32_t q = q0 + (uint32_t)lane;
                    const uint32_t v = window_bits(s0, s1, s2, s3, s4, q);
                    const uint32_t e = L.lit[v & ((1u << kLitBits) - 1u)];
                    const uint32_t cl = e & 15u, kind = (e >> 4) & 3u;
                    const uint32_t xb = (e >> 20) & 7u;
                    const uint32_t len = ((e >> 8) & 511u) + ((v >> cl) & ((1u << xb) - 1u));
                    const uint32_t v2 = window_bits(s0, s1, s2, s3, s4, q + cl + xb);
                    const uint32_t d = L.dist[v2 & ((1u << kDistBits) - 1u)];
                    const uint32_t dl = d & 15u, dx = (d >> 4) & 15u;
                    const uint32_t dist = (d >> 8) + ((v2 >> dl) & ((1u << dx) - 1u));
                    const bool m_ok = dl != 0 && dx != 15u && dist != 0;
                    const uint32_t adv = cl == 0 || kind == 3 ? 0u : kind == 1 ? (m_ok ? cl + xb + dl + dx : 0u) : cl;
                    tok = kind == 1 ? make_token(1, adv, len, m_ok ? dist : 1u) : make_token(kind, adv, kind == 0 ? (e >> 8) & 255u : 0u, 1u);
                }
                uint32_t off = 0;
                for (;;) {
                    uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)tok, (int)uni(off));
                    if (__builtin_expect(((t >> 2) & 63u) == 0, 0)) {
                        // a code longer than the table index (or an invalid one) starts here: decode this symbol bit by bit
                        const uint32_t qu = q0 + off;
                        const unsigned long long v64 = (unsigned long long)uni(window_bits(s0, s1, s2, s3, s4, qu)) | ((unsigned long long)uni(window_bits(s0, s1, s2, s3, s4, qu + 32)) << 32);
                        uint32_t e = uni(L.lit[(uint32_t)v64 & ((1u << kLitBits) - 1u)]);
                        int n = (int)(e & 15u);
                        if (n == 0) {
                            const int sl = slow_symbol_v((uint32_t)v64, L.lcount, L.lsym);
                            e = sl < 0 ? (3u << 4) : make_entry<0>((uint32_t)sl & 0xffffu);
                            n = sl < 0 ? 1 : sl >> 16;
                        }
                        const uint32_t kind = (e >> 4) & 3u;
                        if (kind == 1) {
                            const int xb = (int)((e >> 20) & 7u);
                            const uint32_t len = ((e >> 8) & 511u) + ((uint32_t)(v64 >> n) & ((1u << xb) - 1u));
                            n += xb;
                            uint32_t d = uni(L.dist[(uint32_t)(v64 >> n) & ((1u << kDistBits) - 1u)]);
                            int dl = (int)(d & 15u);
                            if (dl == 0) {
                                const int sl = slow_symbol_v((uint32_t)(v64 >> n), L.dcount, L.dsym);
                                d = sl < 0 ? (15u << 4) : make_entry<1>((uint32_t)sl & 0xffffu);
                                dl = sl < 0 ? 1 : sl >> 16;
                            }
                            n += dl;
                            const int dx = (int)((d >> 4) & 15u);
                            if (dx == 15) { bad |= kBadDistance; t = make_token(3, 1, 0, 1); }
                            else {
                                const uint32_t dist = (d >> 8) + ((uint32_t)(v64 >> n) & ((1u << dx) - 1u));
                                n += dx;
                                t = make_token(1, (uint32_t)n, len, dist ? dist : 1u);
                                if (dist == 0) bad |= kBadDistance;
                            }
                        } else t = make_token(kind, (uint32_t)n, kind == 0 ? (e >> 8) & 255u : 0u, 1u);
                    }
                    const uint32_t kind = t & 3u, adv = (t >> 2) & 63u;
                    if (kind == 0) {
                        L.out[pos & kRingMask] = (uint8_t)((t >> 8) & 255u);
                        pos += 1;
                    } else if (kind == 1) {
                        const uint32_t len = (t >> 8) & 511u, dist = (t >> 17) + 1u;
                        const bool inside = dist <= pos - sh;
                        bad |= inside ? 0u : kBadDistance;
                        copy_match(L, gbase, pos, dist, len, inside, lane);
                        pos += len;
                    } else {
                        done = true;   // 2: end of block
                        bad |= kind == 3 ? kBadSymbol : 0u;
                    }
                    off += adv;
                    if (__builtin_expect(pos >= next_stop, 0)) {
                        if (pos > lim) { bad |= kBadOutput; done = true; }
                        else if (bad) done = true;
                        else if ((const uint8_t*)b.g + ((bp + off) >> 3) > in_end + 8) { bad |= kBadInput; done = true; }   // (a corrupt stream must not read far beyond its member: kInflateInputSlack)
                        else if (pos - flushed >= kFlush + 512) { const uint32_t to = pos & ~(kFlush - 1); flush_ring(L, gbase, flushed, to, lane); flushed = to; }
                        next_stop = flushed + kFlush + 512 < lim + 1 ? flushed + kFlush + 512 : lim + 1;
                    }
                    if (done || off >= 64) break;
                }
                bp += off;
            } while (!done);
            // back to the bit reader at bp (the block header of the next block is read through it)
            b.w = bp >> 5;
            b.cur = b.g[64u * (b.w >> 6) + (uint32_t)lane]; b.nxt = b.g[64u * ((b.w >> 6) + 1) + (uint32_t)lane];
            b.buf = 0; b.cnt = 0;
            refill(b, lane);
            drop(b, (int)(bp & 31u));
        } else {
        refill(b, lane);
        uint32_t e = uni(L.lit[peek(b, kLitBits)]);
        do {
            if (__builtin_expect((e & 15u) == 0, 0)) {
                const int sym = slow_symbol(b, L.lcount, L.lsym);
                e = sym < 0 ? (3u << 4) : make_entry<0>((uint32_t)sym);
            } else drop(b, (int)(e & 15u));
            const uint32_t kind = (e >> 4) & 3u;
            if (kind == 0) {
                const uint32_t byte = e >> 8;
                refill(b, lane);
                const uint32_t ev = L.lit[peek(b, kLitBits)];   // (made uniform after the store: the read is in flight meanwhile)
                L.out[pos & kRingMask] = (uint8_t)byte;         // (every lane stores the same byte to the same address)
                pos += 1;
                e = uni(ev);
            } else if (kind == 1) {
                const int xb = (int)((e >> 20) & 7u);
                const uint32_t len = ((e >> 8) & 511u) + peek(b, xb);
                drop(b, xb);
                refill(b, lane);
                uint32_t d = uni(L.dist[peek(b, kDistBits)]);
                if (__builtin_expect((d & 15u) == 0, 0)) {
                    const int sym = slow_symbol(b, L.dcount, L.dsym);
                    d = sym < 0 ? (15u << 4) : make_entry<1>((uint32_t)sym);
                } else drop(b, (int)(d & 15u));
                const int dx = (int)((d >> 4) & 15u);
                const uint32_t dist = (d >> 8) + peek(b, dx);
                drop(b, dx);
                const bool inside = (dx != 15) & (dist <= pos - sh) & (dist != 0);
                bad |= inside ? 0u : kBadDistance;
                refill(b, lane);
                const uint32_t ev = L.lit[peek(b, kLitBits)];   // the next symbol's entry: in flight while the bytes are copied
                copy_match(L, gbase, pos, dist, len, inside, lane);
                pos += len;
                e = uni(ev);
            } else {
                done = true;   // 2: end of block
                bad |= kind == 3 ? kBadSymbol : 0u;
            }
            if (__builtin_expect(pos >= next_stop, 0)) {
                if (pos > lim) { bad |= kBadOutput; done = true; }
                else if (bad) done = true;
                else if (bits_used_end(b) > in_end + 8) { bad |= kBadInput; done = true; }
                else if (pos - flushed >= kFlush + 512) { const uint32_t to = pos & ~(kFlush - 1); flush_ring(L, gbase, flushed, to, lane); flushed = to; }
                next_stop = flushed + kFlush + 512 < lim + 1 ? flushed + kFlush + 512 : lim + 1;
            }
        } while (!done);
        }
        if (pos > lim) bad |= kBadOutput;
        if (bad) err = (bad & kBadDistance) ? INFL_BAD_DISTANCE : (bad & kBadSymbol) ? INFL_BAD_SYMBOL : (bad & kBadOutput) ? INFL_OUTPUT_OVERRUN : INFL_INPUT_OVERRUN;
        if (err == INFL_OK && bits_used_end(b) > in_end) err = INFL_INPUT_OVERRUN;
    }
    if (err == INFL_OK && pos != lim) err = INFL_SIZE_MISMATCH;
    if (err == INFL_OK && pos > flushed) flush_ring(L, gbase, flushed, pos, lane);
    if (lane == 0) status[blk] = err;
}

// ---- CRC32 of every inflated member against its trailer (RFC 1952 2.3.1; htslib checks it per block: bgzf.c inflate_block /
// bgzf_read_block "CRC32 checksum mismatch", the reader behind the reference's bcf::Reader, calling.rs:306-318).  A flipped bit in a
// literal or a stored byte decodes to another valid stream of the same length: without this check it would end in wrong pileups.
// One wave per member.  Lane 0 takes the first n - 63 C bytes, lanes 1..63 C bytes each (C: the multiple of four below n / 64), sixteen
// bytes per load, slicing-by-4 through tables in LDS (4 KiB); the lane values are combined like zlib's crc32_combine:
// crc(A || B) = crc(A) x^(8 |B|) mod P  xor  crc(B), along a binary tree whose right-hand lengths are C, 2 C, 4 C, ...
constexpr uint32_t kCrcPoly = 0xedb88320u;   // reflected CRC-32 (IEEE 802.3)
// a(x) b(x) mod P in the reflected representation (zlib crc32.c multmodp)
__host__ __device__ constexpr uint32_t crc_multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
struct CrcX2n { uint32_t v[32]; };   // x^(2^n) mod P
constexpr CrcX2n crc_x2n_table() {
    CrcX2n t{};
    uint32_t p = 1u << 30;   // x^1
    t.v[0] = p;
    for (int n = 1; n < 32; ++n) { p = crc_multmodp(p, p); t.v[n] = p; }
    return t;
}
__device__ constexpr CrcX2n kCrcX2n = crc_x2n_table();
// x^(n 2^k) mod P (zlib x2nmodp)
__device__ __forceinline__ uint32_t crc_x2nmodp(uint32_t n, unsigned k) {
    uint32_t p = 1u << 31;   // x^0
    while (n) {
        if (n & 1u) p = crc_multmodp(kCrcX2n.v[k & 31u], p);
        n >>= 1;
        ++k;
    }
    return p;
}
struct __attribute__((packed, aligned(1))) CrcQuad { uint32_t w[4]; };
__global__ void __launch_bounds__(64) vlr_crc_kernel(const uint8_t* __restrict__ out, const InflateBlock* __restrict__ blocks, int n_blocks, int* __restrict__ status) {
    __shared__ uint32_t T[4][256];
    const int lane = threadIdx.x;
    const int blk = blockIdx.x;
    if (blk >= n_blocks) return;
    for (int i = lane; i < 256; i += 64) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        T[0][i] = c;
    }
    __syncthreads();
    for (int i = lane; i < 256; i += 64) {
        uint32_t c = T[0][i];
        for (int t = 1; t < 4; ++t) { c = T[0][c & 0xffu] ^ (c >> 8); T[t][i] = c; }
    }
    __syncthreads();
    const uint32_t n = blocks[blk].isize;
    const uint32_t C = (n >> 6) & ~3u;
    const uint32_t first = n - 63u * C;                      // lane 0's share (C .. C + 255 bytes)
    const uint32_t len = lane == 0 ? first : C;
    const uint8_t* g = out + blocks[blk].dst + (lane == 0 ? 0u : first + (uint32_t)(lane - 1) * C);
    uint32_t c = 0xffffffffu;
    uint32_t i = 0;
    for (; i + 16 <= len; i += 16) {
        const CrcQuad q = *(const CrcQuad*)(g + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c ^= q.w[j];
            c = T[3][c & 0xffu] ^ T[2][(c >> 8) & 0xffu] ^ T[1][(c >> 16) & 0xffu] ^ T[0][c >> 24];
        }
    }
    for (; i < len; ++i) c = T[0][(c ^ g[i]) & 0xffu] ^ (c >> 8);
    c = ~c;                                                  // the finished CRC of the lane's piece (of nothing: 0)
    // tree: at level k the left neighbour's value moves over 2^k C bytes
    uint32_t X = crc_x2nmodp(C, 3);                          // x^(8 C)
    for (int k = 0; k < 6; ++k) {
        const uint32_t right = (uint32_t)__shfl_down((int)c, 1 << k, 64);
        if ((lane & ((2 << k) - 1)) == 0) c = crc_multmodp(X, c) ^ right;
        X = crc_multmodp(X, X);
    }
    if (lane == 0 && status[blk] == INFL_OK && c != blocks[blk].crc) status[blk] = INFL_CRC_MISMATCH;
}

}  // namespace
}  // namespace vlr

extern "C" int vlr_launch_inflate_kernel(const uint8_t* d_comp, const vlr::InflateBlock* d_blocks, int n_blocks, uint8_t* d_out, int* d_status, void* stream) {
    if (n_blocks <= 0) return 0;
    // VLR_INFLATE_BATCH=1: speculative batches of 64 candidate symbol starts; 0: one symbol at a time (read per launch: the tests run both)
    const char* env = getenv("VLR_INFLATE_BATCH");
    const bool batch = env ? atoi(env) != 0 : vlr::kInflateBatchDefault;
    if (batch) hipLaunchKernelGGL(vlr::vlr_inflate_kernel<true>, dim3((unsigned)n_blocks), dim3(64), 0, (hipStream_t)stream, d_comp, d_blocks, n_blocks, d_out, d_status);
    else hipLaunchKernelGGL(vlr::vlr_inflate_kernel<false>, dim3((unsigned)n_blocks), dim3(64), 0, (hipStream_t)stream, d_comp, d_blocks, n_blocks, d_out, d_status);
    // the members' CRC32 against their trailers, behind the inflate in stream order (VLR_INFLATE_CRC=0: measurement only)
    const char* ce = getenv("VLR_INFLATE_CRC");
    if (!ce || atoi(ce) != 0) hipLaunchKernelGGL(vlr::vlr_crc_kernel, dim3((unsigned)n_blocks), dim3(64), 0, (hipStream_t)stream, d_out, d_blocks, n_blocks, d_status);
    return (int)hipGetLastError();
}
