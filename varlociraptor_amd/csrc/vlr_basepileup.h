// vlr_basepileup.h — per-(record, locus) scoring of SNV / MNV candidates from a BAM record: the text the kernel of vlr_basepileup.hip and
// the host translation unit vlr_basepileup_host.cpp (built with the sanitizers by tests/test_basepileup_host.py) both compile.  Plain
// C++: no HIP types, no library calls in the scoring functions.
//
// Restates the no-realignment branch of Snv::allele_support_per_read (variants/types/snv.rs:66-150) and Mnv::allele_support_per_read
// (variants/types/mnv.rs:73-205) with prob_read_base (variants/evidence/bases.rs), SingleLocus::overlap without clips
// (variants/types/mod.rs:440-473), rust-htslib's CigarStringView::read_pos(pos, false, false), the record filter of
// variants/sample.rs:281-286 and the strand rules of read_observation.rs:60-122; varlociraptor_amd/basecalls.py is the same in Python.
//
// Bounds: `decode` is the only function that looks at a record before its lengths are known.  It checks the 36 bytes of the fixed
// head against the record's size, block_size against that size, l_read_name / n_cigar_op / l_seq against block_size, every CIGAR
// operation code, the number of read bases the CIGAR consumes against l_seq, and walks the aux fields with every length checked.
// Only a record it accepts is scored, and the scoring reads CIGAR words below n_cigar, bases and qualities below l_seq and SI
// characters below the tag's length — all inside [p, p + size).  A record it refuses is reported and never followed.
//
// MNV sums are sequential f64 additions in locus order, starting from ln 1 = 0.0, as in the reference.  `explainable`
// (edit_distance.rs:31-47 with pairhmm.rs:436-451) compares the edit distance with len * mean miscall rate of the read; the mean is
// taken here as sum(10^(-q/10)) / l_seq from a table, in read order, where the reference takes exp(ln_sum_exp(miscall) - ln l_seq):
// the two differ by a few ulp, which matters only when the edit distance equals the expectation to that precision (it is an integer
// >= 1 against len * rate with rate < 1: tests keep half a unit away from it).
#ifndef VLR_BASEPILEUP_H
#define VLR_BASEPILEUP_H

#include <stdint.h>

#include "../../include/vlr.h"

#if defined(__HIPCC__)
#define VLR_BP_HD __host__ __device__
#else
#define VLR_BP_HD
#endif

namespace vlr_bp {

struct Tables {
    const double* call;      // [256] ln(1 - 10^(-q/10))
    const double* miscall;   // [256] -q ln(10) / 10
    const double* linear;    // [256] 10^(-q/10)
    double confusion, any;   // ln 0.3333, ln 0.25
};

struct Loci {
    int64_t n;
    const int32_t* ref_id;     // sorted by (ref_id, start)
    const int64_t* start;
    const int32_t* len;
    const uint8_t* kind;       // VLR_BASEPILEUP_SNV / _MNV
    const uint64_t* base_off;  // offset of the locus' alleles in ref_bases / alt_bases
    const uint8_t* ref_bases;
    const uint8_t* alt_bases;
};

enum RecClass { REC_OK = 0, REC_REJECTED = 1, REC_BAD = 2 };
enum { STRAND_FORWARD = 0, STRAND_REVERSE = 1, STRAND_BOTH = 2, STRAND_NONE = 3 };

struct Rec {
    const uint8_t* p;
    int32_t ref_id;
    int64_t pos, end_pos;
    uint32_t n_cigar, l_seq, flag, mapq;
    uint32_t cig_off, seq_off, qual_off;
    uint32_t si_off, si_len;   // SI:Z characters at p + si_off (has_si)
    uint32_t lead_hard;
    bool has_si, has_indel;
};

VLR_BP_HD inline uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
VLR_BP_HD inline uint32_t ld32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// bytes of one aux value of type `t` at [o, size), or 0 when it is malformed (SAM spec 4.2.4)
VLR_BP_HD inline uint64_t aux_value_bytes(const uint8_t* p, uint64_t o, uint64_t size, uint32_t t) {
    switch (t) {
        case 'A': case 'c': case 'C': return 1;
        case 's': case 'S': return 2;
        case 'i': case 'I': case 'f': return 4;
        case 'Z': case 'H': {
            for (uint64_t k = o; k < size; ++k) if (p[k] == 0) return k - o + 1;
            return 0;
        }
        case 'B': {
            if (o + 5 > size) return 0;
            const uint32_t sub = p[o];
            const uint64_t n = ld32(p + o + 1);
            const uint64_t w = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
            return w ? 5 + w * n : 0;
        }
        default: return 0;
    }
}

// the record at [p, p + size): `size` covers the block_size word and everything the split gave the record
VLR_BP_HD inline RecClass decode(const uint8_t* p, uint64_t size, Rec& r) {
    if (size < 36) return REC_BAD;
    const uint64_t bs = ld32(p);
    if (bs + 4 != size) return REC_BAD;
    const uint32_t l_rn = p[12];
    r.p = p;
    r.ref_id = (int32_t)ld32(p + 4);
    r.pos = (int64_t)(int32_t)ld32(p + 8);
    r.mapq = p[13];
    r.n_cigar = ld16(p + 16);
    r.flag = ld16(p + 18);
    const int32_t l_seq = (int32_t)ld32(p + 20);
    if (l_seq < 0 || l_rn < 1) return REC_BAD;
    r.l_seq = (uint32_t)l_seq;
    const uint64_t fixed = 32ull + l_rn + 4ull * r.n_cigar + ((uint64_t)r.l_seq + 1) / 2 + (uint64_t)r.l_seq;
    if (fixed > bs) return REC_BAD;
    r.cig_off = 36u + l_rn;
    r.seq_off = r.cig_off + 4u * r.n_cigar;
    r.qual_off = r.seq_off + (r.l_seq + 1) / 2;
    // sample.rs:281-286: secondary, duplicate, unmapped and QC-fail records are no evidence (supplementary ones are)
    if (r.flag & (0x100u | 0x400u | 0x4u | 0x200u)) return REC_REJECTED;
    // CIGAR: operation codes, reference and read extent
    int64_t ref_len = 0;
    uint64_t query_len = 0;
    r.has_indel = false;
    r.lead_hard = 0;
    for (uint32_t k = 0; k < r.n_cigar; ++k) {
        const uint32_t v = ld32(p + r.cig_off + 4u * k);
        const uint32_t op = v & 15u, l = v >> 4;
        if (op > 8) return REC_BAD;
        if (op == 0 || op == 7 || op == 8) { ref_len += l; query_len += l; }
        else if (op == 2 || op == 3) ref_len += l;
        else if (op == 1 || op == 4) query_len += l;
        if (op == 1 || op == 2) r.has_indel = true;
        if (k == 0 && op == 5) r.lead_hard = l;
    }
    if (query_len > (uint64_t)r.l_seq) return REC_BAD;   // a read position past the bases (the reference reads unchecked there)
    r.end_pos = r.pos + ref_len;
    // aux fields: every length checked; the first SI field counts, as a strand string when its type is Z
    r.has_si = false;
    r.si_off = r.si_len = 0;
    uint64_t o = 4 + fixed;
    bool seen_si = false;
    while (o < size) {
        if (o + 3 > size) return REC_BAD;
        const uint32_t t0 = p[o], t1 = p[o + 1], ty = p[o + 2];
        const uint64_t nb = aux_value_bytes(p, o + 3, size, ty);
        if (nb == 0 || o + 3 + nb > size) return REC_BAD;
        if (t0 == 'S' && t1 == 'I' && !seen_si) {
            seen_si = true;
            if (ty == 'Z') { r.has_si = true; r.si_off = (uint32_t)(o + 3); r.si_len = (uint32_t)(nb - 1); }
        }
        o += 3 + nb;
    }
    return REC_OK;
}

enum { RP_NONE = -1, RP_ERROR = -2 };

// CigarStringView::read_pos(ref_pos, include_softclips = false, include_dels = false): the read position aligned to ref_pos, RP_NONE, or
// RP_ERROR for a CIGAR that begins with a reference skip
VLR_BP_HD inline int64_t read_pos(const Rec& r, int64_t ref_pos) {
    const uint8_t* c = r.p + r.cig_off;
    const uint32_t n = r.n_cigar;
    int64_t rpos = r.pos, qpos = 0;
    uint32_t j = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t v = ld32(c + 4u * i), op = v & 15u, l = v >> 4;
        if (op == 0 || op == 7 || op == 8 || op == 1 || op == 4) { j = i; break; }
        if (op == 2) rpos += l;
        else if (op == 3) return RP_ERROR;
        else if (i == n - 1) return RP_NONE;   // H, P
    }
    while (rpos <= ref_pos && j < n) {
        const uint32_t v = ld32(c + 4u * j), op = v & 15u, l = v >> 4;
        if (op == 0 || op == 7 || op == 8) {
            if (ref_pos < rpos + (int64_t)l) return qpos + (ref_pos - rpos);
            rpos += l; qpos += l;
        } else if (op == 4 || op == 1) qpos += l;
        else if (op == 2 || op == 3) rpos += l;
        else if (op == 5 && j == n - 1) return RP_NONE;
        ++j;
    }
    return RP_NONE;
}

VLR_BP_HD inline uint32_t read_base(const Rec& r, uint32_t i) {   // decoded, upper case by construction
    const uint32_t b = r.p[r.seq_off + (i >> 1)];
    return (uint32_t)(uint8_t)"=ACMGRSVTWYHKDBN"[(i & 1u) ? (b & 15u) : (b >> 4)];
}

// bases.rs:14-26 (both bases upper case here)
VLR_BP_HD inline double prob_read_base(const Tables& t, uint32_t rb, uint32_t allele, uint32_t q) {
    if (rb == allele) return t.call[q];
    if (rb == 'N') return t.any;
    return t.miscall[q] + t.confusion;
}

// Strand::from_aux_item; 4 = invalid
VLR_BP_HD inline uint32_t strand_of_item(uint32_t ch) {
    return ch == '+' ? STRAND_FORWARD : ch == '-' ? STRAND_REVERSE : ch == '*' ? STRAND_BOTH : ch == '.' ? STRAND_NONE : 4u;
}
VLR_BP_HD inline uint32_t strand_or(uint32_t a, uint32_t b) {   // BitOrAssign for Strand
    if (a == STRAND_NONE) return b;
    if (b == STRAND_NONE) return a;
    return a != b ? (uint32_t)STRAND_BOTH : a;
}

// One enclosed locus of an accepted record: true = a hit (scored, or flagged), false = no observation
VLR_BP_HD inline bool score(const Tables& t, const Loci& L, int64_t li, const Rec& r, uint64_t ordinal, bool realign_indel_reads, vlr_basepileup_hit& h) {
    h.prob_ref = 0.0; h.prob_alt = 0.0;
    h.record = ordinal;
    h.locus = (uint32_t)li;
    h.read_position = VLR_BASEPILEUP_NO_READ_POSITION;
    h.third_allele = 0;
    h.flag = (uint16_t)(r.flag & (0x1u | 0x10u | 0x40u));
    h.strand = STRAND_NONE;
    h.mapq = (uint8_t)r.mapq;
    h.status = 0;
    for (int k = 0; k < 7; ++k) h.pad[k] = 0;
    if (realign_indel_reads && r.has_indel) { h.status = VLR_BASEPILEUP_HIT_NEEDS_REALIGN; return true; }
    const int64_t start = L.start[li];
    const uint32_t len = (uint32_t)L.len[li];
    const uint8_t* refb = L.ref_bases + L.base_off[li];
    const uint8_t* altb = L.alt_bases + L.base_off[li];
    const uint32_t rec_strand = (r.flag & 0x10u) ? STRAND_REVERSE : STRAND_FORWARD;
    if (L.kind[li] == VLR_BASEPILEUP_SNV) {
        const int64_t qp = read_pos(r, start);
        if (qp == RP_ERROR) { h.status = VLR_BASEPILEUP_HIT_LEADING_REFSKIP; return true; }
        if (qp < 0) return false;
        const uint32_t qpos = (uint32_t)qp;
        const uint32_t rb = read_base(r, qpos), q = r.p[r.qual_off + qpos], alt = altb[0], ref = refb[0];
        const double pa = prob_read_base(t, rb, alt, q);
        uint32_t non_alt = ref;
        bool third = false;
        if (rb != 'N' && rb != alt) { third = rb != ref; non_alt = rb; }
        const double pr = prob_read_base(t, rb, non_alt, q);
        h.prob_ref = pr; h.prob_alt = pa;
        h.read_position = qpos + r.lead_hard;
        h.third_allele = third ? 1u : 0u;
        if (pr != pa) {
            if (r.has_si) {
                if (qpos >= r.si_len) { h.status = VLR_BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS; return true; }
                const uint32_t s = strand_of_item(r.p[r.si_off + qpos]);
                if (s > 3u) { h.status = VLR_BASEPILEUP_HIT_INVALID_STRAND_INFO; return true; }
                h.strand = (uint8_t)s;
            } else h.strand = (uint8_t)rec_strand;
        }
        return true;
    }
    double pr = 0.0, pa = 0.0, pt = 0.0;
    uint32_t strand = STRAND_NONE, dist = 0;
    for (uint32_t b = 0; b < len; ++b) {
        const int64_t qp = read_pos(r, start + (int64_t)b);
        if (qp == RP_ERROR) { h.status = VLR_BASEPILEUP_HIT_LEADING_REFSKIP; return true; }
        if (qp < 0) return false;
        const uint32_t qpos = (uint32_t)qp;
        if (b == 0) h.read_position = qpos + r.lead_hard;
        const uint32_t rb = read_base(r, qpos), q = r.p[r.qual_off + qpos], alt = altb[b], ref = refb[b];
        if (rb != 'N' && rb != alt) ++dist;
        const double ba = prob_read_base(t, rb, alt, q), br = prob_read_base(t, rb, ref, q), bt = prob_read_base(t, rb, rb, q);
        if (ba != br && r.has_si) {
            if (qpos >= r.si_len) { h.status = VLR_BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS; return true; }
            const uint32_t s = strand_of_item(r.p[r.si_off + qpos]);
            if (s > 3u) { h.status = VLR_BASEPILEUP_HIT_INVALID_STRAND_INFO; return true; }
            strand = strand_or(strand, s);
        }
        pr += br; pa += ba; pt += bt;
    }
    if (pa > pr && dist > 0) {
        // is_explainable_by_error_rates: the insertion / deletion terms are 0 <= x and always hold
        double sum = 0.0;
        for (uint32_t j = 0; j < r.l_seq; ++j) sum += t.linear[r.p[r.qual_off + j]];
        const double rate = sum / (double)r.l_seq;
        const bool explainable = (double)dist <= (double)len * rate;
        if (!explainable) { pr = pt; h.third_allele = dist; }
    }
    if (!r.has_si && pr != pa) strand = rec_strand;
    h.prob_ref = pr; h.prob_alt = pa;
    h.strand = (uint8_t)strand;
    return true;
}

// first locus at or behind (ref_id, pos) in the sorted loci (any Loci with n, ref_id and start: also vlr_ip::Loci)
template <class L_>
VLR_BP_HD inline int64_t lower_bound(const L_& L, int32_t ref_id, int64_t pos) {
    int64_t lo = 0, hi = L.n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        const bool less = L.ref_id[mid] < ref_id || (L.ref_id[mid] == ref_id && L.start[mid] < pos);
        if (less) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct RecResult { uint32_t n_hits, n_needs_realign; RecClass cls; };

// Everything one record gives: its hits, loci ascending, written to out[0 .. room) when out != nullptr (hits behind `room` are
// counted, not written).  The count pass (out == nullptr) and the fill pass run the same text.
VLR_BP_HD inline RecResult record_hits(const Tables& t, const Loci& L, const uint8_t* p, uint64_t size, uint64_t ordinal, bool realign_indel_reads,
                                       vlr_basepileup_hit* out, uint64_t room) {
    RecResult res = {0u, 0u, REC_OK};
    Rec r;
    res.cls = decode(p, size, r);
    if (res.cls != REC_OK || r.ref_id < 0 || r.pos < 0) return res;
    // Enclosing: pos <= start && end_pos >= start + len
    for (int64_t li = lower_bound(L, r.ref_id, r.pos); li < L.n && L.ref_id[li] == r.ref_id && L.start[li] < r.end_pos; ++li) {
        if (L.start[li] + (int64_t)L.len[li] > r.end_pos) continue;
        vlr_basepileup_hit h;
        if (!score(t, L, li, r, ordinal, realign_indel_reads, h)) continue;
        if (out != nullptr && (uint64_t)res.n_hits < room) out[res.n_hits] = h;
        if (h.status & VLR_BASEPILEUP_HIT_NEEDS_REALIGN) ++res.n_needs_realign;
        ++res.n_hits;
    }
    return res;
}

}  // namespace vlr_bp

#include <cmath>
namespace vlr_bp {
// (host side: the tables are computed once with the host's libm and uploaded)
// BASEQUAL_TO_PROB_MISCALL / _CALL of bases.rs:38-53 (LogProb::from(PHREDProb(q)), LogProb::ln_one_minus_exp) and 10^(-q/10)
inline void fill_tables(double* call, double* miscall, double* linear) {
    for (int q = 0; q < 256; ++q) {
        const double m = -(double)q * std::log(10.0) / 10.0;
        miscall[q] = m;
        call[q] = m < -0.693 ? std::log1p(-std::exp(m)) : std::log(-std::expm1(m));
        if (linear) linear[q] = std::pow(10.0, -(double)q / 10.0);
    }
}
inline double ln_confusion() { return std::log(0.3333); }
inline double ln_any() { return std::log(0.25); }
}  // namespace vlr_bp

#endif
