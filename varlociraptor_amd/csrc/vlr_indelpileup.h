// vlr_indelpileup.h — per-(record, locus) evidence of indel candidates from a BAM record: which loci a record is evidence for, the read
// window and the ref allele window of each, and the bytes of those windows.  The text the kernels of vlr_indelpileup.hip and the host
// translation unit vlr_indelpileup_host.cpp (built with the sanitizers by tests/test_indelpileup_host.py) both compile.  Plain C++: no
// HIP types, no library calls.
//
// Restates rust-htslib's CigarStringView::read_pos(pos, include_softclips, include_dels), SingleLocus::overlap with soft clips
// (variants/types/mod.rs) as varlociraptor_amd/readwindows.py `overlaps` has it, and Realigner::candidate_region
// (variants/evidence/realignment/mod.rs:58-153); varlociraptor_amd/readwindows.py `evidence` is the same in Python.  The record decode,
// its bounds checks and the flag rule (variants/sample.rs:281-286) are vlr_bp::decode of vlr_basepileup.h.
//
// Bounds: vlr_bp::decode is the only function that looks at a record before its lengths are known (see vlr_basepileup.h); only a
// record it accepts is followed, and everything here reads CIGAR words below n_cigar and bases / qualities below l_seq — `window_byte`
// checks the index against l_seq again.  Every index into a contig is checked against the contig's length (`window_byte`), and the
// intervals `candidate_region` returns lie inside [0, l_seq] and [0, contig length].
#ifndef VLR_INDELPILEUP_H
#define VLR_INDELPILEUP_H

#include <stdint.h>

#include "vlr_basepileup.h"

namespace vlr_ip {

using vlr_bp::ld32;
using vlr_bp::lower_bound;
using vlr_bp::Rec;
using vlr_bp::RecClass;
using vlr_bp::REC_BAD;
using vlr_bp::REC_OK;
using vlr_bp::REC_REJECTED;
using vlr_bp::RP_ERROR;
using vlr_bp::RP_NONE;

constexpr int64_t kMaxPatternLen = 128;   // edit_distance.rs:145-147

struct Loci {
    int64_t n;
    const int32_t* ref_id;      // sorted by (ref_id, start)
    const int64_t* start;
    const int64_t* end;         // exclusive
    const uint64_t* alt_off;    // [n + 1]: the alt allele window of locus k is alt_bases[alt_off[k] .. alt_off[k + 1])
    int64_t max_locus_len;      // largest end - start: how far in front of an alignment a locus that reaches it can start
    int64_t n_refs;             // contigs of the BAM header
    const int64_t* ctg_len;     // [n_refs] length of the contig in the reference; -1: not loaded (no locus lies on it)
};

VLR_BP_HD inline int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
VLR_BP_HD inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// CigarStringView::read_pos(ref_pos, include_softclips, include_dels): the read position aligned to ref_pos, RP_NONE, or RP_ERROR for a
// CIGAR that begins with a reference skip.  Leading deletions move the start, hard clips and pads consume nothing, a leading soft
// clip that is included moves the start back (not below 0), and a position inside a deletion projects to the read position at which
// the deletion starts.
VLR_BP_HD inline int64_t read_pos(const Rec& r, int64_t ref_pos, bool include_softclips, bool include_dels) {
    const uint8_t* c = r.p + r.cig_off;
    const uint32_t n = r.n_cigar;
    int64_t rpos = r.pos, qpos = 0;
    uint32_t j = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t v = ld32(c + 4u * i), op = v & 15u, l = v >> 4;
        if (op == 0 || op == 7 || op == 8 || op == 1) { j = i; break; }
        if (op == 4) {
            j = i;
            if (include_softclips) rpos = max64(0, rpos - (int64_t)l);
            break;
        }
        if (op == 2) rpos += l;
        else if (op == 3) return RP_ERROR;
        else if (i == n - 1) return RP_NONE;   // H, P
    }
    while (rpos <= ref_pos && j < n) {
        const uint32_t v = ld32(c + 4u * j), op = v & 15u, l = v >> 4;
        const bool inside = ref_pos < rpos + (int64_t)l;
        if (op == 0 || op == 7 || op == 8) {
            if (inside) return qpos + (ref_pos - rpos);
            rpos += l; qpos += l;
        } else if (op == 4) {
            if (include_softclips && inside) return qpos + (ref_pos - rpos);
            qpos += l;
            if (include_softclips) rpos += l;
        } else if (op == 1) qpos += l;
        else if (op == 2) {
            if (include_dels && inside) return qpos;
            rpos += l;
        } else if (op == 3) rpos += l;
        else if (op == 5 && j == n - 1) return RP_NONE;
        ++j;
    }
    return RP_NONE;
}

// the alignment with its soft clips shares a position with [start, end) (readwindows.overlaps: a clip counts when it is the first /
// the last operation of the CIGAR)
VLR_BP_HD inline bool overlaps(const Rec& r, int64_t start, int64_t end) {
    int64_t lead = 0, trail = 0;
    if (r.n_cigar > 0) {
        const uint32_t v = ld32(r.p + r.cig_off);
        if ((v & 15u) == 4) lead = v >> 4;
    }
    if (r.n_cigar > 1) {
        const uint32_t v = ld32(r.p + r.cig_off + 4u * (r.n_cigar - 1));
        if ((v & 15u) == 4) trail = v >> 4;
    }
    return r.pos - lead < end && r.end_pos + trail > start;
}

struct Region {
    bool error;      // read_pos failed (leading reference skip)
    bool overlap;
    int64_t read_begin, read_end, ref_begin, ref_end;
};

// Realigner::candidate_region (mod.rs:58-153); window = --realignment-window, ref window = window * 3 / 2 (== int(window * 1.5))
VLR_BP_HD inline Region candidate_region(const Rec& r, int64_t locus_start, int64_t locus_end, int64_t contig_len, int64_t window) {
    Region g = {false, true, 0, 0, 0, 0};
    const int64_t ref_window = window * 3 / 2;
    const int64_t seq_len = (int64_t)r.l_seq;
    const int64_t qs = read_pos(r, locus_start, true, true);
    const int64_t qe = qs == RP_ERROR ? (int64_t)RP_ERROR : read_pos(r, locus_end, true, true);
    if (qs == RP_ERROR || qe == RP_ERROR) { g.error = true; g.overlap = false; return g; }
    int64_t breakpoint = locus_start;
    if (qs >= 0 && qe >= 0) {            // the read encloses the variant
        const int64_t max_window = max64(0, window - (qe - qs) / 2);
        g.read_begin = max64(0, qs - max_window);
        g.read_end = min64(qe + max_window, seq_len);
        const int64_t exceed = max64(0, (g.read_end - g.read_begin) - kMaxPatternLen);
        if (exceed > 0) {
            g.read_begin += exceed / 2;
            g.read_end -= (exceed + 1) / 2;   // ceil(exceed / 2)
        }
    } else if (qs >= 0) {                // the read overlaps from the right
        g.read_begin = max64(0, qs - window);
        g.read_end = min64(qs + window, seq_len);
    } else if (qe >= 0) {                // the read overlaps from the left
        g.read_begin = max64(0, qe - window);
        g.read_end = min64(qe + window, seq_len);
        breakpoint = locus_end;
    } else {                             // neither end: evidence only when the read lies inside the variant (a long deletion)
        const int64_t m = seq_len / 2;
        g.read_begin = max64(0, m - window);
        g.read_end = min64(m + window - 1, seq_len);
        breakpoint = r.pos + m;
        g.overlap = r.pos >= locus_start && r.end_pos <= locus_end;
    }
    g.ref_end = max64(0, min64(breakpoint + ref_window, contig_len));
    g.ref_begin = min64(max64(0, breakpoint - ref_window), g.ref_end);
    g.read_end = max64(g.read_end, g.read_begin);
    return g;
}

// Byte k of a window.  WB_READ_BASE: base begin + k of the 4-bit SEQ at src (src_len = l_seq), decoded — upper case by construction;
// WB_READ_QUAL: quality begin + k of QUAL at src (src_len = l_seq); WB_REF_BASE: base begin + k of the upper-cased contig at src
// (src_len = its length).  An index outside [0, src_len) reads nothing and gives 'N' (0 for a quality).
enum { WB_READ_BASE = 0, WB_READ_QUAL = 1, WB_REF_BASE = 2 };
VLR_BP_HD inline uint8_t window_byte(int what, const uint8_t* src, int64_t src_len, int64_t begin, uint32_t k) {
    const int64_t i = begin + (int64_t)k;
    if (i < 0 || i >= src_len) return what == WB_READ_QUAL ? (uint8_t)0 : (uint8_t)'N';
    if (what == WB_READ_BASE) {
        const uint32_t b = src[i >> 1];
        return (uint8_t)"=ACMGRSVTWYHKDBN"[(i & 1) ? (b & 15u) : (b >> 4)];
    }
    return src[i];
}

struct RecEvidence {
    uint32_t n_ev;               // evidences of the record
    uint64_t x_bytes, y_bytes;   // bytes of their pairs: allele windows (ref + alt), read windows (twice: one per pair)
    RecClass cls;
    uint32_t seq_off, qual_off, l_seq;   // of an accepted record: where its packed SEQ and its QUAL start
};

// Everything one record gives: its evidences, loci ascending, written to out[0 .. room) when out != nullptr (evidences behind `room`
// are counted, not written; scores and distances are left zero / -1 for the collect pass).  The count pass (out == nullptr) and the
// fill pass run the same text.
VLR_BP_HD inline RecEvidence record_evidence(const Loci& L, const uint8_t* p, uint64_t size, uint64_t ordinal, int64_t window, vlr_indelpileup_hit* out,
                                             uint64_t room) {
    RecEvidence res = {0u, 0ull, 0ull, REC_OK, 0u, 0u, 0u};
    Rec r;
    res.cls = vlr_bp::decode(p, size, r);
    if (res.cls != REC_OK || r.ref_id < 0 || r.pos < 0 || (int64_t)r.ref_id >= L.n_refs) return res;
    res.seq_off = r.seq_off; res.qual_off = r.qual_off; res.l_seq = r.l_seq;
    const int64_t contig_len = L.ctg_len[r.ref_id];
    if (contig_len < 0) return res;
    // the alignment with its clips is inside [pos - l_seq, end_pos + l_seq): loci that start at or behind its end cannot overlap, loci that
    // start more than max_locus_len in front of it cannot reach it
    const int64_t lo = r.pos - (int64_t)r.l_seq, hi = r.end_pos + (int64_t)r.l_seq;
    for (int64_t li = lower_bound(L, r.ref_id, lo - L.max_locus_len); li < L.n && L.ref_id[li] == r.ref_id && L.start[li] < hi; ++li) {
        const int64_t ls = L.start[li], le = L.end[li];
        if (!overlaps(r, ls, le)) continue;
        const Region g = candidate_region(r, ls, le, contig_len, window);
        vlr_indelpileup_hit h;
        h.ln_ref = 0.0; h.ln_alt = 0.0;
        h.record = ordinal;
        h.ref_begin = 0;
        h.locus = (uint32_t)li;
        h.ref_len = 0; h.read_begin = 0; h.read_len = 0;
        h.dist_ref = -1; h.dist_alt = -1;
        h.flag = (uint16_t)(r.flag & (0x1u | 0x10u | 0x40u));
        h.mapq = (uint8_t)r.mapq;
        h.status = 0;
        for (int k = 0; k < 4; ++k) h.pad[k] = 0;
        if (g.error) h.status = VLR_INDELPILEUP_HIT_LEADING_REFSKIP;
        else if (!g.overlap) h.status = VLR_INDELPILEUP_HIT_NO_OVERLAP;
        else {
            if (g.read_end - g.read_begin < 1) continue;
            h.ref_begin = g.ref_begin;
            h.ref_len = (uint32_t)(g.ref_end - g.ref_begin);
            h.read_begin = (uint32_t)g.read_begin;
            h.read_len = (uint32_t)(g.read_end - g.read_begin);
            res.x_bytes += (uint64_t)h.ref_len + (L.alt_off[li + 1] - L.alt_off[li]);
            res.y_bytes += 2ull * h.read_len;
        }
        if (out != nullptr && (uint64_t)res.n_ev < room) out[res.n_ev] = h;
        ++res.n_ev;
    }
    return res;
}

}  // namespace vlr_ip

#endif
