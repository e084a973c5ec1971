// vlr_fragpileup.h — fragments of SNV / MNV candidates from BAM records: the text the kernels of vlr_fragpileup.hip and the host
// translation unit vlr_fragpileup_host.cpp (built with the sanitizers by tests/test_fragpileup_host.py) both compile.  Plain C++: no HIP
// types, no library calls.  It reuses decode, the flag rule and the scoring of vlr_basepileup.h and adds
//   the window test          variants/sample.rs:96-108, 259-268: a record is a member of a locus when its START lies in
//                            [start - window, end).  The test is on the start alone: that is how rust-htslib's RecordBuffer::fetch (a
//                            crate that is not vendored with the reference) keeps records
//   the per-record features  Evidence::softclipped (read_observation.rs:774-790; leading_softclips / trailing_softclips of rust-htslib skip
//                            one hard clip), read_orientation (:131-159; RO:Z or rust-htslib's read_pair_orientation from the flags),
//                            the XA:Z walk (ExactAltLoci::from, :167-210): entries with exactly four items, one leading '-' of the
//                            position stripped, the position parsed as Rust parses a u64, every byte read below the value's own
//                            length; an entry becomes the key (64-bit FNV-1a of the contig bytes, bucket position) with the bucket of
//                            locus_to_bucket (:593-605).  Two contig names that collide in 64 bits would be merged
//   the pairing rule         variants/types/mod.rs:325-338 over a run of members with one QNAME in record order
//   validity and the merge   mod.rs:352-384, snv.rs:186-242, mnv.rs:242-270, AlleleSupport::merge (mod.rs:104-160)
//   the observation fields   read_observation.rs:644-670, mod.rs:255-281
//   calc_major_feature       read_observation.rs:498-527 over sorted values (read positions, alt-locus keys) and the alt-locus class of
//                            ReadObservation::process (:338-350)
//   the realignment          snv.rs:72-86, mnv.rs:83 with Realigner::allele_support (realignment/mod.rs:161-424): a record that encloses
//                            the locus and carries an I or D operation is not scored from its alignment but realigned.  Here: its
//                            candidate region (vlr_ip::candidate_region, mod.rs:58-153) on [start, start + len), the ref allele window
//                            (the region's ref_interval) and the alt allele window of Snv / MnvEmissionParams (snv.rs:157-178,
//                            mnv.rs:224-233: [max(0, start - rw), min(start + len + rw, contig length)) with the locus bytes replaced,
//                            rw = window * 3 / 2, clamped on its own) as a vlr_indelpileup_hit (`realign_evidence`), and the
//                            normalisation of mod.rs:358-376 (`normalize_support`).  The strand is the record's when the normalised
//                            supports differ, else none (mod.rs:409-413); read position and third-allele evidence are none.
//                            NOT mirrored: the read-inferred third allele (mod.rs:317-348 needs the Myers traceback of the bio crate,
//                            which the reference does not vendor), homopolymer_indel_len.  alt_variants (the other alleles of the
//                            locus on the reference side, and mnv.rs:83's realignment of every enclosing record of an MNV that has
//                            one) is vlr_altvariants.h's, in a session with vlr_fragpileup_set_alt_variants.  Two inputs are refused, each with a status of its own: a
//                            CIGAR that begins with N (read_pos fails) and a record with an SI:Z tag (strand information over an
//                            interval, mod.rs:381-387).  A region without overlap or with an empty read window gives ln 0.5 / ln 0.5
//                            (mod.rs:186-199).
//   indel candidates         (an indel session, vlr_fragpileup_open_indel) deletion.rs:41-85, 158-197, insertion.rs:57-61, 139-157,
//                            Realigner::allele_support (mod.rs:161-424), insert_size.rs:17-45.  A locus is [start, end) of a deletion
//                            (REF longer than one base, ALT its first base: end - start deleted bases behind the anchor) or
//                            [start, start + 1) of an insertion, its alt allele window computed by the caller as for
//                            vlr_indelpileup_open (deletion.rs:120-141, insertion.rs:73-99).  A deletion is fetched at `start`,
//                            centerpoint = start + round(len / 2) (f64::round: half away from zero, `centerpoint`) and end - 1; only
//                            deletions whose three fetch loci merge into one fetch are given to a session (the caller refuses the
//                            others), so membership is the window test above on [start, end).  EVERY member of an indel locus is
//                            realigned (`realign_evidence` with the locus's own alt window; no overlap or an empty read window gives
//                            ln 0.5 / ln 0.5, strand none, VLR_INDELPILEUP_HIT_NO_OVERLAP); a CIGAR that begins with N and an SI:Z tag
//                            are refused as above.  A member carries M_OVERLAPS when SingleLocus::overlap(r, true, 0, 0) != None
//                            (vlr_ip::overlaps: with soft clips, on [start, end)) and a Side record beside it (pos, end_pos, the four
//                            clip lengths).  A fragment is valid (`make_obs_indel`): a single read when it overlaps; an insertion pair,
//                            or a deletion pair of a session without an insert size, when either read overlaps; a deletion pair with
//                            an insert size when left.pos < centerpoint && right.end_pos > centerpoint AND either read overlaps.  Its
//                            support is AlleleSupport::merge(left, right) (read position none, third allele 0); an observation exists
//                            only for a merged strand other than none (read_observation.rs:638-646) — the insert-size term, which
//                            the host adds (it needs libm), has strand none and never decides that.  `insert_size` (insert_size.rs:
//                            17-45): per read (pos - leading soft - leading hard, saturating at 0; end_pos + trailing soft + trailing
//                            hard), inner distance + both spans; a value <= 0 is the reference's assertion and comes back flagged.
//                            `cigar_maxima`: the longest D, the longest I and the largest soft clip of a record, which the reference
//                            folds into the alignment properties while it reads (mod.rs:310, alignment_properties.rs:94-144).
//                            The other alleles of the locus (alt_variants): vlr_altvariants.h, in a session with
//                            vlr_fragpileup_set_alt_variants.  NOT mirrored: the read-inferred third allele, homopolymer_indel_len and the two
//                            prob_observable_at_homopolymer_* fields (the Myers traceback of the bio crate), max_depth subsampling,
//                            report_fragment_ids, replacements, SVs, breakends, deletions with more than one fetch.
//   methylation candidates   (a methylation session, vlr_fragpileup_open_methylation) variants/types/methylation.rs: vlr_methylation.h, included at
//                            the end of this file, has the rule, what of it is not mirrored, and its own member pass (record_members_meth);
//                            the fragment pass below runs on its members as it is.
// varlociraptor_amd/fragments.py is the same in Python (methylation.py for the methylation rule).
//
// Bounds: `features` runs only on a record vlr_bp::decode accepted, so the fixed head, the name (l_read_name bytes behind the head) and
// every aux field lie inside [p, p + size); it walks the aux fields again with the same length checks and reads RO and XA values byte
// by byte below the value's own length (the NUL that ends a Z value lies inside the record: aux_value_bytes found it).
#ifndef VLR_FRAGPILEUP_H
#define VLR_FRAGPILEUP_H

#include "vlr_basepileup.h"
#include "vlr_indelpileup.h"

namespace vlr_fp {

using vlr_bp::ld32;
using vlr_bp::Rec;

enum { ORIENT_INVALID = 255 };
// bits of Member::bits
enum { M_SOFTCLIPPED = 1, M_HAS_XA = 2, M_ENCLOSING = 4, M_HAS_SUPPORT = 8, M_OVERLAPS = 16 };   // (M_OVERLAPS: an indel session)

// one alt locus of a record: the key the mode is taken over
struct AltKey { uint64_t contig_hash, bucket; };
VLR_BP_HD inline bool key_less(const AltKey& a, const AltKey& b) { return a.contig_hash != b.contig_hash ? a.contig_hash < b.contig_hash : a.bucket < b.bucket; }
VLR_BP_HD inline bool key_equal(const AltKey& a, const AltKey& b) { return a.contig_hash == b.contig_hash && a.bucket == b.bucket; }

// one (record, locus) membership; 72 bytes
struct Member {
    double prob_ref, prob_alt;      // the support (M_HAS_SUPPORT)
    uint64_t ordinal;
    uint64_t name_off;              // the QNAME in the name pool
    uint64_t xa_off;                // the record's alt-locus keys in the key pool: [xa_off, xa_off + xa_n)
    uint32_t locus;
    uint32_t read_position, third_allele, l_seq;
    uint16_t flag;                  // the record's FLAG
    uint8_t name_len, mapq, orientation, strand, bits, status;
    uint32_t xa_n;
};

// what an indel session keeps beside a member (parallel to the members; the 72 bytes of a Member stay): the alignment and its clips
struct Side {
    int64_t pos, end_pos;
    uint32_t lead_soft, lead_hard, trail_soft, trail_hard;   // rust-htslib's leading_softclips / leading_hardclips / trailing_*
};

// what the member pass of an indel session knows beyond the loci: how long a locus can be (first_candidate) and where the Side records
// of the record's members go (parallel to `out` of record_members; nullptr in the count pass)
struct Indel {
    int64_t max_locus_len;
    Side* side;
};

// Deletion::centerpoint (deletion.rs:45): start + (len as f64 / 2.0).round(), half away from zero
VLR_BP_HD inline int64_t centerpoint(int64_t start, int64_t len) { return start + (len + 1) / 2; }

// the clips of insert_size.rs:21-28: a soft clip counts at an end when it is the outermost operation or lies behind one hard clip
VLR_BP_HD inline Side side_of(const Rec& r) {
    Side s = {r.pos, r.end_pos, 0u, 0u, 0u, 0u};
    const uint8_t* c = r.p + r.cig_off;
    const uint32_t n = r.n_cigar;
    if (n == 0) return s;
    uint32_t v = ld32(c);
    if ((v & 15u) == 5u) { s.lead_hard = v >> 4; v = n > 1 ? ld32(c + 4) : 0u; }
    if ((v & 15u) == 4u) s.lead_soft = v >> 4;
    v = ld32(c + 4u * (n - 1));
    if ((v & 15u) == 5u) { s.trail_hard = v >> 4; v = n > 1 ? ld32(c + 4u * (n - 2)) : 0u; }
    if ((v & 15u) == 4u) s.trail_soft = v >> 4;
    return s;
}

// estimate_insert_size (insert_size.rs:17-45) as written: inner mate distance + both spans; <= 0 is the reference's assertion
VLR_BP_HD inline int64_t insert_size(const Side& l, const Side& r) {
    const int64_t lc = (int64_t)l.lead_soft + (int64_t)l.lead_hard, rc = (int64_t)r.lead_soft + (int64_t)r.lead_hard;
    const int64_t ls = l.pos > lc ? l.pos - lc : 0, rs = r.pos > rc ? r.pos - rc : 0;
    const int64_t le = l.end_pos + (int64_t)l.trail_soft + (int64_t)l.trail_hard, re = r.end_pos + (int64_t)r.trail_soft + (int64_t)r.trail_hard;
    return (rs - le) + (le - ls) + (re - rs);
}

// update_max_cigar_ops_len (alignment_properties.rs:94-144) of one record: its longest D, its longest I, its largest S
VLR_BP_HD inline void cigar_maxima(const Rec& r, uint32_t* max_del, uint32_t* max_ins, uint32_t* max_clip) {
    *max_del = 0; *max_ins = 0; *max_clip = 0;
    for (uint32_t i = 0; i < r.n_cigar; ++i) {
        const uint32_t v = ld32(r.p + r.cig_off + 4u * i), op = v & 15u, l = v >> 4;
        if (op == 2u && l > *max_del) *max_del = l;
        if (op == 1u && l > *max_ins) *max_ins = l;
        if (op == 4u && l > *max_clip) *max_clip = l;
    }
}

// the order of the soft-clip fractions clip / l_seq, packed (clip << 32 | l_seq): by the fraction (exact in integers: a CIGAR length
// is below 2^28 and l_seq below 2^32, so the products fit 64 bits), then by the clip — a total order, so the maximum of a set does not
// depend on the order it is taken in.  l_seq == 0 (no fraction) is the least element.
VLR_BP_HD inline bool clip_frac_greater(uint64_t a, uint64_t b) {
    const uint64_t ac = a >> 32, al = a & 0xffffffffull, bc = b >> 32, bl = b & 0xffffffffull;
    if (al == 0) return false;
    if (bl == 0) return true;
    const uint64_t x = ac * bl, y = bc * al;
    return x != y ? x > y : ac > bc;
}

struct Feat {
    int32_t mtid;
    int64_t mpos;
    uint32_t name_len;              // without the NUL
    uint8_t orientation;            // VLR_FRAG_* or ORIENT_INVALID
    bool softclipped, has_xa;
    uint32_t xa_off, xa_len;        // the XA:Z value at p + xa_off (has_xa), without its NUL
};

// str::parse::<u64> of [v, v + n): an optional '+', then decimal digits only, at least one, no overflow
VLR_BP_HD inline bool parse_u64(const uint8_t* v, uint32_t n, uint64_t* out) {
    uint32_t k = 0;
    if (n > 0 && v[0] == '+') k = 1;
    if (k >= n) return false;
    uint64_t x = 0;
    for (; k < n; ++k) {
        if (v[k] < '0' || v[k] > '9') return false;
        const uint64_t d = (uint64_t)(v[k] - '0');
        if (x > (0xffffffffffffffffull - d) / 10ull) return false;
        x = x * 10ull + d;
    }
    *out = x;
    return true;
}

VLR_BP_HD inline uint64_t fnv1a64(const uint8_t* v, uint32_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint32_t k = 0; k < n; ++k) h = (h ^ (uint64_t)v[k]) * 0x100000001b3ull;
    return h;
}

// ExactAltLoci::from over the XA:Z value [v, v + n): the keys of its entries, in order, written to out[0 .. room) when out != nullptr;
// returns their number.  coeff = 10 * max_read_len (> 0).
VLR_BP_HD inline uint32_t xa_keys(const uint8_t* v, uint32_t n, uint64_t coeff, AltKey* out, uint64_t room) {
    uint32_t count = 0, e = 0;
    while (e <= n) {
        uint32_t end = e;
        while (end < n && v[end] != ';') ++end;
        if (end > e) {   // a non-empty entry [e, end): exactly four ','-separated items
            uint32_t commas = 0, c1 = end, c2 = end;
            for (uint32_t k = e; k < end; ++k)
                if (v[k] == ',') { if (commas == 0) c1 = k; else if (commas == 1) c2 = k; ++commas; }
            if (commas == 3) {
                uint32_t ps = c1 + 1;
                if (ps < c2 && v[ps] == '-') ++ps;
                uint64_t pos;
                if (parse_u64(v + ps, c2 - ps, &pos)) {
                    if (out != nullptr && (uint64_t)count < room) out[count] = AltKey{fnv1a64(v + e, c1 - e), pos / coeff * coeff};
                    ++count;
                }
            }
        }
        e = end + 1;
    }
    return count;
}

VLR_BP_HD inline bool value_is(const uint8_t* v, uint32_t n, const char* s) {
    uint32_t k = 0;
    for (; k < n && s[k]; ++k) if (v[k] != (uint8_t)s[k]) return false;
    return k == n && s[k] == 0;
}

// read_orientation's RO:Z branch (read_observation.rs:131-156): more than one comma-separated value = None, an unknown value an error
VLR_BP_HD inline uint8_t orientation_of_ro(const uint8_t* v, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) if (v[k] == ',') return VLR_FRAG_ORIENT_NONE;
    if (value_is(v, n, "F1R2")) return VLR_FRAG_F1R2;
    if (value_is(v, n, "F2R1")) return VLR_FRAG_F2R1;
    if (value_is(v, n, "F1F2")) return VLR_FRAG_F1F2;
    if (value_is(v, n, "F2F1")) return VLR_FRAG_F2F1;
    if (value_is(v, n, "R1R2")) return VLR_FRAG_R1R2;
    if (value_is(v, n, "R2R1")) return VLR_FRAG_R2R1;
    if (value_is(v, n, "R1F2")) return VLR_FRAG_R1F2;
    if (value_is(v, n, "R2F1")) return VLR_FRAG_R2F1;
    if (value_is(v, n, "None")) return VLR_FRAG_ORIENT_NONE;
    return ORIENT_INVALID;
}

// rust-htslib's read_pair_orientation: paired, both mates mapped, one contig, different positions; the mate that lies left comes first
VLR_BP_HD inline uint8_t orientation_of_flags(uint32_t flag, int32_t tid, int32_t mtid, int64_t pos, int64_t mpos) {
    if (!(flag & 0x1u) || (flag & 0x4u) || (flag & 0x8u) || tid != mtid || pos == mpos) return VLR_FRAG_ORIENT_NONE;
    const bool fwd = !(flag & 0x10u), mfwd = !(flag & 0x20u), first = (flag & 0x40u) != 0;
    const int64_t p1 = first ? pos : mpos, p2 = first ? mpos : pos;
    const bool f1 = first ? fwd : mfwd, f2 = first ? mfwd : fwd;
    if (p1 < p2) return f1 ? (f2 ? VLR_FRAG_F1F2 : VLR_FRAG_F1R2) : (f2 ? VLR_FRAG_R1F2 : VLR_FRAG_R1R2);
    return f2 ? (f1 ? VLR_FRAG_F2F1 : VLR_FRAG_F2R1) : (f1 ? VLR_FRAG_R2F1 : VLR_FRAG_R2R1);
}

// leading_softclips() > 0 || trailing_softclips() > 0: one hard clip at either end is skipped
VLR_BP_HD inline bool softclipped(const Rec& r) {
    const uint8_t* c = r.p + r.cig_off;
    const uint32_t n = r.n_cigar;
    if (n == 0) return false;
    uint32_t v = ld32(c);
    if ((v & 15u) == 5u && n > 1) v = ld32(c + 4);
    if ((v & 15u) == 4u && (v >> 4) > 0) return true;
    v = ld32(c + 4u * (n - 1));
    if ((v & 15u) == 5u && n > 1) v = ld32(c + 4u * (n - 2));
    return (v & 15u) == 4u && (v >> 4) > 0;
}

// the features of a record that vlr_bp::decode accepted (size = the size decode saw)
VLR_BP_HD inline void features(const Rec& r, uint64_t size, Feat& f) {
    const uint8_t* p = r.p;
    f.mtid = (int32_t)ld32(p + 24);
    f.mpos = (int64_t)(int32_t)ld32(p + 28);
    f.name_len = (uint32_t)p[12] - 1u;
    f.softclipped = softclipped(r);
    f.has_xa = false;
    f.xa_off = f.xa_len = 0;
    bool seen_ro = false, seen_xa = false, ro_string = false;
    uint8_t ro = VLR_FRAG_ORIENT_NONE;
    uint64_t o = (uint64_t)r.qual_off + r.l_seq;
    while (o + 3 <= size) {
        const uint32_t t0 = p[o], t1 = p[o + 1], ty = p[o + 2];
        const uint64_t nb = vlr_bp::aux_value_bytes(p, o + 3, size, ty);
        if (nb == 0 || o + 3 + nb > size) break;   // (decode refused such a record)
        if (t0 == 'R' && t1 == 'O' && !seen_ro) {
            seen_ro = true;
            if (ty == 'Z') { ro_string = true; ro = orientation_of_ro(p + o + 3, (uint32_t)(nb - 1)); }
        }
        if (t0 == 'X' && t1 == 'A' && !seen_xa) {
            seen_xa = true;
            if (ty == 'Z') { f.has_xa = true; f.xa_off = (uint32_t)(o + 3); f.xa_len = (uint32_t)(nb - 1); }
        }
        o += 3 + nb;
    }
    f.orientation = ro_string ? ro : orientation_of_flags(r.flag, r.ref_id, f.mtid, r.pos, f.mpos);
}

// the loci of which a record starting at (ref_id, pos) is a member: [first, ...) while member_of says so
// (max_len: the longest locus of the session — VLR_BASEPILEUP_MAX_LEN for SNVs / MNVs, an indel session's own)
VLR_BP_HD inline int64_t first_candidate(const vlr_bp::Loci& L, int32_t ref_id, int64_t pos, int64_t max_len = VLR_BASEPILEUP_MAX_LEN) {
    return vlr_bp::lower_bound(L, ref_id, pos - max_len + 1);
}
VLR_BP_HD inline bool in_reach(const vlr_bp::Loci& L, int64_t li, int32_t ref_id, int64_t pos, int64_t window) {
    return li < L.n && L.ref_id[li] == ref_id && L.start[li] - window <= pos;
}
VLR_BP_HD inline bool member_of(const vlr_bp::Loci& L, int64_t li, int64_t pos, int64_t window) {
    // start - window saturates at 0 in the reference; pos >= 0 makes that the same test
    return L.start[li] - window <= pos && pos < L.start[li] + (int64_t)L.len[li];
}

struct RecMembers {
    uint32_t n_members, name_bytes, n_xa;
    vlr_bp::RecClass cls;
    uint32_t n_ev, x_bytes, y_bytes;   // a realigning pass: the record's evidences and the bytes of their pairs (allele windows; read windows, twice)
    uint32_t seq_off, qual_off, l_seq; // of an accepted record: where its packed SEQ and its QUAL start
    uint32_t max_del, max_ins, max_clip;   // an indel session: cigar_maxima of a record that is a member of any locus
};

// what a realigning pass knows beyond the loci: --indel-window and the contigs of the BAM header (-1: not loaded, no locus lies on it)
struct Realign {
    int64_t window;
    int64_t n_refs;
    const int64_t* ctg_len;
};

// the alt allele window of locus li on its contig: [*begin, *end), clamped on its own; byte k of it is `alt_window_byte`
VLR_BP_HD inline void alt_window(const vlr_bp::Loci& L, int64_t li, int64_t contig_len, int64_t window, int64_t* begin, int64_t* end) {
    const int64_t rw = window * 3 / 2;
    *end = vlr_ip::max64(0, vlr_ip::min64(L.start[li] + (int64_t)L.len[li] + rw, contig_len));
    *begin = vlr_ip::min64(vlr_ip::max64(0, L.start[li] - rw), *end);
}
VLR_BP_HD inline uint8_t alt_window_byte(const vlr_bp::Loci& L, int64_t li, const uint8_t* contig, int64_t contig_len, int64_t begin, uint32_t k) {
    const int64_t i = begin + (int64_t)k - L.start[li];
    if (i >= 0 && i < (int64_t)L.len[li]) return L.alt_bases[L.base_off[li] + (uint64_t)i];
    return vlr_ip::window_byte(vlr_ip::WB_REF_BASE, contig, contig_len, begin, k);
}

// The evidence of a record that needs realignment at locus li: the windows of its candidate region, or a status.  *x_bytes / *y_bytes:
// the bytes of its two pairs.  own_alt_window: an indel session, whose loci bring their alt allele windows
// (alt_bases[base_off[li] .. base_off[li + 1])).
VLR_BP_HD inline vlr_indelpileup_hit realign_evidence(const Realign& ra, const vlr_bp::Loci& L, int64_t li, const Rec& r, uint64_t ordinal, uint32_t* x_bytes,
                                                      uint32_t* y_bytes, bool own_alt_window = false) {
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
    *x_bytes = 0; *y_bytes = 0;
    const int64_t contig_len = (int64_t)r.ref_id < ra.n_refs ? ra.ctg_len[r.ref_id] : -1;
    if (contig_len < 0) { h.status = VLR_INDELPILEUP_HIT_NO_OVERLAP; return h; }   // (every contig with a locus is loaded: not reached)
    const int64_t ls = L.start[li], le = ls + (int64_t)L.len[li];
    const vlr_ip::Region g = vlr_ip::candidate_region(r, ls, le, contig_len, ra.window);
    if (g.error) h.status = VLR_INDELPILEUP_HIT_LEADING_REFSKIP;
    else if (r.has_si) h.status = VLR_INDELPILEUP_HIT_STRAND_INFO;
    else if (!g.overlap || g.read_end - g.read_begin < 1) h.status = VLR_INDELPILEUP_HIT_NO_OVERLAP;
    else {
        int64_t ab = 0, ae = 0;
        if (own_alt_window) ae = (int64_t)(L.base_off[li + 1] - L.base_off[li]);
        else alt_window(L, li, contig_len, ra.window, &ab, &ae);
        h.ref_begin = g.ref_begin;
        h.ref_len = (uint32_t)(g.ref_end - g.ref_begin);
        h.read_begin = (uint32_t)g.read_begin;
        h.read_len = (uint32_t)(g.read_end - g.read_begin);
        *x_bytes = h.ref_len + (uint32_t)(ae - ab);
        *y_bytes = 2u * h.read_len;
    }
    return h;
}

// Everything one record gives: its members, loci ascending, written to out[0 .. room) when out != nullptr, its name to
// name_dst[0 .. name_len) when name_dst != nullptr and its alt-locus keys to xa_dst[0 .. xa_room) when xa_dst != nullptr.  The count pass
// (out == nullptr) and the fill pass run the same text.
VLR_BP_HD inline RecMembers record_members(const vlr_bp::Tables& t, const vlr_bp::Loci& L, const uint8_t* p, uint64_t size, uint64_t ordinal,
                                           bool realign_indel_reads, int64_t window, uint64_t coeff, Member* out, uint64_t room, uint64_t name_off, uint8_t* name_dst,
                                           uint64_t xa_off, AltKey* xa_dst, uint64_t xa_room, const Realign* ra = nullptr, vlr_indelpileup_hit* ev_out = nullptr,
                                           uint64_t ev_room = 0, const Indel* ia = nullptr, const uint64_t* comp_off = nullptr) {
    RecMembers res = {0u, 0u, 0u, vlr_bp::REC_OK, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    Rec r;
    res.cls = vlr_bp::decode(p, size, r);
    if (res.cls != vlr_bp::REC_OK || r.ref_id < 0 || r.pos < 0) return res;
    res.seq_off = r.seq_off; res.qual_off = r.qual_off; res.l_seq = r.l_seq;
    Feat f;
    bool have_f = false;
    const int64_t max_len = ia != nullptr ? ia->max_locus_len : (int64_t)VLR_BASEPILEUP_MAX_LEN;
    for (int64_t li = first_candidate(L, r.ref_id, r.pos, max_len); in_reach(L, li, r.ref_id, r.pos, window); ++li) {
        if (!member_of(L, li, r.pos, window)) continue;
        if (!have_f) {
            features(r, size, f);
            have_f = true;
            if (f.has_xa) res.n_xa = xa_keys(p + f.xa_off, f.xa_len, coeff, xa_dst, xa_room);
            if (ia != nullptr) cigar_maxima(r, &res.max_del, &res.max_ins, &res.max_clip);
        }
        if (ia != nullptr && ra != nullptr) {   // an indel locus: every member is realigned; no base-by-base score, no enclosing rule
            uint32_t xb, yb;
            const vlr_indelpileup_hit h = realign_evidence(*ra, L, li, r, ordinal, &xb, &yb, true);
            if (ev_out != nullptr && (uint64_t)res.n_ev < ev_room) ev_out[res.n_ev] = h;
            ++res.n_ev; res.x_bytes += xb; res.y_bytes += yb;
            if (out != nullptr && (uint64_t)res.n_members < room) {
                Member m;
                m.prob_ref = 0.0; m.prob_alt = 0.0;
                m.ordinal = ordinal;
                m.name_off = name_off;
                m.xa_off = xa_off;
                m.xa_n = res.n_xa;
                m.locus = (uint32_t)li;
                m.read_position = VLR_BASEPILEUP_NO_READ_POSITION;
                m.third_allele = 0;
                m.l_seq = r.l_seq;
                m.flag = (uint16_t)r.flag;
                m.name_len = (uint8_t)f.name_len;
                m.mapq = (uint8_t)r.mapq;
                m.orientation = f.orientation;
                m.strand = vlr_bp::STRAND_NONE;
                m.bits = (uint8_t)((f.softclipped ? M_SOFTCLIPPED : 0) | (f.has_xa ? M_HAS_XA : 0) | M_HAS_SUPPORT |
                                   (vlr_ip::overlaps(r, L.start[li], L.start[li] + (int64_t)L.len[li]) ? M_OVERLAPS : 0));
                m.status = VLR_BASEPILEUP_HIT_NEEDS_REALIGN;   // (until apply_realigned writes the evidence into it)
                out[res.n_members] = m;
                if (ia->side != nullptr) ia->side[res.n_members] = side_of(r);
            }
            ++res.n_members;
            continue;
        }
        // SingleLocus::overlap(read, false, 0, 0) == Enclosing
        const bool enclosing = r.pos <= L.start[li] && r.end_pos >= L.start[li] + (int64_t)L.len[li];
        // mnv.rs:83: an MNV whose locus has other alleles (comp_off: a session with vlr_fragpileup_set_alt_variants) realigns every
        // enclosing record; snv.rs:76 asks for the I / D operation whatever the locus has
        const bool by_competitor = comp_off != nullptr && ra != nullptr && realign_indel_reads && !r.has_indel && L.kind[li] == VLR_BASEPILEUP_MNV &&
                                   comp_off[li + 1] > comp_off[li];
        // a realigning pass: the evidence of a record vlr_bp::score flags (the count pass and the fill pass see the same ones)
        if (ra != nullptr && enclosing && realign_indel_reads && (r.has_indel || by_competitor)) {
            uint32_t xb, yb;
            const vlr_indelpileup_hit h = realign_evidence(*ra, L, li, r, ordinal, &xb, &yb);
            if (ev_out != nullptr && (uint64_t)res.n_ev < ev_room) ev_out[res.n_ev] = h;
            ++res.n_ev; res.x_bytes += xb; res.y_bytes += yb;
        }
        if (out != nullptr && (uint64_t)res.n_members < room) {
            Member m;
            m.prob_ref = 0.0; m.prob_alt = 0.0;
            m.ordinal = ordinal;
            m.name_off = name_off;
            m.xa_off = xa_off;
            m.xa_n = res.n_xa;
            m.locus = (uint32_t)li;
            m.read_position = VLR_BASEPILEUP_NO_READ_POSITION;
            m.third_allele = 0;
            m.l_seq = r.l_seq;
            m.flag = (uint16_t)r.flag;
            m.name_len = (uint8_t)f.name_len;
            m.mapq = (uint8_t)r.mapq;
            m.orientation = f.orientation;
            m.strand = vlr_bp::STRAND_NONE;
            m.bits = (uint8_t)((f.softclipped ? M_SOFTCLIPPED : 0) | (f.has_xa ? M_HAS_XA : 0));
            m.status = 0;
            if (enclosing) {
                m.bits |= M_ENCLOSING;
                vlr_basepileup_hit h;
                if (by_competitor) { m.bits |= M_HAS_SUPPORT; m.status = VLR_BASEPILEUP_HIT_NEEDS_REALIGN; }   // (until apply_realigned)
                else if (vlr_bp::score(t, L, li, r, ordinal, realign_indel_reads, h)) {
                    m.bits |= M_HAS_SUPPORT;
                    m.prob_ref = h.prob_ref; m.prob_alt = h.prob_alt;
                    m.read_position = h.read_position;
                    m.third_allele = h.third_allele;
                    m.strand = h.strand;
                    m.status = h.status;
                }
            }
            out[res.n_members] = m;
        }
        ++res.n_members;
    }
    if (res.n_members) {
        res.name_bytes = f.name_len;
        if (name_dst != nullptr) for (uint32_t k = 0; k < f.name_len; ++k) name_dst[k] = p[36 + k];
    }
    return res;
}

// mod.rs:358-376: both supports normalised by their sum when neither is ln 0; ln 0.5 each when both are.  Host only: std::log1p and
// std::exp are the calls math.log1p / math.exp of realign.normalize_support make.
inline void normalize_support(double* prob_ref, double* prob_alt) {
    const double ninf = -HUGE_VAL;
    if (*prob_ref != ninf && *prob_alt != ninf) {
        const double hi = *prob_ref > *prob_alt ? *prob_ref : *prob_alt, lo = *prob_ref > *prob_alt ? *prob_alt : *prob_ref;
        const double t = hi + std::log1p(std::exp(lo - hi));
        *prob_ref -= t; *prob_alt -= t;
    }
    if (*prob_ref == ninf && *prob_alt == ninf) { *prob_ref = std::log(0.5); *prob_alt = *prob_ref; }
}

// A realigned evidence into its member: the normalised supports (pr, pa) of a scored evidence, or the status of one that cannot be scored
VLR_BP_HD inline void apply_realigned(Member& m, const vlr_indelpileup_hit& h, double pr, double pa) {
    m.read_position = VLR_BASEPILEUP_NO_READ_POSITION;
    m.third_allele = 0;
    m.strand = vlr_bp::STRAND_NONE;
    m.prob_ref = 0.0; m.prob_alt = 0.0;
    if (h.status & VLR_INDELPILEUP_HIT_LEADING_REFSKIP) { m.status = VLR_BASEPILEUP_HIT_LEADING_REFSKIP; return; }
    if (h.status & VLR_INDELPILEUP_HIT_STRAND_INFO) { m.status = VLR_FRAGPILEUP_OBS_REALIGN_STRAND_INFO; return; }
    m.status = 0;
    m.prob_ref = pr; m.prob_alt = pa;
    if (pr != pa) m.strand = (m.flag & 0x10u) ? vlr_bp::STRAND_REVERSE : vlr_bp::STRAND_FORWARD;
}

// QNAME order: bytes, a shorter name before any name it prefixes (BTreeMap<Vec<u8>>)
VLR_BP_HD inline int compare_names(const uint8_t* names, const Member& a, const Member& b) {
    const uint8_t* x = names + a.name_off;
    const uint8_t* y = names + b.name_off;
    const uint32_t n = a.name_len < b.name_len ? a.name_len : b.name_len;
    for (uint32_t k = 0; k < n; ++k) if (x[k] != y[k]) return x[k] < y[k] ? -1 : 1;
    return a.name_len == b.name_len ? 0 : (a.name_len < b.name_len ? -1 : 1);
}
// the total order of the sort: (name, ordinal)
VLR_BP_HD inline bool member_less(const uint8_t* names, const Member& a, const Member& b) {
    const int c = compare_names(names, a, b);
    return c != 0 ? c < 0 : a.ordinal < b.ordinal;
}

// mod.rs:329-334, as written: the record is skipped when both it and `left` are first AND last in template
VLR_BP_HD inline bool skipped_as_partial(const Member& left, const Member& rec) {
    return ((left.flag & 0x40u) && (rec.flag & 0x40u)) && ((left.flag & 0x80u) && (rec.flag & 0x80u));
}

VLR_BP_HD inline bool is_alt_support(double pr, double pa) { return pa > pr; }

// the end of make_obs below, for make_obs_indel (make_obs keeps its own text, so that the kernels of the other sessions compile to the
// code they had): the status / strand rule (read_observation.rs:638-646) and the features of the fragment
VLR_BP_HD inline bool finish_obs(const Member& l, const Member* r, double pr, double pa, uint32_t pos, uint32_t strand, uint32_t third, uint32_t status,
                                 uint32_t max_mapq, vlr_fragpileup_obs& o) {
    if (status != 0) { pr = 0.0; pa = 0.0; pos = VLR_BASEPILEUP_NO_READ_POSITION; strand = vlr_bp::STRAND_NONE; third = 0; }
    else if (strand == vlr_bp::STRAND_NONE) return false;
    uint32_t orient = l.orientation;
    if (r != nullptr) {
        if (l.orientation == ORIENT_INVALID || r->orientation == ORIENT_INVALID) orient = ORIENT_INVALID;
        else if (l.orientation != r->orientation) orient = VLR_FRAG_ORIENT_NONE;
    }
    if (orient == ORIENT_INVALID) { status |= VLR_FRAGPILEUP_OBS_INVALID_RO; orient = VLR_FRAG_ORIENT_NONE; }
    const uint32_t min_mapq = r != nullptr && r->mapq < l.mapq ? r->mapq : l.mapq;
    uint32_t bits = 0;
    if ((l.bits & M_SOFTCLIPPED) || (r != nullptr && (r->bits & M_SOFTCLIPPED))) bits |= VLR_FRAGPILEUP_SOFTCLIPPED;
    if (l.flag & 0x1u) bits |= VLR_FRAGPILEUP_PAIRED;
    if (min_mapq == max_mapq) bits |= VLR_FRAGPILEUP_MAX_MAPQ;
    if ((l.bits & M_HAS_XA) || (r != nullptr && (r->bits & M_HAS_XA))) bits |= VLR_FRAGPILEUP_HAS_XA;
    o.prob_ref = pr; o.prob_alt = pa;
    o.left = l.ordinal;
    o.right = r != nullptr ? r->ordinal : VLR_FRAGPILEUP_NO_RECORD;
    o.read_position = pos;
    o.third_allele = third;
    o.len_sum = l.l_seq + (r != nullptr ? r->l_seq : 0u);
    o.min_mapq = (uint8_t)min_mapq;
    o.orientation = (uint8_t)orient;
    o.strand = (uint8_t)strand;
    o.bits = (uint8_t)bits;
    o.status = (uint8_t)status;
    o.alt_locus = VLR_ALTLOCUS_NONE;   // (set once the locus' major alt locus is known)
    for (int k = 0; k < 6; ++k) o.pad[k] = 0;
    return true;
}

// The observation of a fragment (`right` may be null): false = none (the pair is ambiguous, no record encloses the locus, no support,
// or the merged strand is None).
VLR_BP_HD inline bool make_obs(const Member& l, const Member* r, uint32_t max_mapq, vlr_fragpileup_obs& o) {
    if (r != nullptr) {
        if (l.mapq == 0 || r->mapq == 0) return false;
        if (!(l.bits & M_ENCLOSING) && !(r->bits & M_ENCLOSING)) return false;
    } else if (!(l.bits & M_ENCLOSING)) return false;
    const bool ls = (l.bits & M_HAS_SUPPORT) != 0, rs = r != nullptr && (r->bits & M_HAS_SUPPORT) != 0;
    if (!ls && !rs) return false;
    const Member& a = ls ? l : *r;
    double pr = a.prob_ref, pa = a.prob_alt;
    uint32_t pos = a.read_position, strand = a.strand, third = a.third_allele, status = a.status;
    if (ls && rs) {   // AlleleSupport::merge: *r into l
        const Member& b = *r;
        if (is_alt_support(pr, pa)) {
            if (is_alt_support(b.prob_ref, b.prob_alt) && pos != b.read_position) pos = VLR_BASEPILEUP_NO_READ_POSITION;
        } else if (is_alt_support(b.prob_ref, b.prob_alt)) pos = b.read_position;
        pr += b.prob_ref; pa += b.prob_alt;
        if (strand == vlr_bp::STRAND_NONE) strand = b.strand;
        else if (b.strand != vlr_bp::STRAND_NONE && strand != b.strand) strand = vlr_bp::STRAND_BOTH;
        third += b.third_allele;
        status |= b.status;
    }
    if (status != 0) { pr = 0.0; pa = 0.0; pos = VLR_BASEPILEUP_NO_READ_POSITION; strand = vlr_bp::STRAND_NONE; third = 0; }
    else if (strand == vlr_bp::STRAND_NONE) return false;
    uint32_t orient = l.orientation;
    if (r != nullptr) {
        if (l.orientation == ORIENT_INVALID || r->orientation == ORIENT_INVALID) orient = ORIENT_INVALID;
        else if (l.orientation != r->orientation) orient = VLR_FRAG_ORIENT_NONE;
    }
    if (orient == ORIENT_INVALID) { status |= VLR_FRAGPILEUP_OBS_INVALID_RO; orient = VLR_FRAG_ORIENT_NONE; }
    const uint32_t min_mapq = r != nullptr && r->mapq < l.mapq ? r->mapq : l.mapq;
    uint32_t bits = 0;
    if ((l.bits & M_SOFTCLIPPED) || (r != nullptr && (r->bits & M_SOFTCLIPPED))) bits |= VLR_FRAGPILEUP_SOFTCLIPPED;
    if (l.flag & 0x1u) bits |= VLR_FRAGPILEUP_PAIRED;
    if (min_mapq == max_mapq) bits |= VLR_FRAGPILEUP_MAX_MAPQ;
    if ((l.bits & M_HAS_XA) || (r != nullptr && (r->bits & M_HAS_XA))) bits |= VLR_FRAGPILEUP_HAS_XA;
    o.prob_ref = pr; o.prob_alt = pa;
    o.left = l.ordinal;
    o.right = r != nullptr ? r->ordinal : VLR_FRAGPILEUP_NO_RECORD;
    o.read_position = pos;
    o.third_allele = third;
    o.len_sum = l.l_seq + (r != nullptr ? r->l_seq : 0u);
    o.min_mapq = (uint8_t)min_mapq;
    o.orientation = (uint8_t)orient;
    o.strand = (uint8_t)strand;
    o.bits = (uint8_t)bits;
    o.status = (uint8_t)status;
    o.alt_locus = VLR_ALTLOCUS_NONE;   // (set once the locus' major alt locus is known)
    for (int k = 0; k < 6; ++k) o.pad[k] = 0;
    return true;
}

// The observation of a fragment of an indel locus (an indel session; the head of this file has the rule).  sl / sr: the Side records
// of the two members; x: the insert size (0 = none), the two read lengths, VLR_FRAGPILEUP_INDEL_* flags.
VLR_BP_HD inline bool make_obs_indel(const Member& l, const Member* r, const Side& sl, const Side* sr, uint32_t kind, int64_t locus_start, int64_t locus_len,
                                     bool has_insert_size, uint32_t max_mapq, vlr_fragpileup_obs& o, vlr_fragpileup_indel_obs& x) {
    const bool with_isize = r != nullptr && sr != nullptr && kind == VLR_INDELPILEUP_DELETION && has_insert_size;
    if (r != nullptr) {
        if (l.mapq == 0 || r->mapq == 0) return false;
        if (!(l.bits & M_OVERLAPS) && !(r->bits & M_OVERLAPS)) return false;
        if (with_isize) {
            const int64_t c = centerpoint(locus_start, locus_len);
            if (!(sl.pos < c && sr->end_pos > c)) return false;
        }
    } else if (!(l.bits & M_OVERLAPS)) return false;
    double pr = l.prob_ref, pa = l.prob_alt;
    uint32_t strand = l.strand, status = l.status;
    if (r != nullptr) {   // AlleleSupport::merge: *r into l (no read positions, no third-allele evidence)
        pr += r->prob_ref; pa += r->prob_alt;
        if (strand == vlr_bp::STRAND_NONE) strand = r->strand;
        else if (r->strand != vlr_bp::STRAND_NONE && strand != r->strand) strand = vlr_bp::STRAND_BOTH;
        status |= r->status;
    }
    if (!finish_obs(l, r, pr, pa, VLR_BASEPILEUP_NO_READ_POSITION, strand, 0u, status, max_mapq, o)) return false;
    x.insert_size = 0;
    x.len_left = l.l_seq;
    x.len_right = r != nullptr ? r->l_seq : 0u;
    x.flags = 0; x.pad = 0;
    if (with_isize) {
        x.insert_size = insert_size(sl, *sr);
        if (x.insert_size <= 0) x.flags |= VLR_FRAGPILEUP_INDEL_NONPOSITIVE_ISIZE;
    }
    return true;
}

// The pair of the run of equal names that begins at sorted position i (idx[i .. n), members M; mod.rs:325-338): the first member is
// `left`, every later one replaces `right` unless both are first AND last in template; *right_member = 0xffffffff for a single read
template <class Index>
VLR_BP_HD inline void run_pair(const Member* M, const uint8_t* names, const Index* idx, uint32_t i, uint32_t n, uint32_t* left_member, uint32_t* right_member) {
    const Member& left = M[idx[i]];
    *left_member = (uint32_t)idx[i];
    *right_member = 0xffffffffu;
    for (uint32_t j = i + 1; j < n; ++j) {
        const Member& rec = M[idx[j]];
        if (compare_names(names, left, rec) != 0) break;
        if (skipped_as_partial(left, rec)) continue;
        *right_member = (uint32_t)idx[j];
    }
}

// The fragment of that run: its observation, if any (the loop of run_pair, as it always stood here).
template <class Index>
VLR_BP_HD inline bool run_obs(const Member* M, const uint8_t* names, const Index* idx, uint32_t i, uint32_t n, uint32_t max_mapq, vlr_fragpileup_obs& o,
                              uint32_t* left_member, uint32_t* right_member) {
    const Member& left = M[idx[i]];
    const Member* right = nullptr;
    *left_member = (uint32_t)idx[i];
    *right_member = 0xffffffffu;
    for (uint32_t j = i + 1; j < n; ++j) {
        const Member& rec = M[idx[j]];
        if (compare_names(names, left, rec) != 0) break;
        if (skipped_as_partial(left, rec)) continue;
        right = &rec;
        *right_member = (uint32_t)idx[j];
    }
    return make_obs(left, right, max_mapq, o);
}

// the same for an indel locus (S: the Side records parallel to M)
template <class Index>
VLR_BP_HD inline bool run_obs_indel(const Member* M, const Side* S, const uint8_t* names, const Index* idx, uint32_t i, uint32_t n, uint32_t kind, int64_t locus_start,
                                    int64_t locus_len, bool has_insert_size, uint32_t max_mapq, vlr_fragpileup_obs& o, vlr_fragpileup_indel_obs& x,
                                    uint32_t* left_member, uint32_t* right_member) {
    run_pair(M, names, idx, i, n, left_member, right_member);
    const bool pair = *right_member != 0xffffffffu;
    return make_obs_indel(M[*left_member], pair ? &M[*right_member] : nullptr, S[*left_member], pair ? &S[*right_member] : nullptr, kind, locus_start, locus_len,
                          has_insert_size, max_mapq, o, x);
}

// does this observation's read position count for major_read_position (read_observation.rs:549-559)?
VLR_BP_HD inline bool counts_for_major(const vlr_fragpileup_obs& o) {
    return o.status == 0 && o.prob_alt > o.prob_ref && o.read_position != VLR_BASEPILEUP_NO_READ_POSITION;
}

// ReadObservation::process, alt_locus: Major when one of the fragment's keys is the major one, None without keys or without a major one
VLR_BP_HD inline uint8_t alt_locus_class(const AltKey* keys, const Member& l, const Member* r, bool have_major, const AltKey& major) {
    if (!have_major) return VLR_ALTLOCUS_NONE;
    const uint32_t n = l.xa_n + (r != nullptr ? r->xa_n : 0u);
    if (n == 0) return VLR_ALTLOCUS_NONE;
    for (uint32_t k = 0; k < l.xa_n; ++k) if (key_equal(keys[l.xa_off + k], major)) return VLR_ALTLOCUS_MAJOR;
    if (r != nullptr) for (uint32_t k = 0; k < r->xa_n; ++k) if (key_equal(keys[r->xa_off + k], major)) return VLR_ALTLOCUS_MAJOR;
    return VLR_ALTLOCUS_SOME;
}

// calc_major_feature over the keys keys[idx[0 .. n)], ascending by key_less, as major_of_sorted: the place in idx of the major key, -1 = none
template <class Index>
VLR_BP_HD inline int64_t major_key_of_sorted(const AltKey* keys, const Index* idx, uint32_t n) {
    uint32_t best = 0, best_n = 0, ties = 0;
    for (uint32_t i = 0; i < n;) {
        uint32_t j = i + 1;
        while (j < n && key_equal(keys[idx[j]], keys[idx[i]])) ++j;
        if (j - i > best_n) { best_n = j - i; best = i; ties = 1; }
        else if (j - i == best_n) ++ties;
        i = j;
    }
    return best_n > 1 && ties == 1 ? (int64_t)best : -1;
}

// calc_major_feature over ascending values v[0 .. n): the value that occurs most often, if it occurs more than once and more often than
// any other; *found = false otherwise
VLR_BP_HD inline uint32_t major_of_sorted(const uint32_t* v, uint32_t n, bool* found) {
    uint32_t best = 0, best_n = 0, ties = 0;
    for (uint32_t i = 0; i < n;) {
        uint32_t j = i + 1;
        while (j < n && v[j] == v[i]) ++j;
        if (j - i > best_n) { best_n = j - i; best = v[i]; ties = 1; }
        else if (j - i == best_n) ++ties;
        i = j;
    }
    *found = best_n > 1 && ties == 1;
    return best;
}

}  // namespace vlr_fp

#include "vlr_methylation.h"   // methylation candidates (a methylation session, vlr_fragpileup_open_methylation): the rule and its member pass

#endif
