// vlr_methylation.h — methylation candidates (ALT <METH>) in the fragment session: the text the methylation kernels of
// vlr_fragpileup.hip and the host translation unit vlr_fragpileup_host.cpp (input magic "VFMH") both compile.  Plain C++: no HIP types,
// no library calls.  Included by vlr_fragpileup.h; varlociraptor_amd/methylation.py is the same in Python.  Restates
// variants/types/methylation.rs:
//   the locus                [pos, pos + 1) at the candidate's POS, the C of a CpG (:31-39); prob_sample_alt = ln 1 (:464-466); no
//                            homopolymer model, no third allele
//   read_reverse_orientation :486-495: unpaired, the reverse flag; paired, (reverse && first) || (!reverse && !first).  A record of
//                            reverse orientation is read at pos + 1 (the G), the others at pos (:47-50)
//   is_valid_evidence        :393-435: SingleLocus::overlap(read, false, start_offset, 0) == Enclosing with start_offset = 1 for reverse
//                            orientation (mod.rs:440-473): rec.pos <= start + off && rec.end_pos >= start + 1.  A reverse-orientation record
//                            that ends exactly at start + 1 is enclosing and has no base at start + 1: enclosing, without support.  In an
//                            annotated session a fragment is valid only when either record has an Mm / MM tag of any type (mm_exists,
//                            :98-118).  Support implies that tag (a support needs the map, the map needs the tag) and support implies
//                            enclosing (read_pos gives a position only inside [rec.pos, rec.end_pos), so pos <= start + off and end_pos
//                            >= start + off + 1 >= start + 1), and an observation needs a support: so vlr_fp::make_obs, which asks for
//                            an enclosing member and a support, decides as the reference does, and the fragment pass runs as it is
//   allele_support_per_read  :41-86 with process_read (:250-275): read_pos(position, false, false) (vlr_bp::read_pos; none inside a D or
//                            an N or outside; a CIGAR that begins with N is VLR_BASEPILEUP_HIT_LEADING_REFSKIP, whatever the flag); no
//                            support for a FLAG that is not one of 0, 16, 83, 99, 147, 163 (read_invalid, :374-376), for a mutation at
//                            the read position (:334-367: converted A / G forward and C / T reverse, annotated G / A / T forward and
//                            C / A / T reverse), and in an annotated session for a record without a usable map
//   converted reads          :306-324: prob_alt = prob_read_base(base, 'C' ('G' reverse), qual), prob_ref = prob_read_base(base, 'T' ('A'
//                            reverse), qual) on the tables of the SNV arm; an N gives ln 0.25 twice
//   annotated reads          :283-298: the record's 5mC map at the read position gives prob_alt = ln((ml + 0.5) / 256) and prob_ref =
//                            ln(1 - exp(prob_alt)), both from two 256-entry tables the host fills with libm (MethTables); a position
//                            that is not in the map gives ln 0 / ln 1
//   the 5mC map              extract_mm_ml_5mc (:130-221), as written: Mm before MM and Ml before ML, the first field of each name; MM
//                            must be of type Z and ML of type B with subtype C, else there is no map.  Blocks are split at ';'; an empty
//                            block and a block without ',' are skipped and consume no ML value; the header is the text before the first
//                            ','; a block is 5mC when its header starts with "C+m" or "C-m"; deltas parse as str::parse::<usize>
//                            (vlr_fp::parse_u64), tokens that do not parse are dropped; a block of another modification advances the ML
//                            index by its parsed deltas; in a 5mC block the k-th C of the read is meant, for reverse orientation the
//                            G's counted from the read's end; a missing ML value is 0; a later insert at a position wins; a delta that
//                            runs past the last C / G makes the whole record mapless, wherever it stands
//   strand                   Strand::from_record_and_pos(read, qpos) (SI:Z at qpos, else the record's) when prob_ref != prob_alt, else
//                            none (:60-66); the statuses of the SNV arm for an SI tag that is too short or holds another character
//   read position            Some(qpos) as :72 writes it: the position in the record's SEQ, WITHOUT the leading hard clip the SNV arm adds
//                            (snv.rs adds it, methylation.rs does not)
// NOT mirrored: max_depth subsampling, report_fragment_ids; an MM value that is not UTF-8 (rust-htslib fails to read it); in an annotated
// session a CIGAR that begins with N is refused even in a fragment without any Mm / MM tag, which the reference never scores.
//
// Cost: SEQ is walked once per record of an annotated session that is a member of any locus (a running count of the C's / G's in front of
// the members' read positions — a record's loci ascend, and so do its read positions — finished to the end of the read for the total);
// for reverse orientation the index from the end is total - 1 - prefix.  The MM value is walked once per member with a read position
// whose base is a C / G: O(bytes of MM) each, no storage — a record of 20 000 bases that is a member of 300 loci reads its MM value 300
// times.  A converted session walks nothing.  The count pass needs none of it: a member is a member with or without support.
//
// Bounds: everything runs on a record vlr_bp::decode accepted.  `find_mm` walks the aux fields again with the same length checks; every
// byte of the MM value is read below the value's own length (its NUL lies inside the record), every ML value below the array's count,
// bases and qualities below l_seq (read_pos gives a position below the read bases the CIGAR consumes, which decode checked against l_seq).
#ifndef VLR_METHYLATION_H
#define VLR_METHYLATION_H

namespace vlr_fp {

// ln((ml + 0.5) / 256) and ln(1 - exp of it), ml = 0 .. 255: filled by the host with libm (fill_meth_tables), as methylation.py does
struct MethTables {
    const double* ln_meth;     // [256]
    const double* ln_unmeth;   // [256]
};

// what the member pass of a methylation session knows beyond the loci
struct Meth {
    int annotated;             // VLR_METH_ANNOTATED, else converted
    MethTables mt;
};

VLR_BP_HD inline bool reverse_orientation(uint32_t flag) {
    const bool paired = (flag & 0x1u) != 0, reverse = (flag & 0x10u) != 0, first = (flag & 0x40u) != 0;
    return paired ? ((reverse && first) || (!reverse && !first)) : reverse;
}

VLR_BP_HD inline bool meth_enclosing(const Rec& r, int64_t start, bool rev) { return r.pos <= start + (rev ? 1 : 0) && r.end_pos >= start + 1; }

VLR_BP_HD inline bool read_invalid(uint32_t flag) { return !(flag == 0u || flag == 16u || flag == 83u || flag == 99u || flag == 147u || flag == 163u); }

VLR_BP_HD inline bool mutation_occurred(bool rev, bool annotated, uint32_t base) {
    if (rev) return base == 'C' || base == 'T' || (annotated && base == 'A');
    return base == 'G' || base == 'A' || (annotated && base == 'T');
}

// the Mm / MM and Ml / ML fields of a record
struct MmTags {
    bool usable;               // the chosen MM is Z and the chosen ML is B:C
    uint32_t mm_off, mm_len;   // the MM value at p + mm_off, without its NUL
    uint32_t ml_off, ml_n;     // the ML values at p + ml_off
};

VLR_BP_HD inline void find_mm(const Rec& r, uint64_t size, MmTags& m) {
    const uint8_t* p = r.p;
    // [0] Mm, [1] MM, [2] Ml, [3] ML: the first field of each name
    bool seen[4] = {false, false, false, false};
    uint32_t ty_of[4] = {0, 0, 0, 0}, off[4] = {0, 0, 0, 0}, nb_of[4] = {0, 0, 0, 0};
    uint64_t o = (uint64_t)r.qual_off + r.l_seq;
    while (o + 3 <= size) {
        const uint32_t t0 = p[o], t1 = p[o + 1], ty = p[o + 2];
        const uint64_t nb = vlr_bp::aux_value_bytes(p, o + 3, size, ty);
        if (nb == 0 || o + 3 + nb > size) break;   // (decode refused such a record)
        int which = -1;
        if (t0 == 'M' && t1 == 'm') which = 0; else if (t0 == 'M' && t1 == 'M') which = 1; else if (t0 == 'M' && t1 == 'l') which = 2; else if (t0 == 'M' && t1 == 'L') which = 3;
        if (which >= 0 && !seen[which]) { seen[which] = true; ty_of[which] = ty; off[which] = (uint32_t)(o + 3); nb_of[which] = (uint32_t)nb; }
        o += 3 + nb;
    }
    m.usable = false;
    m.mm_off = m.mm_len = m.ml_off = m.ml_n = 0;
    const int mm = seen[0] ? 0 : (seen[1] ? 1 : -1), ml = seen[2] ? 2 : (seen[3] ? 3 : -1);
    if (mm < 0 || ml < 0 || ty_of[mm] != 'Z' || ty_of[ml] != 'B' || p[off[ml]] != 'C') return;
    m.usable = true;
    m.mm_off = off[mm]; m.mm_len = nb_of[mm] - 1u;
    m.ml_off = off[ml] + 5u; m.ml_n = nb_of[ml] - 5u;   // (subtype C: one byte per value; aux_value_bytes checked 5 + count)
}

// the nibble of the packed SEQ: 2 = C, 4 = G
VLR_BP_HD inline uint32_t seq_nibble(const Rec& r, uint32_t i) {
    const uint32_t b = r.p[r.seq_off + (i >> 1)];
    return (i & 1u) ? (b & 15u) : (b >> 4);
}
// the C's (G's for reverse orientation) in [from, to) of the read
VLR_BP_HD inline uint32_t count_target(const Rec& r, bool rev, uint32_t from, uint32_t to) {
    const uint32_t want = rev ? 4u : 2u;
    uint32_t n = 0;
    for (uint32_t i = from; i < to; ++i) n += seq_nibble(r, i) == want ? 1u : 0u;
    return n;
}

// extract_mm_ml_5mc for one position: the read has `total` C's (G's), the position of interest is the k-th of the list the reference
// builds (k >= total: the position holds no C / G and cannot be in the map).  false = the record has no map (a delta past the last
// C / G); else *found says whether the position is in the map and *ml holds its value (the last insert).
VLR_BP_HD inline bool mm_lookup(const uint8_t* v, uint32_t n, const uint8_t* mlv, uint32_t ml_n, uint64_t total, uint64_t k, bool* found, uint32_t* ml) {
    *found = false; *ml = 0;
    uint64_t ml_index = 0;
    uint32_t e = 0;
    while (e <= n) {
        uint32_t end = e;
        while (end < n && v[end] != ';') ++end;
        uint32_t c1 = e;
        while (c1 < end && v[c1] != ',') ++c1;
        if (end > e && c1 < end) {   // a non-empty block with a ',': header [e, c1), deltas behind it
            const bool is5mc = c1 - e >= 3 && v[e] == 'C' && (v[e + 1] == '+' || v[e + 1] == '-') && v[e + 2] == 'm';
            uint64_t meth_pos = 0;
            uint32_t ts = c1 + 1;
            while (ts <= end) {
                uint32_t te = ts;
                while (te < end && v[te] != ',') ++te;
                uint64_t d;
                if (parse_u64(v + ts, te - ts, &d)) {
                    if (is5mc) {
                        if (meth_pos >= total || d >= total - meth_pos) return false;
                        meth_pos += d;
                        if (meth_pos == k) { *found = true; *ml = ml_index < (uint64_t)ml_n ? (uint32_t)mlv[ml_index] : 0u; }
                        ++meth_pos;
                    }
                    ++ml_index;
                }
                ts = te + 1;
            }
        }
        e = end + 1;
    }
    return true;
}

// what process_read and the strand rule give for a read position: false = no support
VLR_BP_HD inline bool meth_support(const vlr_bp::Tables& t, const Meth& me, const Rec& r, bool rev, uint32_t qpos, const MmTags* tags, uint64_t total, uint64_t prefix,
                                   double* prob_ref, double* prob_alt, uint8_t* strand, uint8_t* status) {
    *prob_ref = 0.0; *prob_alt = 0.0; *strand = vlr_bp::STRAND_NONE; *status = 0;
    const bool annotated = me.annotated != 0;
    const uint32_t base = vlr_bp::read_base(r, qpos);
    double pr, pa;
    if (annotated) {
        if (tags == nullptr || !tags->usable) return false;
        const bool target = base == (rev ? (uint32_t)'G' : (uint32_t)'C');
        const uint64_t k = target ? (rev ? total - 1 - prefix : prefix) : total;   // (a target base at qpos: prefix < total)
        bool found; uint32_t ml;
        if (!mm_lookup(r.p + tags->mm_off, tags->mm_len, r.p + tags->ml_off, tags->ml_n, total, k, &found, &ml)) return false;
        if (mutation_occurred(rev, true, base) || read_invalid(r.flag)) return false;
        if (found) { pa = me.mt.ln_meth[ml]; pr = me.mt.ln_unmeth[ml]; }
        else { pa = -HUGE_VAL; pr = 0.0; }
    } else {
        if (mutation_occurred(rev, false, base) || read_invalid(r.flag)) return false;
        const uint32_t q = r.p[r.qual_off + qpos];
        pa = vlr_bp::prob_read_base(t, base, rev ? 'G' : 'C', q);
        pr = vlr_bp::prob_read_base(t, base, rev ? 'A' : 'T', q);
    }
    *prob_ref = pr; *prob_alt = pa;
    if (pr != pa) {
        if (r.has_si) {
            if (qpos >= r.si_len) { *status = VLR_BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS; return true; }
            const uint32_t s = vlr_bp::strand_of_item(r.p[r.si_off + qpos]);
            if (s > 3u) { *status = VLR_BASEPILEUP_HIT_INVALID_STRAND_INFO; return true; }
            *strand = (uint8_t)s;
        } else *strand = (uint8_t)((r.flag & 0x10u) ? vlr_bp::STRAND_REVERSE : vlr_bp::STRAND_FORWARD);
    }
    return true;
}

// vlr_fp::record_members for a methylation session (loci of one base; L.kind, L.ref_bases and L.alt_bases are not read): the members of
// one record, loci ascending, with the same count / fill contract.  The fill pass writes every member first — an enclosing member with a
// read position keeps that position and, in an annotated session, the running count of C's / G's in front of it (in third_allele, until
// the second loop) — then finishes the walk of SEQ for the total and scores the members it wrote.
VLR_BP_HD inline RecMembers record_members_meth(const vlr_bp::Tables& t, const vlr_bp::Loci& L, const Meth& me, const uint8_t* p, uint64_t size, uint64_t ordinal,
                                                int64_t window, uint64_t coeff, Member* out, uint64_t room, uint64_t name_off, uint8_t* name_dst, uint64_t xa_off,
                                                AltKey* xa_dst, uint64_t xa_room) {
    RecMembers res = {0u, 0u, 0u, vlr_bp::REC_OK, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    Rec r;
    res.cls = vlr_bp::decode(p, size, r);
    if (res.cls != vlr_bp::REC_OK || r.ref_id < 0 || r.pos < 0) return res;
    res.seq_off = r.seq_off; res.qual_off = r.qual_off; res.l_seq = r.l_seq;
    Feat f;
    bool have_f = false;
    const bool rev = reverse_orientation(r.flag), annotated = me.annotated != 0;
    uint32_t walked = 0, prefix = 0;   // the C's / G's in [0, walked) of the read
    bool any_pos = false;
    for (int64_t li = first_candidate(L, r.ref_id, r.pos, 1); in_reach(L, li, r.ref_id, r.pos, window); ++li) {
        if (!(L.start[li] - window <= r.pos && r.pos < L.start[li] + 1)) continue;   // member_of for a locus of one base
        if (!have_f) {
            features(r, size, f);
            have_f = true;
            if (f.has_xa) res.n_xa = xa_keys(p + f.xa_off, f.xa_len, coeff, xa_dst, xa_room);
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
            if (meth_enclosing(r, L.start[li], rev)) {
                m.bits |= M_ENCLOSING;
                const int64_t qp = vlr_bp::read_pos(r, L.start[li] + (rev ? 1 : 0));
                if (qp == vlr_bp::RP_ERROR) { m.bits |= M_HAS_SUPPORT; m.status = VLR_BASEPILEUP_HIT_LEADING_REFSKIP; }
                else if (qp >= 0) {
                    m.read_position = (uint32_t)qp;
                    any_pos = true;
                    if (annotated && (uint32_t)qp >= walked) {   // (read positions ascend with the loci)
                        prefix += count_target(r, rev, walked, (uint32_t)qp);
                        walked = (uint32_t)qp;
                        m.third_allele = prefix;
                    } else if (annotated) m.third_allele = count_target(r, rev, 0, (uint32_t)qp);
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
    if (out != nullptr && any_pos) {
        MmTags tags = {false, 0u, 0u, 0u, 0u};
        uint64_t total = 0;
        if (annotated) {
            find_mm(r, size, tags);
            if (tags.usable) total = (uint64_t)prefix + count_target(r, rev, walked, r.l_seq);
        }
        const uint64_t written = (uint64_t)res.n_members < room ? (uint64_t)res.n_members : room;
        for (uint64_t k = 0; k < written; ++k) {
            Member& m = out[k];
            if (m.read_position == VLR_BASEPILEUP_NO_READ_POSITION || m.status != 0) continue;
            const uint64_t pre = m.third_allele;
            m.third_allele = 0;
            double pr, pa; uint8_t strand, status;
            if (meth_support(t, me, r, rev, m.read_position, annotated ? &tags : nullptr, total, pre, &pr, &pa, &strand, &status)) {
                m.bits |= M_HAS_SUPPORT;
                m.prob_ref = pr; m.prob_alt = pa; m.strand = strand; m.status = status;
            } else m.read_position = VLR_BASEPILEUP_NO_READ_POSITION;
        }
    }
    return res;
}

// the two tables of an annotated session (host side: libm, the calls methylation.py makes)
inline void fill_meth_tables(double* ln_meth, double* ln_unmeth) {
    for (int ml = 0; ml < 256; ++ml) {
        ln_meth[ml] = std::log(((double)ml + 0.5) / 256.0);
        ln_unmeth[ml] = std::log(1.0 - std::exp(ln_meth[ml]));
    }
}

}  // namespace vlr_fp

#endif
