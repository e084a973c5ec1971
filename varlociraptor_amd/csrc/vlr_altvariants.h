// vlr_altvariants.h — the other alleles of a locus on the reference side of a realigned evidence (`alt_variants` of the reference): the
// text the kernels of vlr_fragpileup.hip and the host program vlr_altvariants_host.cpp (built with the sanitizers by
// tests/test_altvariants_host_program.py) both compile.  Plain C++: no HIP types, no library calls.
//
// The rule (realignment/mod.rs:250-292, `prob_allele` 426-479): the reference side of an evidence is the best of the reference allele
// (i = 0) and the alt allele windows of the other candidates at its (CHROM, POS) (i = 1 .. K, utils/variant_buffer.rs:203-222: the ones
// before it in the file, then the ones after it).  Every allele gets its edit distance; alleles without a hit are out; the alleles at
// the minimum distance are the tied set; only those go through the pair HMM; the largest score wins, the lowest i on equal scores
// (`p > prob`, strict, mod.rs:466).  ln_ref is the winner's score, dist_ref the minimum distance.  The alt side is `prob_allele` over the
// candidate's one alt allele: its pair is always scored.  When no reference-side allele has a hit (an evidence with a status: its windows are
// empty) the reference's pair is kept, so that the evidence gets what a session without competitors gives it.
//
// Layout: evidence e of a scored range has 2 + K(locus) pairs at pair_base[e] ..: pair 0 = (ref allele window, read window), pair 1 =
// (alt allele window, read window), pair 1 + i = (window of competitor i, read window).  `layout_evidence` states the bytes, the passes
// below copy (`expand_evidence`), select (`select`), compact (`compact_pair`) and collect (`collect_evidence`); each takes (lane, lanes) so
// that a wave runs it lane-strided and the host program one lane at a time.
//
// Bounds: every copy is bounded by the destination pair's own length as its offsets state it AND by the source's length; a competitor
// is read only below comp_off[locus + 1] and its bytes below comp_base_off[c + 1], both checked by `check_table` before anything runs.
#ifndef VLR_ALTVARIANTS_H
#define VLR_ALTVARIANTS_H

#include "vlr_basepileup.h"

namespace vlr_av {

enum { kMaxAlt = VLR_FRAGPILEUP_MAX_ALT_VARIANTS, kMaxPairs = VLR_FRAGPILEUP_MAX_ALT_VARIANTS + 2, kEditBand = 4 };

// the competitor table of a session: competitors of locus l are comp_off[l] .. comp_off[l + 1], the window of competitor c is
// bases[base_off[c] .. base_off[c + 1])
struct Table {
    int64_t n_loci;
    const uint64_t* comp_off;
    const uint64_t* base_off;
    const uint8_t* bases;
};

VLR_BP_HD inline uint32_t n_competitors(const Table& t, uint32_t locus) {
    return (int64_t)locus < t.n_loci ? (uint32_t)(t.comp_off[locus + 1] - t.comp_off[locus]) : 0u;
}

// what is wrong with a table (0 = nothing): 1 offsets not ascending or not starting at 0, 2 more than kMaxAlt competitors at *where,
// 3 the window of competitor *where is empty or longer than max_window.  base_off == nullptr: the loci's counts alone are checked
VLR_BP_HD inline int check_table(int64_t n_loci, const uint64_t* comp_off, const uint64_t* base_off, uint64_t max_window, int64_t* where) {
    *where = 0;
    if (comp_off[0] != 0) return 1;
    for (int64_t l = 0; l < n_loci; ++l) {
        *where = l;
        if (comp_off[l + 1] < comp_off[l]) return 1;
        if (comp_off[l + 1] - comp_off[l] > (uint64_t)kMaxAlt) return 2;
    }
    if (base_off == nullptr) return 0;   // (the competitor counts alone)
    const uint64_t n = comp_off[n_loci];
    if (n > 0 && base_off[0] != 0) return 1;
    for (uint64_t c = 0; c < n; ++c) {
        *where = (int64_t)c;
        if (base_off[c + 1] < base_off[c]) return 1;
        if (base_off[c + 1] == base_off[c] || base_off[c + 1] - base_off[c] > max_window) return 3;
    }
    return 0;
}

// the reference-side allele i (0 = the reference, 1 .. K = the competitors) is pair `pair_of_allele(i)` of its evidence
VLR_BP_HD inline uint32_t pair_of_allele(uint32_t i) { return i == 0 ? 0u : i + 1u; }

// The bytes of the pairs of one evidence: x_len[j] / y_len[j] for j < 2 + K; returns 2 + K.  An evidence with a status has empty
// windows (ref_len = alt_len = read_len = 0 are given) and keeps its pairs, all empty.
VLR_BP_HD inline uint32_t layout_evidence(const Table& t, uint32_t locus, bool scored, uint32_t ref_len, uint32_t alt_len, uint32_t read_len, uint32_t* x_len,
                                          uint32_t* y_len) {
    const uint32_t k = n_competitors(t, locus);
    x_len[0] = scored ? ref_len : 0u;
    x_len[1] = scored ? alt_len : 0u;
    for (uint32_t i = 1; i <= k; ++i) {
        const uint64_t c = t.comp_off[locus] + (i - 1);
        x_len[1 + i] = scored ? (uint32_t)(t.base_off[c + 1] - t.base_off[c]) : 0u;
    }
    for (uint32_t j = 0; j < 2 + k; ++j) y_len[j] = scored ? read_len : 0u;
    return 2 + k;
}

// The windows of one evidence into its 2 + K pairs.  src_x: its two allele windows as the session gathered them ([0, ref_len) the ref
// window, [ref_len, ref_len + alt_len) the alt window); src_y / src_q: its read window.  xoff / yoff: the offsets of the range's pairs
// (np + 1 entries), pair0 the evidence's first pair, k its competitors.
VLR_BP_HD inline void expand_evidence(uint32_t lane, uint32_t lanes, const Table& t, uint32_t locus, uint32_t k, const uint8_t* src_x, uint32_t ref_len, uint32_t alt_len,
                                      const uint8_t* src_y, const uint8_t* src_q, uint32_t read_len, const uint32_t* xoff, const uint32_t* yoff, uint32_t pair0,
                                      uint8_t* x, uint8_t* y, uint8_t* q) {
    if (k > n_competitors(t, locus)) k = n_competitors(t, locus);
    for (uint32_t j = 0; j < 2 + k; ++j) {
        const uint32_t p = pair0 + j;
        const uint32_t xl = xoff[p + 1] - xoff[p], yl = yoff[p + 1] - yoff[p];
        const uint8_t* from;
        uint32_t n;
        if (j == 0) { from = src_x; n = ref_len; }
        else if (j == 1) { from = src_x + ref_len; n = alt_len; }
        else {
            const uint64_t c = t.comp_off[locus] + (j - 2);
            from = t.bases + t.base_off[c];
            n = (uint32_t)(t.base_off[c + 1] - t.base_off[c]);
        }
        for (uint32_t i = lane; i < n && i < xl; i += lanes) x[xoff[p] + i] = from[i];
        for (uint32_t i = lane; i < read_len && i < yl; i += lanes) { y[yoff[p] + i] = src_y[i]; q[yoff[p] + i] = src_q[i]; }
    }
}

struct Selected {
    int32_t min_dist;        // -1: no reference-side allele has a hit
    uint32_t n_tied, n_hits; // alleles at the minimum distance; alleles with a hit
    uint32_t keep;           // bit j: pair j of the evidence goes through the pair HMM
};

// prob_allele's first loop over the reference side (mod.rs:433-449) and what is scored: dist[j] of the evidence's 2 + k pairs
VLR_BP_HD inline Selected select(const int32_t* dist, uint32_t k) {
    Selected s = {-1, 0u, 0u, 2u};   // (the alt pair is always scored)
    for (uint32_t i = 0; i <= k; ++i) {
        const int32_t d = dist[pair_of_allele(i)];
        if (d < 0) continue;
        ++s.n_hits;
        if (s.min_dist < 0 || d < s.min_dist) { s.min_dist = d; s.n_tied = 1; s.keep = 2u | (1u << pair_of_allele(i)); }
        else if (d == s.min_dist) { ++s.n_tied; s.keep |= 1u << pair_of_allele(i); }
    }
    if (s.n_hits == 0) s.keep |= 1u;
    return s;
}

// the band of a kept pair: distance + 4 (pairhmm.rs:20), -1 without a hit and in fast mode
VLR_BP_HD inline int32_t band_of(int32_t dist, bool fast) { return !fast && dist >= 0 ? dist + kEditBand : -1; }

// One pair into the compacted batch (a pair that is not kept is not called): its bytes to cx / cy / cq at (cx_at, cy_at), its offsets and
// band at slot c; the last slot also writes the end of the offsets.  n_kept, x_total, y_total: the sums of the scans, which bound every
// write.
VLR_BP_HD inline void compact_pair(uint32_t lane, uint32_t lanes, const uint32_t* xoff, const uint32_t* yoff, const uint8_t* x, const uint8_t* y, const uint8_t* q, uint32_t p,
                                   int32_t band, uint64_t c, uint64_t cx_at, uint64_t cy_at, uint64_t n_kept, uint64_t x_total, uint64_t y_total, uint32_t* cxoff,
                                   uint32_t* cyoff, int32_t* cband, uint8_t* cx, uint8_t* cy, uint8_t* cq) {
    if (c >= n_kept) return;
    const uint32_t xl = xoff[p + 1] - xoff[p], yl = yoff[p + 1] - yoff[p];
    if (cx_at + xl > x_total || cy_at + yl > y_total) return;
    if (lane == 0) {
        cxoff[c] = (uint32_t)cx_at; cyoff[c] = (uint32_t)cy_at; cband[c] = band;
        if (c + 1 == n_kept) { cxoff[n_kept] = (uint32_t)x_total; cyoff[n_kept] = (uint32_t)y_total; }
    }
    for (uint32_t i = lane; i < xl; i += lanes) cx[cx_at + i] = x[xoff[p] + i];
    for (uint32_t i = lane; i < yl; i += lanes) { cy[cy_at + i] = y[yoff[p] + i]; cq[cy_at + i] = q[yoff[p] + i]; }
}

// prob_allele's second loop (mod.rs:455-471) over the tied set, and the alt side: slot[j] = the compacted slot of pair j (read only
// for kept pairs), lnp the scores of the compacted batch
VLR_BP_HD inline void collect_evidence(const int32_t* dist, uint32_t k, const uint64_t* slot, const double* lnp, uint64_t n_kept, vlr_indelpileup_hit* h,
                                       vlr_fragpileup_alt_hit* a) {
    const Selected s = select(dist, k);
    const double ninf = -__builtin_huge_val();
    double best = ninf;
    uint32_t winner = 0;
    bool have = false;
    for (uint32_t i = 0; i <= k; ++i) {
        const uint32_t j = pair_of_allele(i);
        if (!(s.keep & (1u << j)) || slot[j] >= n_kept) continue;
        const double p = lnp[slot[j]];
        if (!have || p > best) { best = p; winner = i; have = true; }
    }
    h->ln_ref = best;
    h->ln_alt = slot[1] < n_kept ? lnp[slot[1]] : ninf;
    h->dist_ref = s.min_dist;
    h->dist_alt = dist[1];
    a->winner = (uint8_t)winner;
    a->n_tied = (uint8_t)s.n_tied;
    a->n_ref_side_hits = (uint8_t)s.n_hits;
    for (int b = 0; b < 5; ++b) a->pad[b] = 0;
}

}  // namespace vlr_av

#endif
