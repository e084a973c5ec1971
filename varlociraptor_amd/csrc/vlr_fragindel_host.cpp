// vlr_fragindel_host.cpp — the indel arms of vlr_fragpileup.h compiled for the CPU: what the kIndel kernels of vlr_fragpileup.hip run, as a
// small program that tests/test_fragment_indel_host.py builds with -fsanitize=address,undefined and runs over hand cases.  Not part of
// libvlr.so.  It is the indel session (vlr_fragpileup_open_indel) without its pair-HMM kernels: the member pass with the indel arm of
// vlr_fp::record_members (count, then fill into exactly what was counted), the Side records, the per-locus CIGAR maxima, the gather of
// the four windows of every evidence byte by byte (vlr_ip::window_byte; the alt window from the locus's own bytes), the raw scores the
// input gives per evidence normalised (vlr_fp::normalize_support) and written into the members (vlr_fp::apply_realigned), and the
// fragment pass with the validity rule and the insert size (vlr_fp::run_obs_indel).
//
//   vlr_fragindel_host <input> <output>
// input  (little endian): "VFIH", i64 window, i32 max_mapq, i32 max_read_len, i32 has_insert_size, i32 realign_window, i64 n_refs, per contig
//        of the BAM header i64 length (-1: not loaded) and its bytes (upper case), i64 n_loci, i32 ref_id[n], i64 start[n], i64 end[n], u8 kind[n],
//        u64 alt_offset[n + 1], the alt windows, i64 n_records, u64 starts[n_records + 1], i64 n_scores, f64 (ln_ref, ln_alt)[n_scores] (one
//        pair per evidence, in evidence order), the records one behind the other
// output: i64 n_obs, vlr_fragpileup_obs[n_obs] locus-major, vlr_fragpileup_indel_obs[n_obs], vlr_fragpileup_locus[n_loci],
//        vlr_fragpileup_indel_locus[n_loci], i64 n_evidences, vlr_indelpileup_hit[n] (scores as given), per evidence its ref allele window,
//        alt allele window, read bases, read qualities
// Every record, every contig, every alt window array, the members, the Side records and every gathered window lie in heap blocks of
// exactly their size, so that a read or write past one is a sanitizer report.  The members of a locus are handed to the sort in reverse
// order: the kernels' placement within a locus is not stable either.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "vlr_fragpileup.h"

static_assert(sizeof(vlr_fragpileup_obs) == 56, "observation layout");
static_assert(sizeof(vlr_fragpileup_indel_obs) == 24, "indel side record layout");
static_assert(sizeof(vlr_fragpileup_indel_locus) == 16, "indel locus record layout");
static_assert(sizeof(vlr_fp::Side) == 32, "side record layout");

namespace {

struct In {
    std::vector<uint8_t> d;
    size_t o = 0;
    bool ok = true;
    const uint8_t* take(size_t n) {
        if (n > d.size() - o) { ok = false; return nullptr; }
        const uint8_t* p = d.data() + o;
        o += n;
        return p;
    }
    template <class T> std::vector<T> arr(size_t n) {
        std::vector<T> v(n);
        const uint8_t* p = take(n * sizeof(T));
        if (p && n) memcpy(v.data(), p, n * sizeof(T));
        return v;
    }
    template <class T> T one() { const std::vector<T> v = arr<T>(1); return v[0]; }
};

template <class T> T* exact(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <input> <output>\n", argv[0]); return 2; }
    In in;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        fseek(f, 0, SEEK_END);
        const long sz = ftell(f);
        fseek(f, 0, SEEK_SET);
        in.d.resize((size_t)sz);
        const bool ok = !sz || fread(in.d.data(), 1, (size_t)sz, f) == (size_t)sz;
        fclose(f);
        if (!ok) return 2;
    }
    const uint8_t* magic = in.take(4);
    if (!magic || memcmp(magic, "VFIH", 4) != 0) { fprintf(stderr, "bad input\n"); return 2; }
    const int64_t window = in.one<int64_t>();
    const int32_t max_mapq = in.one<int32_t>(), max_read_len = in.one<int32_t>(), has_isize = in.one<int32_t>(), rwin = in.one<int32_t>();
    const int64_t n_refs = in.one<int64_t>();
    if (!in.ok || window < 0 || max_read_len <= 0 || rwin < 1 || rwin > VLR_INDELPILEUP_MAX_WINDOW || n_refs < 0 || n_refs > (1 << 20)) return 2;
    std::vector<int64_t> ctg_len;
    std::vector<uint8_t*> ctg;
    for (int64_t k = 0; k < n_refs; ++k) {
        const int64_t len = in.one<int64_t>();
        if (!in.ok || len < -1) return 2;
        uint8_t* c = exact<uint8_t>(len > 0 ? (size_t)len : 0);
        const uint8_t* p = len > 0 ? in.take((size_t)len) : nullptr;
        if (len > 0 && !p) return 2;
        if (len > 0) memcpy(c, p, (size_t)len);
        ctg_len.push_back(len);
        ctg.push_back(c);
    }
    const int64_t n_loci = in.one<int64_t>();
    if (!in.ok || n_loci < 0 || n_loci > (1 << 24)) return 2;
    const size_t nl = (size_t)n_loci;
    const auto ref_id = in.arr<int32_t>(nl);
    const auto start = in.arr<int64_t>(nl);
    const auto end = in.arr<int64_t>(nl);
    const auto kind = in.arr<uint8_t>(nl);
    const auto alt_off = in.arr<uint64_t>(nl + 1);
    if (!in.ok || alt_off[0] != 0) return 2;
    std::vector<int32_t> len(nl);
    int64_t max_locus_len = 1;
    for (size_t k = 0; k < nl; ++k) {   // (what vlr_fragpileup_open_indel and vlr_fragpileup_add_bam check)
        const int64_t l = end[k] - start[k];
        if (ref_id[k] < 0 || (int64_t)ref_id[k] >= n_refs || start[k] < 0 || l < 1 || l > VLR_FRAGPILEUP_MAX_INDEL_LEN || end[k] > ctg_len[(size_t)ref_id[k]] ||
            alt_off[k + 1] < alt_off[k] || kind[k] > VLR_INDELPILEUP_INSERTION)
            return 2;
        len[k] = (int32_t)l;
        max_locus_len = std::max(max_locus_len, l);
    }
    const size_t n_alt = (size_t)alt_off[nl];
    uint8_t* altb = exact<uint8_t>(n_alt);   // exactly the alt windows
    {
        const uint8_t* p = in.take(n_alt);
        if (n_alt && !p) return 2;
        if (n_alt) memcpy(altb, p, n_alt);
    }
    const int64_t n_rec = in.one<int64_t>();
    if (!in.ok || n_rec < 0 || n_rec > (1 << 24)) return 2;
    const auto starts = in.arr<uint64_t>((size_t)n_rec + 1);
    const int64_t n_scores = in.one<int64_t>();
    if (!in.ok || n_scores < 0 || n_scores > (1 << 24)) return 2;
    const auto scores = in.arr<double>(2 * (size_t)n_scores);
    if (!in.ok) return 2;
    const size_t blob = in.o;
    for (int64_t i = 0; i < n_rec; ++i)
        if (starts[(size_t)i] > starts[(size_t)i + 1] || starts[(size_t)i + 1] > in.d.size() - blob) return 2;

    std::vector<double> tab(3 * 256);
    vlr_bp::fill_tables(tab.data(), tab.data() + 256, tab.data() + 512);
    const vlr_bp::Tables T{tab.data(), tab.data() + 256, tab.data() + 512, vlr_bp::ln_confusion(), vlr_bp::ln_any()};
    const vlr_bp::Loci L{n_loci, ref_id.data(), start.data(), len.data(), kind.data(), alt_off.data(), altb, altb};
    const vlr_fp::Realign ra{rwin, n_refs, ctg_len.data()};
    const uint64_t coeff = 10ull * (uint64_t)max_read_len;

    // member pass: count, then fill into exactly what was counted
    std::vector<uint8_t*> recs((size_t)n_rec);
    std::vector<size_t> sizes((size_t)n_rec);
    std::vector<vlr_fp::RecMembers> cnt((size_t)n_rec);
    size_t n_members = 0, n_name_bytes = 0, n_keys = 0, n_ev = 0;
    const vlr_fp::Indel count_arm{max_locus_len, nullptr};
    for (int64_t i = 0; i < n_rec; ++i) {
        const size_t size = (size_t)(starts[(size_t)i + 1] - starts[(size_t)i]);
        uint8_t* rec = exact<uint8_t>(size);   // exactly the record
        if (size) memcpy(rec, in.d.data() + blob + starts[(size_t)i], size);
        recs[(size_t)i] = rec;
        sizes[(size_t)i] = size;
        cnt[(size_t)i] = vlr_fp::record_members(T, L, rec, size, (uint64_t)i, true, window, coeff, nullptr, 0, 0, nullptr, 0, nullptr, 0, &ra, nullptr, 0, &count_arm);
        n_ev += cnt[(size_t)i].n_ev;
        n_members += cnt[(size_t)i].n_members;
        n_name_bytes += cnt[(size_t)i].name_bytes;
        n_keys += cnt[(size_t)i].n_xa;
    }
    if (scores.size() != 2 * n_ev) { fprintf(stderr, "%zu evidences, %zu score pairs\n", n_ev, scores.size() / 2); return 2; }
    vlr_fp::Member* members = exact<vlr_fp::Member>(n_members);
    vlr_fp::Side* sides = exact<vlr_fp::Side>(n_members);
    uint8_t* names = exact<uint8_t>(n_name_bytes);
    vlr_fp::AltKey* keys = exact<vlr_fp::AltKey>(n_keys);
    vlr_indelpileup_hit* ev = exact<vlr_indelpileup_hit>(n_ev);
    std::vector<vlr_fragpileup_indel_locus> lx(nl, vlr_fragpileup_indel_locus{0, 0, 0, 0});
    std::vector<uint8_t> windows;
    size_t m_at = 0, n_at = 0, k_at = 0, e_at = 0;
    for (int64_t i = 0; i < n_rec; ++i) {
        const vlr_fp::RecMembers c = cnt[(size_t)i];
        if (c.n_members) {
            const vlr_fp::Indel arm{max_locus_len, sides + m_at};
            const vlr_fp::RecMembers w = vlr_fp::record_members(T, L, recs[(size_t)i], sizes[(size_t)i], (uint64_t)i, true, window, coeff, members + m_at, c.n_members,
                                                                 (uint64_t)n_at, names + n_at, (uint64_t)k_at, keys + k_at, c.n_xa, &ra, ev + e_at, c.n_ev, &arm);
            if (w.n_members != c.n_members || w.name_bytes != c.name_bytes || w.n_xa != c.n_xa || w.n_ev != c.n_ev || w.x_bytes != c.x_bytes || w.y_bytes != c.y_bytes ||
                w.n_ev != w.n_members || w.max_del != c.max_del || w.max_ins != c.max_ins || w.max_clip != c.max_clip) {
                fprintf(stderr, "count and fill pass differ at record %lld\n", (long long)i);
                return 3;
            }
            size_t xb = 0, yb = 0;
            for (uint32_t k = 0; k < c.n_members; ++k) {   // evidence k of the record belongs to its member k
                vlr_fp::Member& m = members[m_at + k];
                vlr_indelpileup_hit& h = ev[e_at + k];
                if (h.locus != m.locus || h.record != m.ordinal) { fprintf(stderr, "evidence and member differ at record %lld\n", (long long)i); return 3; }
                // the maxima of the locus, as the fill kernel folds them
                vlr_fragpileup_indel_locus& x = lx[m.locus];
                x.max_del = std::max(x.max_del, c.max_del);
                x.max_ins = std::max(x.max_ins, c.max_ins);
                if (c.max_clip && c.l_seq) {
                    const uint64_t mine = ((uint64_t)c.max_clip << 32) | c.l_seq, seen = ((uint64_t)x.max_clip << 32) | x.max_clip_l_seq;
                    if (vlr_fp::clip_frac_greater(mine, seen)) { x.max_clip = c.max_clip; x.max_clip_l_seq = c.l_seq; }
                }
                h.ln_ref = scores[2 * (e_at + k)]; h.ln_alt = scores[2 * (e_at + k) + 1];
                if (!h.status) {
                    const int32_t rid = ref_id[h.locus];
                    const uint8_t* contig = ctg[(size_t)rid];
                    const int64_t clen = ctg_len[(size_t)rid];
                    const size_t al = (size_t)(alt_off[h.locus + 1] - alt_off[h.locus]);
                    uint8_t* xr = exact<uint8_t>(h.ref_len);
                    uint8_t* xa = exact<uint8_t>(al);
                    uint8_t* yb_ = exact<uint8_t>(h.read_len);
                    uint8_t* yq = exact<uint8_t>(h.read_len);
                    for (uint32_t j = 0; j < h.ref_len; ++j) xr[j] = vlr_ip::window_byte(vlr_ip::WB_REF_BASE, contig, clen, h.ref_begin, j);
                    for (size_t j = 0; j < al; ++j) xa[j] = L.alt_bases[L.base_off[h.locus] + j];
                    for (uint32_t j = 0; j < h.read_len; ++j) {
                        yb_[j] = vlr_ip::window_byte(vlr_ip::WB_READ_BASE, recs[(size_t)i] + c.seq_off, c.l_seq, h.read_begin, j);
                        yq[j] = vlr_ip::window_byte(vlr_ip::WB_READ_QUAL, recs[(size_t)i] + c.qual_off, c.l_seq, h.read_begin, j);
                    }
                    windows.insert(windows.end(), xr, xr + h.ref_len);
                    windows.insert(windows.end(), xa, xa + al);
                    windows.insert(windows.end(), yb_, yb_ + h.read_len);
                    windows.insert(windows.end(), yq, yq + h.read_len);
                    xb += h.ref_len + al; yb += 2 * (size_t)h.read_len;
                    free(xr); free(xa); free(yb_); free(yq);
                }
                double pr = h.ln_ref, pa = h.ln_alt;
                vlr_fp::normalize_support(&pr, &pa);
                vlr_fp::apply_realigned(m, h, pr, pa);
            }
            if (xb != c.x_bytes || yb != c.y_bytes) { fprintf(stderr, "the bytes of the evidences differ from the count at record %lld\n", (long long)i); return 3; }
        }
        e_at += c.n_ev;
        m_at += c.n_members;
        n_at += c.name_bytes;
        k_at += c.n_xa;
        free(recs[(size_t)i]);
    }
    // fragment pass
    std::vector<std::vector<uint32_t>> per(nl);
    for (size_t m = n_members; m-- > 0;) per[members[m].locus].push_back((uint32_t)m);
    std::vector<vlr_fragpileup_obs> obs;
    std::vector<vlr_fragpileup_indel_obs> obsx;
    std::vector<vlr_fragpileup_locus> lrec(nl);
    for (size_t l = 0; l < nl; ++l) {
        std::vector<uint32_t>& idx = per[l];
        const uint32_t n = (uint32_t)idx.size();
        vlr_fragpileup_locus& lr = lrec[l];
        lr = vlr_fragpileup_locus{(int64_t)obs.size(), n, 0, VLR_BASEPILEUP_NO_READ_POSITION, 0};
        if (n > VLR_FRAGPILEUP_MAX_MEMBERS) { lr.status = VLR_FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS; continue; }
        std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return vlr_fp::member_less(names, members[a], members[b]); });
        const size_t first = obs.size();
        std::vector<uint32_t> alt_idx;
        std::vector<std::pair<uint32_t, uint32_t>> pairs;
        for (uint32_t i = 0; i < n; ++i) {
            if (i > 0 && vlr_fp::compare_names(names, members[idx[i - 1]], members[idx[i]]) == 0) continue;
            vlr_fragpileup_obs o;
            vlr_fragpileup_indel_obs x;
            uint32_t ml, mr;
            if (!vlr_fp::run_obs_indel(members, sides, names, idx.data(), i, n, kind[l], start[l], (int64_t)len[l], has_isize != 0, (uint32_t)max_mapq, o, x, &ml, &mr)) continue;
            for (uint32_t k = 0; k < members[ml].xa_n; ++k) alt_idx.push_back((uint32_t)(members[ml].xa_off + k));
            if (mr != 0xffffffffu) for (uint32_t k = 0; k < members[mr].xa_n; ++k) alt_idx.push_back((uint32_t)(members[mr].xa_off + k));
            pairs.push_back({ml, mr});
            obs.push_back(o);
            obsx.push_back(x);
        }
        if (alt_idx.size() > VLR_FRAGPILEUP_MAX_MEMBERS) { obs.resize(first); obsx.resize(first); lr.status = VLR_FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI; continue; }
        std::sort(alt_idx.begin(), alt_idx.end(), [&](uint32_t a, uint32_t b) { return vlr_fp::key_less(keys[a], keys[b]); });
        const int64_t at_major = vlr_fp::major_key_of_sorted(keys, alt_idx.data(), (uint32_t)alt_idx.size());
        const bool have = at_major >= 0;
        const vlr_fp::AltKey mk = have ? keys[alt_idx[(size_t)at_major]] : vlr_fp::AltKey{0, 0};
        lr.n_obs = (uint32_t)(obs.size() - first);
        for (size_t k = first; k < obs.size(); ++k) {
            const auto& pr = pairs[k - first];
            obs[k].alt_locus = vlr_fp::alt_locus_class(keys, members[pr.first], pr.second != 0xffffffffu ? &members[pr.second] : nullptr, have, mk);
        }
    }
    free(members); free(sides); free(names); free(keys); free(altb);
    for (uint8_t* c : ctg) free(c);

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int64_t n_obs = (int64_t)obs.size(), ne = (int64_t)n_ev;
    fwrite(&n_obs, 8, 1, o);
    if (n_obs) fwrite(obs.data(), sizeof(vlr_fragpileup_obs), (size_t)n_obs, o);
    if (n_obs) fwrite(obsx.data(), sizeof(vlr_fragpileup_indel_obs), (size_t)n_obs, o);
    if (nl) fwrite(lrec.data(), sizeof(vlr_fragpileup_locus), nl, o);
    if (nl) fwrite(lx.data(), sizeof(vlr_fragpileup_indel_locus), nl, o);
    fwrite(&ne, 8, 1, o);
    if (n_ev) fwrite(ev, sizeof(vlr_indelpileup_hit), n_ev, o);
    if (!windows.empty()) fwrite(windows.data(), 1, windows.size(), o);
    fclose(o);
    free(ev);
    return 0;
}
