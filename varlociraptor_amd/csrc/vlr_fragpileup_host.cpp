// vlr_fragpileup_host.cpp — the text of vlr_fragpileup.h compiled for the CPU: what the kernels of vlr_fragpileup.hip run, as a small program
// that tests/test_fragpileup_host.py builds with -fsanitize=address,undefined and runs over hand cases, fixtures and truncated and
// corrupted records.  Not part of libvlr.so.
//
//   vlr_fragpileup_host <input> <output>
// input  (little endian): "VFPH", i32 realign_indel_reads, i64 window, i32 max_mapq, i32 max_read_len, i64 n_loci, i32 ref_id[n], i64 start[n], i32 len[n],
//        u8 kind[n], ref bases, alt bases (sum of len bytes each), i64 n_records, u64 starts[n_records + 1], the records one behind the other
// output: f64 call[256], f64 miscall[256], i64 n_obs, the observations locus-major (vlr_fragpileup_obs), the locus records
//        (vlr_fragpileup_locus[n_loci]), u8 class[n_records] (0 taken, 1 rejected by the flag rule, 2 bad record)
// Every record is copied into a heap block of exactly its size before it is looked at, and the name pool and the alt-locus key pool are
// heap blocks of exactly what was counted, so that a read or write past either is a sanitizer report.  The members of a locus are handed to the sort in reverse
// order: the kernels' placement within a locus is not stable either.
//
//   vlr_fragpileup_host <input> <output> <realign input> <realign output>
// the realigning session (vlr_fragpileup_open_realign) without its pair-HMM kernels: the count and the fill pass get a vlr_fp::Realign,
// every record that is flagged gets its evidence (candidate region, windows), the four windows of each evidence are gathered byte by
// byte through vlr_ip::window_byte / vlr_fp::alt_window_byte into heap blocks of exactly their size, the raw scores the input gives per
// evidence are normalised (vlr_fp::normalize_support) and written into the members (vlr_fp::apply_realigned); <output> then holds the
// observations of the realigned members (tests/test_fragrealign_host_program.py).  Without the two arguments the output is what it always was.
// realign input:  "VFRH", i32 window, i64 n_refs, per contig of the BAM header i64 length (-1: not loaded) and its bytes (upper case), i64 n_scores,
//        f64 (ln_ref, ln_alt)[n_scores]: one pair per evidence, in evidence order
// realign output: i64 n_evidences, vlr_indelpileup_hit[n] (scores as given), per evidence its ref allele window, alt allele window, read bases, read qualities
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "vlr_fragpileup.h"

static_assert(sizeof(vlr_fragpileup_obs) == 56, "observation layout");
static_assert(sizeof(vlr_fragpileup_locus) == 24, "locus record layout");
static_assert(sizeof(vlr_indelpileup_hit) == 64, "hit layout");

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
};

bool slurp(const char* path, In& in) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); return false; }
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    in.d.resize((size_t)sz);
    const bool ok = !sz || fread(in.d.data(), 1, (size_t)sz, f) == (size_t)sz;
    fclose(f);
    return ok;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 && argc != 5) { fprintf(stderr, "usage: %s <input> <output> [<realign input> <realign output>]\n", argv[0]); return 2; }
    In in;
    if (!slurp(argv[1], in)) return 2;
    // the realigning session: window, the contigs in heap blocks of exactly their length, one pair of raw scores per evidence
    const bool realigning = argc == 5;
    vlr_fp::Realign ra{0, 0, nullptr};
    std::vector<int64_t> ctg_len;
    std::vector<uint8_t*> ctg;
    std::vector<double> scores;
    if (realigning) {
        In rin;
        if (!slurp(argv[3], rin)) return 2;
        const uint8_t* m = rin.take(4);
        if (!m || memcmp(m, "VFRH", 4) != 0) { fprintf(stderr, "bad realign input\n"); return 2; }
        const int32_t rwin = rin.arr<int32_t>(1)[0];
        const int64_t n_refs = rin.arr<int64_t>(1)[0];
        if (!rin.ok || rwin < 1 || rwin > VLR_INDELPILEUP_MAX_WINDOW || n_refs < 0 || n_refs > (1 << 20)) return 2;
        for (int64_t k = 0; k < n_refs; ++k) {
            const int64_t len = rin.arr<int64_t>(1)[0];
            if (!rin.ok || len < -1) return 2;
            uint8_t* c = (uint8_t*)malloc(len > 0 ? (size_t)len : 1);
            const uint8_t* p = len > 0 ? rin.take((size_t)len) : nullptr;
            if (len > 0 && !p) return 2;
            if (len > 0) memcpy(c, p, (size_t)len);
            ctg_len.push_back(len);
            ctg.push_back(c);
        }
        const int64_t n_scores = rin.arr<int64_t>(1)[0];
        if (!rin.ok || n_scores < 0 || n_scores > (1 << 24)) return 2;
        scores = rin.arr<double>(2 * (size_t)n_scores);
        if (!rin.ok) return 2;
        ra = vlr_fp::Realign{rwin, n_refs, ctg_len.data()};
    }
    const vlr_fp::Realign* rap = realigning ? &ra : nullptr;
    const uint8_t* magic = in.take(4);
    if (!magic || memcmp(magic, "VFPH", 4) != 0) { fprintf(stderr, "bad input\n"); return 2; }
    const int32_t realign = in.arr<int32_t>(1)[0];
    const int64_t window = in.arr<int64_t>(1)[0];
    const int32_t max_mapq = in.arr<int32_t>(1)[0];
    const int32_t max_read_len = in.arr<int32_t>(1)[0];
    const int64_t n_loci = in.arr<int64_t>(1)[0];
    if (!in.ok || n_loci < 0 || n_loci > (1 << 24) || window < 0 || max_read_len <= 0) return 2;
    const uint64_t coeff = 10ull * (uint64_t)max_read_len;
    const auto ref_id = in.arr<int32_t>((size_t)n_loci);
    const auto start = in.arr<int64_t>((size_t)n_loci);
    const auto len = in.arr<int32_t>((size_t)n_loci);
    const auto kind = in.arr<uint8_t>((size_t)n_loci);
    if (!in.ok) return 2;
    std::vector<uint64_t> base_off((size_t)n_loci + 1, 0);
    for (int64_t k = 0; k < n_loci; ++k) {
        if (len[(size_t)k] < 1 || len[(size_t)k] > VLR_BASEPILEUP_MAX_LEN) return 2;
        // (vlr_fragpileup_add_bam refuses a locus that does not lie inside its contig)
        if (realigning && (ref_id[(size_t)k] < 0 || (int64_t)ref_id[(size_t)k] >= ra.n_refs || start[(size_t)k] < 0 ||
                           start[(size_t)k] + len[(size_t)k] > ctg_len[(size_t)ref_id[(size_t)k]])) return 2;
        base_off[(size_t)k + 1] = base_off[(size_t)k] + (uint64_t)len[(size_t)k];
    }
    const auto refb = in.arr<uint8_t>((size_t)base_off[(size_t)n_loci]);
    const auto altb = in.arr<uint8_t>((size_t)base_off[(size_t)n_loci]);
    const int64_t n_rec = in.arr<int64_t>(1)[0];
    if (!in.ok || n_rec < 0 || n_rec > (1 << 24)) return 2;
    const auto starts = in.arr<uint64_t>((size_t)n_rec + 1);
    if (!in.ok) return 2;
    const size_t blob = in.o;
    for (int64_t i = 0; i < n_rec; ++i)
        if (starts[(size_t)i] > starts[(size_t)i + 1] || starts[(size_t)i + 1] > in.d.size() - blob) return 2;

    std::vector<double> tab(3 * 256);
    vlr_bp::fill_tables(tab.data(), tab.data() + 256, tab.data() + 512);
    const vlr_bp::Tables T{tab.data(), tab.data() + 256, tab.data() + 512, vlr_bp::ln_confusion(), vlr_bp::ln_any()};
    const vlr_bp::Loci L{n_loci, ref_id.data(), start.data(), len.data(), kind.data(), base_off.data(), refb.data(), altb.data()};

    // member pass: count, then fill into exactly what was counted
    std::vector<uint8_t*> recs((size_t)n_rec);
    std::vector<size_t> sizes((size_t)n_rec);
    std::vector<vlr_fp::RecMembers> cnt((size_t)n_rec);
    std::vector<uint8_t> cls((size_t)n_rec);
    size_t n_members = 0, n_name_bytes = 0, n_keys = 0, n_ev = 0;
    for (int64_t i = 0; i < n_rec; ++i) {
        const size_t size = (size_t)(starts[(size_t)i + 1] - starts[(size_t)i]);
        uint8_t* rec = (uint8_t*)malloc(size ? size : 1);   // exactly the record
        if (size) memcpy(rec, in.d.data() + blob + starts[(size_t)i], size);
        recs[(size_t)i] = rec;
        sizes[(size_t)i] = size;
        cnt[(size_t)i] = vlr_fp::record_members(T, L, rec, size, (uint64_t)i, realign != 0, window, coeff, nullptr, 0, 0, nullptr, 0, nullptr, 0, rap);
        cls[(size_t)i] = (uint8_t)cnt[(size_t)i].cls;
        n_ev += cnt[(size_t)i].n_ev;
        n_members += cnt[(size_t)i].n_members;
        n_name_bytes += cnt[(size_t)i].name_bytes;
        n_keys += cnt[(size_t)i].n_xa;
    }
    vlr_fp::Member* members = (vlr_fp::Member*)malloc(n_members ? n_members * sizeof(vlr_fp::Member) : 1);
    uint8_t* names = (uint8_t*)malloc(n_name_bytes ? n_name_bytes : 1);
    vlr_fp::AltKey* keys = (vlr_fp::AltKey*)malloc(n_keys ? n_keys * sizeof(vlr_fp::AltKey) : 1);
    if (realigning && scores.size() != 2 * n_ev) { fprintf(stderr, "%zu evidences, %zu score pairs\n", n_ev, scores.size() / 2); return 2; }
    vlr_indelpileup_hit* ev = (vlr_indelpileup_hit*)malloc(n_ev ? n_ev * sizeof(vlr_indelpileup_hit) : 1);   // exactly what was counted
    std::vector<uint8_t> windows;
    size_t m_at = 0, n_at = 0, k_at = 0, e_at = 0;
    for (int64_t i = 0; i < n_rec; ++i) {
        const vlr_fp::RecMembers c = cnt[(size_t)i];
        if (c.n_members) {
            const vlr_fp::RecMembers w = vlr_fp::record_members(T, L, recs[(size_t)i], sizes[(size_t)i], (uint64_t)i, realign != 0, window, coeff, members + m_at,
                                                                 c.n_members, (uint64_t)n_at, names + n_at, (uint64_t)k_at, keys + k_at, c.n_xa, rap, ev + e_at, c.n_ev);
            if (w.n_members != c.n_members || w.name_bytes != c.name_bytes || w.n_xa != c.n_xa || w.n_ev != c.n_ev || w.x_bytes != c.x_bytes || w.y_bytes != c.y_bytes) {
                fprintf(stderr, "count and fill pass differ at record %lld\n", (long long)i);
                return 3;
            }
            // the evidences of the record, as the fill kernel pairs them with its flagged members; the gather of their windows, byte by byte
            size_t e = 0, xb = 0, yb = 0;
            for (uint32_t k = 0; k < c.n_members && e < c.n_ev; ++k) {
                vlr_fp::Member& m = members[m_at + k];
                if (!(m.bits & vlr_fp::M_ENCLOSING) || !(m.status & VLR_BASEPILEUP_HIT_NEEDS_REALIGN)) continue;
                vlr_indelpileup_hit& h = ev[e_at + e];
                if (h.locus != m.locus || h.record != m.ordinal) { fprintf(stderr, "evidence and member differ at record %lld\n", (long long)i); return 3; }
                h.ln_ref = scores[2 * (e_at + e)]; h.ln_alt = scores[2 * (e_at + e) + 1];
                if (!h.status) {
                    const int32_t rid = ref_id[h.locus];
                    const uint8_t* contig = ctg[(size_t)rid];
                    const int64_t clen = ctg_len[(size_t)rid];
                    int64_t ab, ae;
                    vlr_fp::alt_window(L, (int64_t)h.locus, clen, ra.window, &ab, &ae);
                    const size_t al = (size_t)(ae - ab);
                    uint8_t* xr = (uint8_t*)malloc(h.ref_len ? h.ref_len : 1);
                    uint8_t* xa = (uint8_t*)malloc(al ? al : 1);
                    uint8_t* yb_ = (uint8_t*)malloc(h.read_len);
                    uint8_t* yq = (uint8_t*)malloc(h.read_len);
                    for (uint32_t j = 0; j < h.ref_len; ++j) xr[j] = vlr_ip::window_byte(vlr_ip::WB_REF_BASE, contig, clen, h.ref_begin, j);
                    for (uint32_t j = 0; j < (uint32_t)al; ++j) xa[j] = vlr_fp::alt_window_byte(L, (int64_t)h.locus, contig, clen, ab, j);
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
                ++e;
            }
            if (e != c.n_ev || xb != c.x_bytes || yb != c.y_bytes) { fprintf(stderr, "evidences and their bytes differ from the count at record %lld\n", (long long)i); return 3; }
        }
        e_at += c.n_ev;
        m_at += c.n_members;
        n_at += c.name_bytes;
        k_at += c.n_xa;
        free(recs[(size_t)i]);
    }
    // fragment pass
    std::vector<std::vector<uint32_t>> per((size_t)n_loci);
    for (size_t m = n_members; m-- > 0;) per[members[m].locus].push_back((uint32_t)m);
    std::vector<vlr_fragpileup_obs> obs;
    std::vector<vlr_fragpileup_locus> lrec((size_t)n_loci);
    for (int64_t l = 0; l < n_loci; ++l) {
        std::vector<uint32_t>& idx = per[(size_t)l];
        const uint32_t n = (uint32_t)idx.size();
        vlr_fragpileup_locus& lr = lrec[(size_t)l];
        lr = vlr_fragpileup_locus{(int64_t)obs.size(), n, 0, VLR_BASEPILEUP_NO_READ_POSITION, 0};
        if (n > VLR_FRAGPILEUP_MAX_MEMBERS) { lr.status = VLR_FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS; continue; }
        std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return vlr_fp::member_less(names, members[a], members[b]); });
        const size_t first = obs.size();
        std::vector<uint32_t> pos_keys, alt_idx;
        std::vector<std::pair<uint32_t, uint32_t>> pairs;
        for (uint32_t i = 0; i < n; ++i) {
            if (i > 0 && vlr_fp::compare_names(names, members[idx[i - 1]], members[idx[i]]) == 0) continue;
            vlr_fragpileup_obs o;
            uint32_t ml, mr;
            if (!vlr_fp::run_obs(members, names, idx.data(), i, n, (uint32_t)max_mapq, o, &ml, &mr)) continue;
            if (vlr_fp::counts_for_major(o)) pos_keys.push_back(o.read_position);
            for (uint32_t k = 0; k < members[ml].xa_n; ++k) alt_idx.push_back((uint32_t)(members[ml].xa_off + k));
            if (mr != 0xffffffffu) for (uint32_t k = 0; k < members[mr].xa_n; ++k) alt_idx.push_back((uint32_t)(members[mr].xa_off + k));
            pairs.push_back({ml, mr});
            obs.push_back(o);
        }
        if (alt_idx.size() > VLR_FRAGPILEUP_MAX_MEMBERS) { obs.resize(first); lr.status = VLR_FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI; continue; }
        std::sort(pos_keys.begin(), pos_keys.end());
        bool found = false;
        const uint32_t major = vlr_fp::major_of_sorted(pos_keys.data(), (uint32_t)pos_keys.size(), &found);
        std::sort(alt_idx.begin(), alt_idx.end(), [&](uint32_t a, uint32_t b) { return vlr_fp::key_less(keys[a], keys[b]); });
        const int64_t at_major = vlr_fp::major_key_of_sorted(keys, alt_idx.data(), (uint32_t)alt_idx.size());
        const bool have = at_major >= 0;
        const vlr_fp::AltKey mk = have ? keys[alt_idx[(size_t)at_major]] : vlr_fp::AltKey{0, 0};
        lr.n_obs = (uint32_t)(obs.size() - first);
        if (found) lr.major_read_position = major;
        for (size_t k = first; k < obs.size(); ++k) {
            if (found && obs[k].status == 0 && obs[k].read_position == major) obs[k].bits |= VLR_FRAGPILEUP_READPOS_MAJOR;
            const auto& pr = pairs[k - first];
            obs[k].alt_locus = vlr_fp::alt_locus_class(keys, members[pr.first], pr.second != 0xffffffffu ? &members[pr.second] : nullptr, have, mk);
        }
    }
    free(members);
    free(names);
    free(keys);
    if (realigning) {
        FILE* ro = fopen(argv[4], "wb");
        if (!ro) { perror(argv[4]); return 2; }
        const int64_t ne = (int64_t)n_ev;
        fwrite(&ne, 8, 1, ro);
        if (n_ev) fwrite(ev, sizeof(vlr_indelpileup_hit), n_ev, ro);
        if (!windows.empty()) fwrite(windows.data(), 1, windows.size(), ro);
        fclose(ro);
    }
    free(ev);
    for (uint8_t* c : ctg) free(c);

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int64_t n_obs = (int64_t)obs.size();
    fwrite(tab.data(), 8, 512, o);
    fwrite(&n_obs, 8, 1, o);
    if (n_obs) fwrite(obs.data(), sizeof(vlr_fragpileup_obs), (size_t)n_obs, o);
    if (n_loci) fwrite(lrec.data(), sizeof(vlr_fragpileup_locus), (size_t)n_loci, o);
    if (n_rec) fwrite(cls.data(), 1, (size_t)n_rec, o);
    fclose(o);
    return 0;
}
