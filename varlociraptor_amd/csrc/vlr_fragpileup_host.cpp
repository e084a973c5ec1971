// vlr_fragpileup_host.cpp — the text of vlr_fragpileup.h compiled for the CPU: what the kernels of vlr_fragpileup.hip run, as a small program
// that tests/test_fragpileup_host.py, tests/test_fragrealign_host_program.py and tests/test_fragment_indel_host.py build with
// -fsanitize=address,undefined and run over hand cases, fixtures and truncated and corrupted records.  Not part of libvlr.so.  The magic
// of <input> tells the session: "VFPH" SNV / MNV candidates, "VFIH" deletions / insertions, "VFMH" methylation candidates
// (tests/test_methylation_host.py).  All run the same passes below; the indel arms (vlr_fp::Indel, vlr_fp::run_obs_indel, the Side
// records, the per-locus CIGAR maxima) and the member pass of a methylation session (vlr_fp::record_members_meth) are the points where
// they differ.
//
//   vlr_fragpileup_host <input> <output>
// input  (little endian): "VFPH", i32 realign_indel_reads, i64 window, i32 max_mapq, i32 max_read_len, i64 n_loci, i32 ref_id[n], i64 start[n], i32 len[n],
//        u8 kind[n], ref bases, alt bases (sum of len bytes each), i64 n_records, u64 starts[n_records + 1], the records one behind the other
// output: f64 call[256], f64 miscall[256], i64 n_obs, the observations locus-major (vlr_fragpileup_obs), the locus records
//        (vlr_fragpileup_locus[n_loci]), u8 class[n_records] (0 taken, 1 rejected by the flag rule, 2 bad record)
//
//   vlr_fragpileup_host <input> <output> <realign input> <realign output>
// the realigning session (vlr_fragpileup_open_realign) without its pair-HMM kernels: the count and the fill pass get a vlr_fp::Realign,
// every record that is flagged gets its evidence (candidate region, windows), the four windows of each evidence are gathered byte by
// byte through vlr_ip::window_byte / vlr_fp::alt_window_byte, the raw scores the input gives per evidence are normalised
// (vlr_fp::normalize_support) and written into the members (vlr_fp::apply_realigned); <output> then holds the observations of the
// realigned members.  Without the two arguments the output is that of the plain session.
// realign input:  "VFRH", i32 window, i64 n_refs, per contig of the BAM header i64 length (-1: not loaded) and its bytes (upper case), i64 n_scores,
//        f64 (ln_ref, ln_alt)[n_scores]: one pair per evidence, in evidence order
// realign output: i64 n_evidences, vlr_indelpileup_hit[n] (scores as given), per evidence its ref allele window, alt allele window, read bases, read qualities
//
//   vlr_fragpileup_host <input> <output>
// the indel session (vlr_fragpileup_open_indel) without its pair-HMM kernels: every member an evidence, the alt window from the locus's
// own bytes, the fragment pass with the validity rule and the insert size.
// input:  "VFIH", i64 window, i32 max_mapq, i32 max_read_len, i32 has_insert_size, i32 realign_window, i64 n_refs, the contigs as above, i64 n_loci,
//        i32 ref_id[n], i64 start[n], i64 end[n], u8 kind[n], u64 alt_offset[n + 1], the alt windows, i64 n_records, u64 starts[n_records + 1],
//        i64 n_scores, f64 (ln_ref, ln_alt)[n_scores], the records one behind the other
// output: i64 n_obs, vlr_fragpileup_obs[n_obs] locus-major, vlr_fragpileup_indel_obs[n_obs], vlr_fragpileup_locus[n_loci],
//        vlr_fragpileup_indel_locus[n_loci], then what the realign output holds
//
//   vlr_fragpileup_host <input> <output>
// the methylation session (vlr_fragpileup_open_methylation): the member pass of vlr_methylation.h, the fragment pass of every session.
// input:  "VFMH", i32 readtype (VLR_METH_*), i64 window, i32 max_mapq, i32 max_read_len, i64 n_loci, i32 ref_id[n], i64 start[n], i64 n_records,
//        u64 starts[n_records + 1], the records one behind the other
// output: f64 call[256], f64 miscall[256], f64 ln_meth[256], f64 ln_unmeth[256], then as for "VFPH" from n_obs on
//
// Every record, every contig, the members, the Side records, the name pool, the alt-locus key pool, the evidences and every gathered
// window lie in heap blocks of exactly their size, so that a read or write past one is a sanitizer report.  The members of a locus are
// handed to the sort in reverse order: the kernels' placement within a locus is not stable either.
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

// a heap block of exactly n items
template <class T> T* exact(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

// a session's input and what its passes build
struct Run {
    bool indel = false;                     // "VFIH"
    bool meth = false;                      // "VFMH"
    vlr_fp::Meth me{0, {nullptr, nullptr}};
    std::vector<double> mtab = std::vector<double>(2 * 256);
    bool realigning = false;                // the count and the fill pass get `ra`; an indel session always
    bool realign = true, has_isize = false; // realign_indel_reads, has_insert_size
    int64_t window = 0, max_locus_len = 1, n_loci = 0, n_rec = 0;
    int32_t max_mapq = 0, max_read_len = 0;
    std::vector<int32_t> ref_id, len;
    std::vector<int64_t> start;
    std::vector<uint8_t> kind, refb, altb;
    std::vector<uint64_t> base_off, starts;
    std::vector<int64_t> ctg_len;
    std::vector<uint8_t*> ctg;
    vlr_fp::Realign ra{0, 0, nullptr};
    std::vector<double> scores, tab = std::vector<double>(3 * 256);
    size_t n_members = 0, n_ev = 0;
    vlr_fp::Member* members = nullptr;
    vlr_fp::Side* sides = nullptr;          // an indel session: parallel to the members
    uint8_t* names = nullptr;
    vlr_fp::AltKey* keys = nullptr;
    vlr_indelpileup_hit* ev = nullptr;
    std::vector<uint8_t> windows, cls;
    std::vector<vlr_fragpileup_indel_locus> lx;
    std::vector<vlr_fragpileup_obs> obs;
    std::vector<vlr_fragpileup_indel_obs> obsx;
    std::vector<vlr_fragpileup_locus> lrec;
    ~Run() {
        free(members); free(sides); free(names); free(keys); free(ev);
        for (uint8_t* c : ctg) free(c);
    }
};

// i32 window, i64 n_refs and the contigs of the BAM header
bool read_contigs(In& in, Run& r) {
    const int32_t rwin = in.one<int32_t>();
    const int64_t n_refs = in.one<int64_t>();
    if (!in.ok || rwin < 1 || rwin > VLR_INDELPILEUP_MAX_WINDOW || n_refs < 0 || n_refs > (1 << 20)) return false;
    for (int64_t k = 0; k < n_refs; ++k) {
        const int64_t len = in.one<int64_t>();
        if (!in.ok || len < -1) return false;
        const uint8_t* p = len > 0 ? in.take((size_t)len) : nullptr;
        if (len > 0 && !p) return false;
        uint8_t* c = exact<uint8_t>(len > 0 ? (size_t)len : 0);
        if (len > 0) memcpy(c, p, (size_t)len);
        r.ctg_len.push_back(len);
        r.ctg.push_back(c);
    }
    r.ra = vlr_fp::Realign{rwin, n_refs, r.ctg_len.data()};
    r.realigning = true;
    return true;
}

// i64 n_scores and one pair of raw scores per evidence
bool read_scores(In& in, Run& r) {
    const int64_t n_scores = in.one<int64_t>();
    if (!in.ok || n_scores < 0 || n_scores > (1 << 24)) return false;
    r.scores = in.arr<double>(2 * (size_t)n_scores);
    return in.ok;
}

// i64 n_records and where each starts in the blob at the end of the input
bool read_starts(In& in, Run& r) {
    r.n_rec = in.one<int64_t>();
    if (!in.ok || r.n_rec < 0 || r.n_rec > (1 << 24)) return false;
    r.starts = in.arr<uint64_t>((size_t)r.n_rec + 1);
    return in.ok;
}

int read_snv(In& in, const uint8_t* magic, const char* realign_path, Run& r) {
    if (realign_path) {
        In rin;
        if (!slurp(realign_path, rin)) return 2;
        const uint8_t* m = rin.take(4);
        if (!m || memcmp(m, "VFRH", 4) != 0) { fprintf(stderr, "bad realign input\n"); return 2; }
        if (!read_contigs(rin, r) || !read_scores(rin, r)) return 2;
    }
    if (!magic || memcmp(magic, "VFPH", 4) != 0) { fprintf(stderr, "bad input\n"); return 2; }
    r.realign = in.one<int32_t>() != 0;
    r.window = in.one<int64_t>();
    r.max_mapq = in.one<int32_t>();
    r.max_read_len = in.one<int32_t>();
    r.n_loci = in.one<int64_t>();
    if (!in.ok || r.n_loci < 0 || r.n_loci > (1 << 24) || r.window < 0 || r.max_read_len <= 0) return 2;
    const size_t nl = (size_t)r.n_loci;
    r.ref_id = in.arr<int32_t>(nl);
    r.start = in.arr<int64_t>(nl);
    r.len = in.arr<int32_t>(nl);
    r.kind = in.arr<uint8_t>(nl);
    if (!in.ok) return 2;
    r.base_off.assign(nl + 1, 0);
    for (size_t k = 0; k < nl; ++k) {
        if (r.len[k] < 1 || r.len[k] > VLR_BASEPILEUP_MAX_LEN) return 2;
        // (vlr_fragpileup_add_bam refuses a locus that does not lie inside its contig)
        if (r.realigning && (r.ref_id[k] < 0 || (int64_t)r.ref_id[k] >= r.ra.n_refs || r.start[k] < 0 || r.start[k] + r.len[k] > r.ctg_len[(size_t)r.ref_id[k]])) return 2;
        r.base_off[k + 1] = r.base_off[k] + (uint64_t)r.len[k];
    }
    r.refb = in.arr<uint8_t>((size_t)r.base_off[nl]);
    r.altb = in.arr<uint8_t>((size_t)r.base_off[nl]);
    return read_starts(in, r) ? 0 : 2;
}

int read_meth(In& in, Run& r) {
    r.meth = true;
    r.realign = false;
    const int32_t readtype = in.one<int32_t>();
    r.window = in.one<int64_t>();
    r.max_mapq = in.one<int32_t>();
    r.max_read_len = in.one<int32_t>();
    r.n_loci = in.one<int64_t>();
    if (!in.ok || (readtype != VLR_METH_CONVERTED && readtype != VLR_METH_ANNOTATED) || r.n_loci < 0 || r.n_loci > (1 << 24) || r.window < 0 || r.max_read_len <= 0) return 2;
    const size_t nl = (size_t)r.n_loci;
    r.ref_id = in.arr<int32_t>(nl);
    r.start = in.arr<int64_t>(nl);
    if (!in.ok) return 2;
    for (size_t k = 0; k < nl; ++k) {   // (what vlr_fragpileup_open_methylation checks)
        if (r.ref_id[k] < 0 || r.start[k] < 0) return 2;
        if (k > 0 && (r.ref_id[k] < r.ref_id[k - 1] || (r.ref_id[k] == r.ref_id[k - 1] && r.start[k] < r.start[k - 1]))) return 2;
    }
    // the loci as the session's tables hold them: one base each; kind and the allele bytes are never read
    r.len.assign(nl, 1);
    r.kind.assign(nl, (uint8_t)VLR_BASEPILEUP_SNV);
    r.base_off.resize(nl + 1);
    for (size_t k = 0; k <= nl; ++k) r.base_off[k] = k;
    r.refb.assign(nl, (uint8_t)'N');
    r.altb.assign(nl, (uint8_t)'N');
    vlr_fp::fill_meth_tables(r.mtab.data(), r.mtab.data() + 256);
    r.me = vlr_fp::Meth{readtype == VLR_METH_ANNOTATED ? 1 : 0, vlr_fp::MethTables{r.mtab.data(), r.mtab.data() + 256}};
    return read_starts(in, r) ? 0 : 2;
}

int read_indel(In& in, Run& r) {
    r.indel = true;
    r.window = in.one<int64_t>();
    r.max_mapq = in.one<int32_t>();
    r.max_read_len = in.one<int32_t>();
    r.has_isize = in.one<int32_t>() != 0;
    if (!in.ok || r.window < 0 || r.max_read_len <= 0 || !read_contigs(in, r)) return 2;
    r.n_loci = in.one<int64_t>();
    if (!in.ok || r.n_loci < 0 || r.n_loci > (1 << 24)) return 2;
    const size_t nl = (size_t)r.n_loci;
    r.ref_id = in.arr<int32_t>(nl);
    r.start = in.arr<int64_t>(nl);
    const auto end = in.arr<int64_t>(nl);
    r.kind = in.arr<uint8_t>(nl);
    r.base_off = in.arr<uint64_t>(nl + 1);   // the alt offsets
    if (!in.ok || r.base_off[0] != 0) return 2;
    r.len.resize(nl);
    for (size_t k = 0; k < nl; ++k) {   // (what vlr_fragpileup_open_indel and vlr_fragpileup_add_bam check)
        const int64_t l = end[k] - r.start[k];
        if (r.ref_id[k] < 0 || (int64_t)r.ref_id[k] >= r.ra.n_refs || r.start[k] < 0 || l < 1 || l > VLR_FRAGPILEUP_MAX_INDEL_LEN || end[k] > r.ctg_len[(size_t)r.ref_id[k]] ||
            r.base_off[k + 1] < r.base_off[k] || r.kind[k] > VLR_INDELPILEUP_INSERTION)
            return 2;
        r.len[k] = (int32_t)l;
        r.max_locus_len = std::max(r.max_locus_len, l);
    }
    r.altb = in.arr<uint8_t>((size_t)r.base_off[nl]);   // (an indel session has no ref allele bytes: the alt windows stand in for them)
    if (!in.ok) return 2;
    return read_starts(in, r) && read_scores(in, r) ? 0 : 2;
}

// the four windows of an evidence, byte by byte, each into a block of exactly its size
void gather_windows(Run& r, const vlr_bp::Loci& L, const vlr_indelpileup_hit& h, const uint8_t* rec, const vlr_fp::RecMembers& c, size_t* xb, size_t* yb) {
    const int32_t rid = r.ref_id[h.locus];
    const uint8_t* contig = r.ctg[(size_t)rid];
    const int64_t clen = r.ctg_len[(size_t)rid];
    int64_t ab = 0, ae = 0;   // the alt window of an SNV / MNV: the contig with the locus bytes replaced; of an indel: the locus's own
    if (!r.indel) vlr_fp::alt_window(L, (int64_t)h.locus, clen, r.ra.window, &ab, &ae);
    const size_t al = r.indel ? (size_t)(L.base_off[h.locus + 1] - L.base_off[h.locus]) : (size_t)(ae - ab);
    uint8_t* xr = exact<uint8_t>(h.ref_len);
    uint8_t* xa = exact<uint8_t>(al);
    uint8_t* yb_ = exact<uint8_t>(h.read_len);
    uint8_t* yq = exact<uint8_t>(h.read_len);
    for (uint32_t j = 0; j < h.ref_len; ++j) xr[j] = vlr_ip::window_byte(vlr_ip::WB_REF_BASE, contig, clen, h.ref_begin, j);
    for (uint32_t j = 0; j < (uint32_t)al; ++j) xa[j] = r.indel ? L.alt_bases[L.base_off[h.locus] + j] : vlr_fp::alt_window_byte(L, (int64_t)h.locus, contig, clen, ab, j);
    for (uint32_t j = 0; j < h.read_len; ++j) {
        yb_[j] = vlr_ip::window_byte(vlr_ip::WB_READ_BASE, rec + c.seq_off, c.l_seq, h.read_begin, j);
        yq[j] = vlr_ip::window_byte(vlr_ip::WB_READ_QUAL, rec + c.qual_off, c.l_seq, h.read_begin, j);
    }
    r.windows.insert(r.windows.end(), xr, xr + h.ref_len);
    r.windows.insert(r.windows.end(), xa, xa + al);
    r.windows.insert(r.windows.end(), yb_, yb_ + h.read_len);
    r.windows.insert(r.windows.end(), yq, yq + h.read_len);
    *xb += h.ref_len + al; *yb += 2 * (size_t)h.read_len;
    free(xr); free(xa); free(yb_); free(yq);
}

// the members of one record: the member pass of the session's kind
vlr_fp::RecMembers members_of(const Run& r, const vlr_bp::Tables& T, const vlr_bp::Loci& L, const uint8_t* rec, size_t size, uint64_t ordinal, uint64_t coeff,
                              vlr_fp::Member* out, uint64_t room, uint64_t name_off, uint8_t* name_dst, uint64_t xa_off, vlr_fp::AltKey* xa_dst, uint64_t xa_room,
                              const vlr_fp::Realign* rap, vlr_indelpileup_hit* ev_out, uint64_t ev_room, const vlr_fp::Indel* arm) {
    if (r.meth) return vlr_fp::record_members_meth(T, L, r.me, rec, size, ordinal, r.window, coeff, out, room, name_off, name_dst, xa_off, xa_dst, xa_room);
    return vlr_fp::record_members(T, L, rec, size, ordinal, r.realign, r.window, coeff, out, room, name_off, name_dst, xa_off, xa_dst, xa_room, rap, ev_out, ev_room, arm);
}

// member pass: count, then fill into exactly what was counted; the evidences of the members scored and applied
int member_pass(const In& in, size_t blob, Run& r, const vlr_bp::Tables& T, const vlr_bp::Loci& L) {
    const size_t n_rec = (size_t)r.n_rec;
    const uint64_t coeff = 10ull * (uint64_t)r.max_read_len;
    const vlr_fp::Realign* rap = r.realigning ? &r.ra : nullptr;
    struct Records { std::vector<uint8_t*> p; ~Records() { for (uint8_t* q : p) free(q); } } held{std::vector<uint8_t*>(n_rec, nullptr)};
    std::vector<uint8_t*>& recs = held.p;
    std::vector<size_t> sizes(n_rec);
    std::vector<vlr_fp::RecMembers> cnt(n_rec);
    r.cls.resize(n_rec);
    size_t n_name_bytes = 0, n_keys = 0;
    const vlr_fp::Indel count_arm{r.max_locus_len, nullptr};
    for (size_t i = 0; i < n_rec; ++i) {
        sizes[i] = (size_t)(r.starts[i + 1] - r.starts[i]);
        recs[i] = exact<uint8_t>(sizes[i]);   // exactly the record
        if (sizes[i]) memcpy(recs[i], in.d.data() + blob + r.starts[i], sizes[i]);
        cnt[i] = members_of(r, T, L, recs[i], sizes[i], (uint64_t)i, coeff, nullptr, 0, 0, nullptr, 0, nullptr, 0, rap, nullptr, 0, r.indel ? &count_arm : nullptr);
        r.cls[i] = (uint8_t)cnt[i].cls;
        r.n_ev += cnt[i].n_ev;
        r.n_members += cnt[i].n_members;
        n_name_bytes += cnt[i].name_bytes;
        n_keys += cnt[i].n_xa;
    }
    if (r.realigning && r.scores.size() != 2 * r.n_ev) { fprintf(stderr, "%zu evidences, %zu score pairs\n", r.n_ev, r.scores.size() / 2); return 2; }
    r.members = exact<vlr_fp::Member>(r.n_members);
    if (r.indel) r.sides = exact<vlr_fp::Side>(r.n_members);
    r.names = exact<uint8_t>(n_name_bytes);
    r.keys = exact<vlr_fp::AltKey>(n_keys);
    r.ev = exact<vlr_indelpileup_hit>(r.n_ev);
    if (r.indel) r.lx.assign((size_t)r.n_loci, vlr_fragpileup_indel_locus{0, 0, 0, 0});
    size_t m_at = 0, n_at = 0, k_at = 0, e_at = 0;
    for (size_t i = 0; i < n_rec; ++i) {
        const vlr_fp::RecMembers c = cnt[i];
        if (c.n_members) {
            const vlr_fp::Indel arm{r.max_locus_len, r.indel ? r.sides + m_at : nullptr};
            const vlr_fp::RecMembers w = members_of(r, T, L, recs[i], sizes[i], (uint64_t)i, coeff, r.members + m_at, c.n_members, (uint64_t)n_at, r.names + n_at,
                                                     (uint64_t)k_at, r.keys + k_at, c.n_xa, rap, r.ev + e_at, c.n_ev, r.indel ? &arm : nullptr);
            if (w.n_members != c.n_members || w.name_bytes != c.name_bytes || w.n_xa != c.n_xa || w.n_ev != c.n_ev || w.x_bytes != c.x_bytes || w.y_bytes != c.y_bytes ||
                (r.indel && (w.n_ev != w.n_members || w.max_del != c.max_del || w.max_ins != c.max_ins || w.max_clip != c.max_clip))) {
                fprintf(stderr, "count and fill pass differ at record %lld\n", (long long)i);
                return 3;
            }
            // the evidences of the record, as the fill kernel pairs them with its members: of an indel session evidence k belongs to member k,
            // of the others to the flagged members in their order
            size_t e = 0, xb = 0, yb = 0;
            for (uint32_t k = 0; k < c.n_members && e < c.n_ev; ++k) {
                vlr_fp::Member& m = r.members[m_at + k];
                if (!r.indel && (!(m.bits & vlr_fp::M_ENCLOSING) || !(m.status & VLR_BASEPILEUP_HIT_NEEDS_REALIGN))) continue;
                vlr_indelpileup_hit& h = r.ev[e_at + e];
                if (h.locus != m.locus || h.record != m.ordinal) { fprintf(stderr, "evidence and member differ at record %lld\n", (long long)i); return 3; }
                if (r.indel) {   // the maxima of the locus, as the fill kernel folds them
                    vlr_fragpileup_indel_locus& x = r.lx[m.locus];
                    x.max_del = std::max(x.max_del, c.max_del);
                    x.max_ins = std::max(x.max_ins, c.max_ins);
                    if (c.max_clip && c.l_seq) {
                        const uint64_t mine = ((uint64_t)c.max_clip << 32) | c.l_seq, seen = ((uint64_t)x.max_clip << 32) | x.max_clip_l_seq;
                        if (vlr_fp::clip_frac_greater(mine, seen)) { x.max_clip = c.max_clip; x.max_clip_l_seq = c.l_seq; }
                    }
                }
                h.ln_ref = r.scores[2 * (e_at + e)]; h.ln_alt = r.scores[2 * (e_at + e) + 1];
                if (!h.status) gather_windows(r, L, h, recs[i], c, &xb, &yb);
                double pr = h.ln_ref, pa = h.ln_alt;
                vlr_fp::normalize_support(&pr, &pa);
                vlr_fp::apply_realigned(m, h, pr, pa);
                ++e;
            }
            if (e != c.n_ev || xb != c.x_bytes || yb != c.y_bytes) {
                fprintf(stderr, r.indel ? "the bytes of the evidences differ from the count at record %lld\n" : "evidences and their bytes differ from the count at record %lld\n",
                        (long long)i);
                return 3;
            }
        }
        e_at += c.n_ev;
        m_at += c.n_members;
        n_at += c.name_bytes;
        k_at += c.n_xa;
        free(recs[i]);
        recs[i] = nullptr;
    }
    return 0;
}

// fragment pass of one locus: its members idx sorted by name, a fragment per run of equal names, the major read position (SNV / MNV),
// the alt-locus class of every observation
void fragment_pass(Run& r, size_t l, std::vector<uint32_t>& idx) {
    const vlr_fp::Member* members = r.members;
    const uint8_t* names = r.names;
    const vlr_fp::AltKey* keys = r.keys;
    const uint32_t n = (uint32_t)idx.size();
    vlr_fragpileup_locus& lr = r.lrec[l];
    lr = vlr_fragpileup_locus{(int64_t)r.obs.size(), n, 0, VLR_BASEPILEUP_NO_READ_POSITION, 0};
    if (n > VLR_FRAGPILEUP_MAX_MEMBERS) { lr.status = VLR_FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS; return; }
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return vlr_fp::member_less(names, members[a], members[b]); });
    const size_t first = r.obs.size();
    std::vector<uint32_t> pos_keys, alt_idx;
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    for (uint32_t i = 0; i < n; ++i) {
        if (i > 0 && vlr_fp::compare_names(names, members[idx[i - 1]], members[idx[i]]) == 0) continue;
        vlr_fragpileup_obs o;
        vlr_fragpileup_indel_obs x{};
        uint32_t ml, mr;
        if (r.indel ? !vlr_fp::run_obs_indel(members, r.sides, names, idx.data(), i, n, r.kind[l], r.start[l], (int64_t)r.len[l], r.has_isize, (uint32_t)r.max_mapq, o, x, &ml, &mr)
                    : !vlr_fp::run_obs(members, names, idx.data(), i, n, (uint32_t)r.max_mapq, o, &ml, &mr))
            continue;
        if (!r.indel && vlr_fp::counts_for_major(o)) pos_keys.push_back(o.read_position);
        for (uint32_t k = 0; k < members[ml].xa_n; ++k) alt_idx.push_back((uint32_t)(members[ml].xa_off + k));
        if (mr != 0xffffffffu) for (uint32_t k = 0; k < members[mr].xa_n; ++k) alt_idx.push_back((uint32_t)(members[mr].xa_off + k));
        pairs.push_back({ml, mr});
        r.obs.push_back(o);
        if (r.indel) r.obsx.push_back(x);
    }
    if (alt_idx.size() > VLR_FRAGPILEUP_MAX_MEMBERS) {
        r.obs.resize(first);
        if (r.indel) r.obsx.resize(first);
        lr.status = VLR_FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI;
        return;
    }
    std::sort(pos_keys.begin(), pos_keys.end());
    bool found = false;
    const uint32_t major = vlr_fp::major_of_sorted(pos_keys.data(), (uint32_t)pos_keys.size(), &found);
    std::sort(alt_idx.begin(), alt_idx.end(), [&](uint32_t a, uint32_t b) { return vlr_fp::key_less(keys[a], keys[b]); });
    const int64_t at_major = vlr_fp::major_key_of_sorted(keys, alt_idx.data(), (uint32_t)alt_idx.size());
    const bool have = at_major >= 0;
    const vlr_fp::AltKey mk = have ? keys[alt_idx[(size_t)at_major]] : vlr_fp::AltKey{0, 0};
    lr.n_obs = (uint32_t)(r.obs.size() - first);
    if (found) lr.major_read_position = major;
    for (size_t k = first; k < r.obs.size(); ++k) {
        if (found && r.obs[k].status == 0 && r.obs[k].read_position == major) r.obs[k].bits |= VLR_FRAGPILEUP_READPOS_MAJOR;
        const auto& pr = pairs[k - first];
        r.obs[k].alt_locus = vlr_fp::alt_locus_class(keys, members[pr.first], pr.second != 0xffffffffu ? &members[pr.second] : nullptr, have, mk);
    }
}

template <class T> void put(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }

// i64 n_evidences, the evidences, their windows
void put_evidences(FILE* f, const Run& r) {
    const int64_t ne = (int64_t)r.n_ev;
    put(f, &ne, 1);
    put(f, r.ev, r.n_ev);
    put(f, r.windows.data(), r.windows.size());
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 && argc != 5) { fprintf(stderr, "usage: %s <input> <output> [<realign input> <realign output>]\n", argv[0]); return 2; }
    In in;
    if (!slurp(argv[1], in)) return 2;
    const uint8_t* magic = in.take(4);
    Run r;
    int rc;
    if (magic && (memcmp(magic, "VFIH", 4) == 0 || memcmp(magic, "VFMH", 4) == 0)) {
        if (argc != 3) { fprintf(stderr, "usage: %s <input> <output>\n", argv[0]); return 2; }
        rc = magic[2] == 'I' ? read_indel(in, r) : read_meth(in, r);
    } else {
        rc = read_snv(in, magic, argc == 5 ? argv[3] : nullptr, r);
    }
    if (rc != 0) return rc;
    const size_t blob = in.o, nl = (size_t)r.n_loci;
    for (size_t i = 0; i < (size_t)r.n_rec; ++i)
        if (r.starts[i] > r.starts[i + 1] || r.starts[i + 1] > in.d.size() - blob) return 2;

    vlr_bp::fill_tables(r.tab.data(), r.tab.data() + 256, r.tab.data() + 512);
    const vlr_bp::Tables T{r.tab.data(), r.tab.data() + 256, r.tab.data() + 512, vlr_bp::ln_confusion(), vlr_bp::ln_any()};
    const vlr_bp::Loci L{r.n_loci, r.ref_id.data(), r.start.data(), r.len.data(), r.kind.data(), r.base_off.data(), r.indel ? r.altb.data() : r.refb.data(), r.altb.data()};
    if ((rc = member_pass(in, blob, r, T, L)) != 0) return rc;
    std::vector<std::vector<uint32_t>> per(nl);
    for (size_t m = r.n_members; m-- > 0;) per[r.members[m].locus].push_back((uint32_t)m);
    r.lrec.resize(nl);
    for (size_t l = 0; l < nl; ++l) fragment_pass(r, l, per[l]);

    if (argc == 5) {
        FILE* ro = fopen(argv[4], "wb");
        if (!ro) { perror(argv[4]); return 2; }
        put_evidences(ro, r);
        fclose(ro);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int64_t n_obs = (int64_t)r.obs.size();
    if (!r.indel) put(o, r.tab.data(), 512);
    if (r.meth) put(o, r.mtab.data(), 512);
    put(o, &n_obs, 1);
    put(o, r.obs.data(), r.obs.size());
    put(o, r.obsx.data(), r.obsx.size());
    put(o, r.lrec.data(), nl);
    if (r.indel) {
        put(o, r.lx.data(), nl);
        put_evidences(o, r);
    } else {
        put(o, r.cls.data(), r.cls.size());
    }
    fclose(o);
    return 0;
}
