// vlr_indelpileup_host.cpp — the evidence text of vlr_indelpileup.h compiled for the CPU: the same text the kernels of vlr_indelpileup.hip
// run, as a small program that tests/test_indelpileup_host.py builds with -fsanitize=address,undefined and runs over the hand records,
// the synthetic set, the fixtures and over truncated and corrupted records.  Not part of libvlr.so.
//
//   vlr_indelpileup_host <input> <output>
// input  (little endian): "VIPH", i32 window, i64 n_loci, i32 ref_id[n], i64 start[n], i64 end[n], u64 alt_off[n + 1], the alt allele
//        windows (alt_off[n] bytes), i64 n_refs, i64 ctg_len[n_refs] (-1: no such contig in the reference), the contigs one behind the
//        other (case as in the FASTA: upper-cased here, as the session does at upload), i64 n_records, u64 starts[n_records + 1], the
//        records one behind the other
// output: i64 n_hits, the descriptors locus-major (vlr_indelpileup_hit; scores zero, distances -1), u32 x_offset[2 n_hits + 1],
//        u32 y_offset[2 n_hits + 1], x bases, y bases, y qualities (pairs 2e = (ref allele, read), 2e + 1 = (alt allele, read) of hit e),
//        u8 class[n_records] (0 followed, 1 rejected by the flag rule, 2 bad record)
// Every record is copied into a heap block of exactly its size before it is looked at, and every contig into one of exactly its
// length, so that a read past either end is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vlr_indelpileup.h"

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

struct Windows { std::vector<uint8_t> x_ref, x_alt, y, q; };

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <input> <output>\n", argv[0]); return 2; }
    In in;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    in.d.resize((size_t)sz);
    if (sz && fread(in.d.data(), 1, (size_t)sz, f) != (size_t)sz) { fclose(f); return 2; }
    fclose(f);
    const uint8_t* magic = in.take(4);
    if (!magic || memcmp(magic, "VIPH", 4) != 0) { fprintf(stderr, "bad input\n"); return 2; }
    const int32_t window = in.arr<int32_t>(1)[0];
    const int64_t n_loci = in.arr<int64_t>(1)[0];
    if (!in.ok || n_loci < 0 || n_loci > (1 << 24) || window < 1 || window > VLR_INDELPILEUP_MAX_WINDOW) return 2;
    const auto ref_id = in.arr<int32_t>((size_t)n_loci);
    const auto start = in.arr<int64_t>((size_t)n_loci);
    const auto end = in.arr<int64_t>((size_t)n_loci);
    const auto alt_off = in.arr<uint64_t>((size_t)n_loci + 1);
    if (!in.ok || alt_off[0] != 0) return 2;
    int64_t max_len = 0;
    for (int64_t k = 0; k < n_loci; ++k) {
        if (alt_off[(size_t)k + 1] < alt_off[(size_t)k] || end[(size_t)k] <= start[(size_t)k] || start[(size_t)k] < 0 || ref_id[(size_t)k] < 0) return 2;
        if (end[(size_t)k] - start[(size_t)k] > max_len) max_len = end[(size_t)k] - start[(size_t)k];
    }
    const auto altb = in.arr<uint8_t>((size_t)alt_off[(size_t)n_loci]);
    const int64_t n_refs = in.arr<int64_t>(1)[0];
    if (!in.ok || n_refs < 0 || n_refs > (1 << 20)) return 2;
    const auto ctg_len = in.arr<int64_t>((size_t)n_refs);
    if (!in.ok) return 2;
    std::vector<uint8_t*> ctg((size_t)n_refs, nullptr);
    for (int64_t k = 0; k < n_refs; ++k) {
        if (ctg_len[(size_t)k] < 0) continue;
        const uint8_t* p = in.take((size_t)ctg_len[(size_t)k]);
        if (!in.ok) return 2;
        ctg[(size_t)k] = (uint8_t*)malloc(ctg_len[(size_t)k] ? (size_t)ctg_len[(size_t)k] : 1);   // exactly the contig
        for (int64_t j = 0; j < ctg_len[(size_t)k]; ++j) ctg[(size_t)k][j] = (p[j] >= 'a' && p[j] <= 'z') ? (uint8_t)(p[j] - 32) : p[j];
    }
    for (int64_t k = 0; k < n_loci; ++k)
        if (ref_id[(size_t)k] >= n_refs || ctg_len[(size_t)ref_id[(size_t)k]] < 0) return 2;
    const int64_t n_rec = in.arr<int64_t>(1)[0];
    if (!in.ok || n_rec < 0 || n_rec > (1 << 24)) return 2;
    const auto starts = in.arr<uint64_t>((size_t)n_rec + 1);
    if (!in.ok) return 2;
    const size_t blob = in.o;
    for (int64_t i = 0; i < n_rec; ++i)
        if (starts[(size_t)i] > starts[(size_t)i + 1] || starts[(size_t)i + 1] > in.d.size() - blob) return 2;

    const vlr_ip::Loci L{n_loci, ref_id.data(), start.data(), end.data(), alt_off.data(), max_len, n_refs, ctg_len.data()};

    std::vector<vlr_indelpileup_hit> raw;
    std::vector<Windows> raw_w;
    std::vector<uint8_t> cls((size_t)n_rec);
    for (int64_t i = 0; i < n_rec; ++i) {
        const size_t size = (size_t)(starts[(size_t)i + 1] - starts[(size_t)i]);
        uint8_t* rec = (uint8_t*)malloc(size ? size : 1);   // exactly the record: the sanitizer sees any byte read behind it
        if (size) memcpy(rec, in.d.data() + blob + starts[(size_t)i], size);
        // the two passes of the kernels: count, then fill into exactly that many
        const vlr_ip::RecEvidence c = vlr_ip::record_evidence(L, rec, size, (uint64_t)i, window, nullptr, 0);
        const size_t at = raw.size();
        raw.resize(at + c.n_ev);
        const vlr_ip::RecEvidence w = vlr_ip::record_evidence(L, rec, size, (uint64_t)i, window, c.n_ev ? raw.data() + at : nullptr, c.n_ev);
        if (w.n_ev != c.n_ev || w.cls != c.cls || w.x_bytes != c.x_bytes || w.y_bytes != c.y_bytes) {
            fprintf(stderr, "count and fill pass differ at record %lld\n", (long long)i);
            return 3;
        }
        cls[(size_t)i] = (uint8_t)c.cls;
        // the gather pass: every window byte through window_byte
        uint64_t xb = 0, yb = 0;
        for (size_t e = at; e < raw.size(); ++e) {
            const vlr_indelpileup_hit& h = raw[e];
            Windows wd;
            if (!h.status) {
                const int32_t id = ref_id[h.locus];
                for (uint32_t k = 0; k < h.ref_len; ++k) wd.x_ref.push_back(vlr_ip::window_byte(vlr_ip::WB_REF_BASE, ctg[(size_t)id], ctg_len[(size_t)id], h.ref_begin, k));
                wd.x_alt.assign(altb.begin() + (long)alt_off[h.locus], altb.begin() + (long)alt_off[h.locus + 1]);
                for (uint32_t k = 0; k < h.read_len; ++k) {
                    wd.y.push_back(vlr_ip::window_byte(vlr_ip::WB_READ_BASE, rec + w.seq_off, w.l_seq, h.read_begin, k));
                    wd.q.push_back(vlr_ip::window_byte(vlr_ip::WB_READ_QUAL, rec + w.qual_off, w.l_seq, h.read_begin, k));
                }
            }
            xb += wd.x_ref.size() + wd.x_alt.size();
            yb += 2 * wd.y.size();
            raw_w.push_back(wd);
        }
        if (xb != c.x_bytes || yb != c.y_bytes) { fprintf(stderr, "counted and gathered bytes differ at record %lld\n", (long long)i); return 3; }
        free(rec);
    }
    // locus-major, record order kept within a locus
    std::vector<uint64_t> first((size_t)n_loci + 1, 0);
    for (const auto& h : raw) ++first[(size_t)h.locus + 1];
    for (size_t k = 0; k < (size_t)n_loci; ++k) first[k + 1] += first[k];
    std::vector<vlr_indelpileup_hit> hits(raw.size());
    std::vector<const Windows*> hw(raw.size());
    for (size_t k = 0; k < raw.size(); ++k) {
        const size_t to = (size_t)first[raw[k].locus]++;
        hits[to] = raw[k];
        hw[to] = &raw_w[k];
    }
    std::vector<uint32_t> xo(2 * hits.size() + 1, 0), yo(2 * hits.size() + 1, 0);
    std::vector<uint8_t> xb, yb, qb;
    for (size_t k = 0; k < hits.size(); ++k) {
        const Windows& w = *hw[k];
        xb.insert(xb.end(), w.x_ref.begin(), w.x_ref.end());
        xo[2 * k + 1] = (uint32_t)xb.size();
        xb.insert(xb.end(), w.x_alt.begin(), w.x_alt.end());
        xo[2 * k + 2] = (uint32_t)xb.size();
        for (int j = 0; j < 2; ++j) {
            yb.insert(yb.end(), w.y.begin(), w.y.end());
            qb.insert(qb.end(), w.q.begin(), w.q.end());
            yo[2 * k + 1 + (size_t)j] = (uint32_t)yb.size();
        }
    }
    for (uint8_t* c : ctg) free(c);

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int64_t n_hits = (int64_t)hits.size();
    fwrite(&n_hits, 8, 1, o);
    if (n_hits) fwrite(hits.data(), sizeof(vlr_indelpileup_hit), (size_t)n_hits, o);
    fwrite(xo.data(), 4, xo.size(), o);
    fwrite(yo.data(), 4, yo.size(), o);
    if (!xb.empty()) fwrite(xb.data(), 1, xb.size(), o);
    if (!yb.empty()) fwrite(yb.data(), 1, yb.size(), o);
    if (!qb.empty()) fwrite(qb.data(), 1, qb.size(), o);
    if (n_rec) fwrite(cls.data(), 1, (size_t)n_rec, o);
    fclose(o);
    return 0;
}
