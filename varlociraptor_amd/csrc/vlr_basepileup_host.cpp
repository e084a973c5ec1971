// vlr_basepileup_host.cpp — the scoring of vlr_basepileup.h compiled for the CPU: the same text the kernel of vlr_basepileup.hip runs, as a
// small program that tests/test_basepileup_host.py builds with -fsanitize=address,undefined and runs over fixtures and over truncated
// and corrupted records.  Not part of libvlr.so.
//
//   vlr_basepileup_host <input> <output>
// input  (little endian): "VBPH", i32 realign_indel_reads, i64 n_loci, i32 ref_id[n], i64 start[n], i32 len[n], u8 kind[n],
//        ref bases, alt bases (sum of len bytes each), i64 n_records, u64 starts[n_records + 1], the records one behind the other
// output: f64 call[256], f64 miscall[256], i64 n_hits, the hits locus-major (vlr_basepileup_hit), u8 class[n_records]
//        (0 scored, 1 rejected by the flag rule, 2 bad record)
// Every record is copied into a heap block of exactly its size before it is scored, so that a read past its end is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vlr_basepileup.h"

static_assert(sizeof(vlr_basepileup_hit) == 48, "hit layout");

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
    if (!magic || memcmp(magic, "VBPH", 4) != 0) { fprintf(stderr, "bad input\n"); return 2; }
    const int32_t realign = in.arr<int32_t>(1)[0];
    const int64_t n_loci = in.arr<int64_t>(1)[0];
    if (!in.ok || n_loci < 0 || n_loci > (1 << 24)) return 2;
    const auto ref_id = in.arr<int32_t>((size_t)n_loci);
    const auto start = in.arr<int64_t>((size_t)n_loci);
    const auto len = in.arr<int32_t>((size_t)n_loci);
    const auto kind = in.arr<uint8_t>((size_t)n_loci);
    if (!in.ok) return 2;
    std::vector<uint64_t> base_off((size_t)n_loci + 1, 0);
    for (int64_t k = 0; k < n_loci; ++k) {
        if (len[(size_t)k] < 1 || len[(size_t)k] > VLR_BASEPILEUP_MAX_LEN) return 2;
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

    std::vector<vlr_basepileup_hit> raw;
    std::vector<uint8_t> cls((size_t)n_rec);
    for (int64_t i = 0; i < n_rec; ++i) {
        const size_t size = (size_t)(starts[(size_t)i + 1] - starts[(size_t)i]);
        uint8_t* rec = (uint8_t*)malloc(size ? size : 1);   // exactly the record: the sanitizer sees any byte read behind it
        if (size) memcpy(rec, in.d.data() + blob + starts[(size_t)i], size);
        // the two passes of the kernel: count, then fill into exactly that many
        const vlr_bp::RecResult c = vlr_bp::record_hits(T, L, rec, size, (uint64_t)i, realign != 0, nullptr, 0);
        const size_t at = raw.size();
        raw.resize(at + c.n_hits);
        const vlr_bp::RecResult w = vlr_bp::record_hits(T, L, rec, size, (uint64_t)i, realign != 0, c.n_hits ? raw.data() + at : nullptr, c.n_hits);
        if (w.n_hits != c.n_hits || w.cls != c.cls) { fprintf(stderr, "count and fill pass differ at record %lld\n", (long long)i); return 3; }
        cls[(size_t)i] = (uint8_t)c.cls;
        free(rec);
    }
    std::vector<uint64_t> first((size_t)n_loci + 1, 0);
    for (const auto& h : raw) ++first[(size_t)h.locus + 1];
    for (size_t k = 0; k < (size_t)n_loci; ++k) first[k + 1] += first[k];
    std::vector<vlr_basepileup_hit> hits(raw.size());
    for (const auto& h : raw) hits[(size_t)first[h.locus]++] = h;

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int64_t n_hits = (int64_t)hits.size();
    fwrite(tab.data(), 8, 512, o);
    fwrite(&n_hits, 8, 1, o);
    if (n_hits) fwrite(hits.data(), sizeof(vlr_basepileup_hit), (size_t)n_hits, o);
    if (n_rec) fwrite(cls.data(), 1, (size_t)n_rec, o);
    fclose(o);
    return 0;
}
