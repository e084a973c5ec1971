// vlr_altvariants_host.cpp — the text of vlr_altvariants.h compiled for the CPU: what the kernels frag_alt_expand_kernel, frag_alt_select_kernel,
// frag_alt_compact_kernel and frag_alt_collect_kernel of vlr_fragpileup.hip run on a range of evidences, as a small program that
// tests/test_altvariants_host_program.py builds with -fsanitize=address,undefined and runs.  Not part of libvlr.so.
//
//   vlr_altvariants_host <input> <output>
// input (little endian): "VAVH", i64 n_loci, u64 comp_off[n_loci + 1], i64 n_base_off, u64 base_off[n_base_off], the competitor windows one
//        behind the other, u64 max_window, i32 fast, i64 n_ev, per evidence u32 (locus, status, ref_len, alt_len, read_len), then per
//        evidence its ref window, alt window, read bases and read qualities, i64 n_pairs, i32 dist[n_pairs], f64 lnp[n_pairs]: the edit distance
//        and the pair-HMM score of EVERY pair of the layout (the program takes the scores of the pairs it keeps)
// output: i32 bad, i64 where (vlr_av::check_table; bad != 0 ends the output), i64 n_pairs, i64 n_kept, u32 xoff[n_pairs + 1], u32 yoff[n_pairs + 1],
//        the expanded x / y / q bytes, u32 cxoff[n_kept + 1], u32 cyoff[n_kept + 1], i32 cband[n_kept], the compacted x / y / q bytes, per
//        evidence f64 ln_ref, f64 ln_alt, i32 dist_ref, i32 dist_alt and its vlr_fragpileup_alt_hit
// Every window, every offset array and every byte array lies in a heap block of exactly its size, so that a read or write past one is a
// sanitizer report; the lane-strided loops run with 64 lanes, one lane after the other.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vlr_altvariants.h"

static_assert(sizeof(vlr_fragpileup_alt_hit) == 8, "alt hit layout");

namespace {

struct In {
    std::vector<uint8_t> d;
    size_t o = 0;
    bool ok = true;
    template <class T> std::vector<T> arr(size_t n) {
        if (n > (d.size() - o) / sizeof(T)) { ok = false; return std::vector<T>(n ? 1 : 0); }
        std::vector<T> v(n);
        if (n) memcpy(v.data(), d.data() + o, n * sizeof(T));
        o += n * sizeof(T);
        return v;
    }
    template <class T> T one() { return arr<T>(1)[0]; }
};

template <class T> void put(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }
template <class T> void put1(FILE* f, T v) { fwrite(&v, sizeof(T), 1, f); }

struct Ev { uint32_t locus, status, ref_len, alt_len, read_len; };

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: vlr_altvariants_host <input> <output>\n"); return 2; }
    In in;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    in.d.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (!in.d.empty() && fread(in.d.data(), 1, in.d.size(), f) != in.d.size()) { fclose(f); return 2; }
    fclose(f);
    const std::vector<uint8_t> magic = in.arr<uint8_t>(4);
    if (!in.ok || memcmp(magic.data(), "VAVH", 4) != 0) { fprintf(stderr, "bad magic\n"); return 2; }
    const int64_t n_loci = in.one<int64_t>();
    const std::vector<uint64_t> comp_off = in.arr<uint64_t>((size_t)n_loci + 1);
    const int64_t n_boff = in.one<int64_t>();
    const std::vector<uint64_t> base_off = in.arr<uint64_t>((size_t)n_boff);
    if (!in.ok) return 2;
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    // the windows' bytes: as many as the last offset says
    const uint64_t n_comp = comp_off[(size_t)n_loci];
    const std::vector<uint8_t> bases = in.arr<uint8_t>(n_boff > 0 ? (size_t)base_off[(size_t)n_boff - 1] : 0);
    const uint64_t limit = in.one<uint64_t>();
    if (!in.ok) { fprintf(stderr, "short input\n"); fclose(out); return 2; }
    // (check_table walks base_off over comp_off[n_loci] + 1 entries once comp_off proved ascending and no locus has too many: offsets
    // that do not cover the competitors are refused here, as the session refuses a null pointer)
    int64_t where = 0;
    int bad = vlr_av::check_table(n_loci, comp_off.data(), nullptr, limit, &where);
    if (bad == 0 && n_comp > 0) bad = (uint64_t)n_boff < n_comp + 1 ? 1 : vlr_av::check_table(n_loci, comp_off.data(), base_off.data(), limit, &where);
    put1<int32_t>(out, bad);
    put1<int64_t>(out, where);
    if (bad) { fclose(out); return 0; }
    const int32_t fast = in.one<int32_t>();
    const int64_t n_ev = in.one<int64_t>();
    std::vector<Ev> ev((size_t)n_ev);
    for (auto& e : ev) { const std::vector<uint32_t> v = in.arr<uint32_t>(5); e = Ev{v[0], v[1], v[2], v[3], v[4]}; }
    std::vector<std::vector<uint8_t>> sx((size_t)n_ev), sy((size_t)n_ev), sq((size_t)n_ev);
    for (size_t e = 0; e < ev.size(); ++e) {
        sx[e] = in.arr<uint8_t>((size_t)ev[e].ref_len + ev[e].alt_len);
        sy[e] = in.arr<uint8_t>(ev[e].read_len);
        sq[e] = in.arr<uint8_t>(ev[e].read_len);
    }
    const int64_t n_pairs_in = in.one<int64_t>();
    const std::vector<int32_t> dist = in.arr<int32_t>((size_t)n_pairs_in);
    const std::vector<double> lnp_in = in.arr<double>((size_t)n_pairs_in);
    if (!in.ok) { fprintf(stderr, "short input\n"); fclose(out); return 2; }
    const vlr_av::Table t{n_loci, comp_off.data(), base_off.data(), bases.data()};
    // the layout
    std::vector<uint32_t> pair_base(ev.size() + 1, 0), xoff(1, 0), yoff(1, 0);
    uint32_t xl[vlr_av::kMaxPairs], yl[vlr_av::kMaxPairs];
    for (size_t e = 0; e < ev.size(); ++e) {
        if ((int64_t)ev[e].locus >= n_loci) { fprintf(stderr, "evidence %zu: locus out of range\n", e); fclose(out); return 2; }
        const uint32_t np = vlr_av::layout_evidence(t, ev[e].locus, ev[e].status == 0, ev[e].ref_len, ev[e].alt_len, ev[e].read_len, xl, yl);
        pair_base[e + 1] = pair_base[e] + np;
        for (uint32_t j = 0; j < np; ++j) { xoff.push_back(xoff.back() + xl[j]); yoff.push_back(yoff.back() + yl[j]); }
    }
    const size_t np = pair_base[ev.size()];
    if ((int64_t)np != n_pairs_in) { fprintf(stderr, "the input scores %lld pairs, the layout has %zu\n", (long long)n_pairs_in, np); fclose(out); return 2; }
    xoff.shrink_to_fit(); yoff.shrink_to_fit();
    std::vector<uint8_t> x(xoff[np]), y(yoff[np]), q(yoff[np]);
    // expand: an evidence with a status is skipped, as in the kernel
    for (size_t e = 0; e < ev.size(); ++e) {
        if (ev[e].status) continue;
        for (uint32_t lane = 0; lane < 64; ++lane)
            vlr_av::expand_evidence(lane, 64, t, ev[e].locus, pair_base[e + 1] - pair_base[e] - 2, sx[e].data(), ev[e].ref_len, ev[e].alt_len, sy[e].data(), sq[e].data(),
                                    ev[e].read_len, xoff.data(), yoff.data(), pair_base[e], x.data(), y.data(), q.data());
    }
    // select
    std::vector<uint32_t> keep(np), klx(np), kly(np);
    std::vector<int32_t> band(np);
    for (size_t e = 0; e < ev.size(); ++e) {
        const uint32_t p0 = pair_base[e], n = pair_base[e + 1] - p0;
        const vlr_av::Selected s = vlr_av::select(dist.data() + p0, n - 2);
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t p = p0 + j, on = (s.keep >> j) & 1u;
            keep[p] = on;
            klx[p] = on ? xoff[p + 1] - xoff[p] : 0u;
            kly[p] = on ? yoff[p + 1] - yoff[p] : 0u;
            band[p] = vlr_av::band_of(dist[p], fast != 0);
        }
    }
    // the three scans
    std::vector<uint64_t> slot(np), cx_at(np), cy_at(np);
    uint64_t n_kept = 0, x_total = 0, y_total = 0;
    for (size_t p = 0; p < np; ++p) { slot[p] = n_kept; cx_at[p] = x_total; cy_at[p] = y_total; n_kept += keep[p]; x_total += klx[p]; y_total += kly[p]; }
    // compact
    std::vector<uint32_t> cxoff((size_t)n_kept + 1), cyoff((size_t)n_kept + 1);
    std::vector<int32_t> cband((size_t)n_kept);
    std::vector<uint8_t> cx((size_t)x_total), cy((size_t)y_total), cq((size_t)y_total);
    std::vector<double> clnp((size_t)n_kept);
    for (size_t p = 0; p < np; ++p) {
        if (!keep[p]) continue;
        for (uint32_t lane = 0; lane < 64; ++lane)
            vlr_av::compact_pair(lane, 64, xoff.data(), yoff.data(), x.data(), y.data(), q.data(), (uint32_t)p, band[p], slot[p], cx_at[p], cy_at[p], n_kept, x_total, y_total,
                                 cxoff.data(), cyoff.data(), cband.data(), cx.data(), cy.data(), cq.data());
        clnp[(size_t)slot[p]] = lnp_in[p];
    }
    // collect
    std::vector<vlr_indelpileup_hit> hits(ev.size());
    std::vector<vlr_fragpileup_alt_hit> alt(ev.size());
    for (size_t e = 0; e < ev.size(); ++e) {
        memset(&hits[e], 0, sizeof(hits[e]));
        const uint32_t p0 = pair_base[e];
        vlr_av::collect_evidence(dist.data() + p0, pair_base[e + 1] - p0 - 2, slot.data() + p0, clnp.data(), n_kept, &hits[e], &alt[e]);
    }
    put1<int64_t>(out, (int64_t)np);
    put1<int64_t>(out, (int64_t)n_kept);
    put(out, xoff); put(out, yoff); put(out, x); put(out, y); put(out, q);
    put(out, cxoff); put(out, cyoff); put(out, cband); put(out, cx); put(out, cy); put(out, cq);
    for (size_t e = 0; e < ev.size(); ++e) {
        put1<double>(out, hits[e].ln_ref); put1<double>(out, hits[e].ln_alt);
        put1<int32_t>(out, hits[e].dist_ref); put1<int32_t>(out, hits[e].dist_alt);
        fwrite(&alt[e], sizeof(alt[e]), 1, out);
    }
    fclose(out);
    return 0;
}
