// vlr_ingest_host.cpp — the parsers of the front door as a small program without HIP: the host units vlr_bgzf.cpp, vlr_ingest.cpp and
// vlr_callsfile.cpp (BGZF members, the BCF2 container, bincode vectors, VCF text) linked against the outside symbols they reference,
// which this file supplies: the library's error text and host allocator over malloc, and every device entry point the units name as
// a function that prints its name and exits 3.  tests/test_ingest_host_program.py builds it with -fsanitize=address,undefined and
// runs it over the fixtures and over truncated and overwritten copies of them.  Not part of libvlr.so.
//
//   vlr_ingest_host obs <file>...     vlr_obs_read of the file, then the streaming reader at 1 and at 7 records per call; one line each:
//                                     "<pass> n_loci=<n> n_obs=<n> checksum=<8 hex digits>"
//   vlr_ingest_host calls <file>...   open_calls + read_call_records without and with ANN / AF, variant_types and tags_prob_sum over
//                                     every record; one line per pass: "<pass> n_records=<n> n_variants=<n> n_sums=<n> checksum=<hex>",
//                                     the second followed by " n_ann=<n> n_af=<n>"
//   vlr_ingest_host <mode> <file> ff <begin> <end>
//                                     the same over the (writable) file with each byte of [begin, end) in turn set to 0xff and put
//                                     back afterwards: thousands of damaged inputs in one process
// Every input is framed by a line "@<file>" (ff: "@<offset>") in front of its output and a line "=<code>" behind it: 0 with the
// digest, 2 with "error <code>: <text>" (the library's error text) when the library refuses the input.  The program exits with the
// largest code of its inputs, with 3 at once when a host path reaches for the device, with 1 on a wrong command line; a sanitizer
// report ends it where it stands, behind the "@" line of the input that caused it.  Threads run at 2.
//
// The checksum of a table does not depend on how the file was cut into tables: every array has a CRC32 of its own that runs on over
// the tables of a pass (per pileup the observation count, the nine columns, flags, third-allele evidence, the four per-locus byte
// arrays, position, the two priors, imprecise, the group key, and per locus the strings contig, ID, REF, ALT each with its NUL); the
// checksum is the CRC32 of those values, in that order, as little-endian 32-bit words.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vlr_hostio.h"

using namespace vlr_hostio;

// ------------------------------------------------------------------------------------------------ what the library supplies
namespace {
std::string g_error;
[[noreturn]] void device_call(const char* name) {
    printf("device entry point reached: %s\n", name);
    fflush(stdout);
    _Exit(3);
}
}  // namespace
#define DEVICE(name) { device_call(#name); }

extern "C" {
void vlr_set_error(const char* msg) { g_error = msg ? msg : ""; }
const char* vlr_last_error(void) { return g_error.c_str(); }
void* vlr_host_alloc(size_t bytes) { return malloc(bytes ? bytes : 1); }
void vlr_host_free(void* p) { free(p); }
// the device entry points the three units name (vlr_gpuio.h, vlr_callstats.h, include/vlr.h), with their signatures
int vlr_dev_file_create(int, vlr_dev_file**) DEVICE(vlr_dev_file_create)
void vlr_dev_file_destroy(vlr_dev_file*) DEVICE(vlr_dev_file_destroy)
void vlr_dev_file_trim() DEVICE(vlr_dev_file_trim)
uint64_t vlr_dev_file_buffered(const vlr_dev_file*) DEVICE(vlr_dev_file_buffered)
int vlr_dev_file_feed(vlr_dev_file*, const uint8_t*, size_t, const vlr::InflateBlock*, int, uint64_t) DEVICE(vlr_dev_file_feed)
int vlr_dev_file_feed_pieces(vlr_dev_file*, const uint8_t* const*, const size_t*, int, const vlr::InflateBlock*, int, uint64_t) DEVICE(vlr_dev_file_feed_pieces)
int vlr_dev_file_feed_wait(vlr_dev_file*) DEVICE(vlr_dev_file_feed_wait)
int vlr_dev_file_feed_wait_oldest(vlr_dev_file*) DEVICE(vlr_dev_file_feed_wait_oldest)
int vlr_dev_file_wait_ready(vlr_dev_file*, uint64_t) DEVICE(vlr_dev_file_wait_ready)
int vlr_dev_file_feeds_in_flight(const vlr_dev_file*) DEVICE(vlr_dev_file_feeds_in_flight)
double vlr_dev_file_inflate_seconds(vlr_dev_file*, int) DEVICE(vlr_dev_file_inflate_seconds)
int vlr_dev_file_skip(vlr_dev_file*, uint64_t) DEVICE(vlr_dev_file_skip)
int vlr_dev_file_split(vlr_dev_file*, int64_t, int, int, const int8_t*, int, int64_t*, const vlr::RecHost**, int*) DEVICE(vlr_dev_file_split)
int vlr_dev_file_anchor_first(vlr_dev_file*, int, int, uint64_t*) DEVICE(vlr_dev_file_anchor_first)
const uint64_t* vlr_dev_file_starts(const vlr_dev_file*, int64_t*) DEVICE(vlr_dev_file_starts)
int vlr_dev_file_decode(vlr_dev_file*, int64_t, const uint32_t*, int, int, const vlr::DeviceCols*) DEVICE(vlr_dev_file_decode)
int vlr_dev_file_cold(vlr_dev_file*, int64_t, const uint64_t*, uint8_t*) DEVICE(vlr_dev_file_cold)
int vlr_dev_file_consume(vlr_dev_file*, int64_t) DEVICE(vlr_dev_file_consume)
int vlr_dev_file_sync(vlr_dev_file*) DEVICE(vlr_dev_file_sync)
int vlr_dev_file_errors(vlr_dev_file*, int64_t, uint32_t*, int64_t*) DEVICE(vlr_dev_file_errors)
int vlr_dev_file_copy(vlr_dev_file*, void*, const void*, size_t, int) DEVICE(vlr_dev_file_copy)
int vlr_dev_file_summaries(vlr_dev_file*, const vlr::DeviceCols*, const uint32_t*, const uint8_t*, int64_t, int, uint32_t, const vlr::SumConsts*, vlr::PileSum*, uint8_t*,
                           uint32_t, float*, uint32_t*, uint64_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*) DEVICE(vlr_dev_file_summaries)
int vlr_dev_copy_to_host(int, void*, const void*, size_t) DEVICE(vlr_dev_copy_to_host)
int vlr_dev_file_copy_detached(vlr_dev_file*, void*, const void*, size_t, void**) DEVICE(vlr_dev_file_copy_detached)
int vlr_dev_file_copy_more(vlr_dev_file*, void*, const void*, size_t) DEVICE(vlr_dev_file_copy_more)
int vlr_dev_file_copy_mark(vlr_dev_file*, void**) DEVICE(vlr_dev_file_copy_mark)
int vlr_dev_file_wait_mark(vlr_dev_file*, void*) DEVICE(vlr_dev_file_wait_mark)
int vlr_dev_event_wait(int, void*) DEVICE(vlr_dev_event_wait)
void vlr_dev_event_destroy(int, void*) DEVICE(vlr_dev_event_destroy)
int vlr_dev_slab_alloc(int, size_t, void**, void**) DEVICE(vlr_dev_slab_alloc)
void vlr_dev_slab_free(int, void*, void*) DEVICE(vlr_dev_slab_free)
int vlr_node_n_devices(const vlr_gpu_node*) DEVICE(vlr_node_n_devices)
int vlr_node_device(const vlr_gpu_node*, int) DEVICE(vlr_node_device)
int vlr_fdr_threshold(int, const double*, int64_t, int, double, double*, int*) DEVICE(vlr_fdr_threshold)
int vlr_posterior_odds_keep(int, int64_t, const double*, const double*, const uint8_t*, int, uint8_t*) DEVICE(vlr_posterior_odds_keep)
int vlr_launch_range_group_lse(int, int64_t, const double*, const double*, const int32_t*, int, const double*, const double*, int, int64_t, double*)
    DEVICE(vlr_launch_range_group_lse)
}

namespace {

constexpr int kThreads = 2;

int refuse(int rc) {
    printf("error %d: %s\n", rc, g_error.c_str());
    return 2;
}

struct Crc {
    uint32_t v = (uint32_t)crc32(0L, Z_NULL, 0);
    void add(const void* p, size_t n) {
        const uint8_t* q = (const uint8_t*)p;
        while (n) { const size_t k = n < (1u << 30) ? n : (1u << 30); v = (uint32_t)crc32(v, q, (uInt)k); q += k; n -= k; }
    }
};

// ------------------------------------------------------------------------------------------------ obs
constexpr int kTableArrays = 22;
struct TableDigest {
    int64_t n_loci = 0, n_obs = 0;
    Crc a[kTableArrays];
    int add(const vlr_obs_table* t) {
        vlr_batch b;
        vlr_obs_sites s;
        if (int rc = vlr_obs_table_batch(t, &b)) return rc;
        if (int rc = vlr_obs_table_sites(t, &s)) return rc;
        const size_t L = (size_t)b.n_loci, P = L * (size_t)b.n_samples, N = (size_t)b.n_obs;
        n_loci += b.n_loci; n_obs += b.n_obs;
        for (size_t p = 0; p < P; ++p) { const uint32_t n = b.obs_offset[p + 1] - b.obs_offset[p]; a[0].add(&n, 4); }
        const float* col[9] = {b.prob_mapping, b.prob_alt, b.prob_ref, b.prob_missed_allele, b.prob_sample_alt, b.prob_double_overlap, b.prob_hit_base,
                               b.prob_hp_artifact, b.prob_hp_variant};
        for (int k = 0; k < 9; ++k) a[1 + k].add(col[k], N * 4);
        a[10].add(b.flags, N * 4);
        a[11].add(s.third_allele_evidence, N * 4);
        a[12].add(b.locus_flags, L); a[13].add(b.variant_type, L); a[14].add(b.ref_base, L); a[15].add(b.alt_base, L);
        a[16].add(s.pos, L * 8);
        a[17].add(s.heterozygosity_ln, L * 8); a[18].add(s.somatic_effective_mutation_rate_ln, L * 8);
        a[19].add(s.imprecise, L);
        a[20].add(s.group_key, L * 8);
        for (size_t l = 0; l < L; ++l) {
            const int32_t c = s.contig[l];
            const std::string chrom = (c >= 0 && c < s.n_contigs) ? std::string(s.contig_names[c]) : std::to_string(c);
            a[21].add(chrom.c_str(), chrom.size() + 1);
            for (const uint64_t* off : {s.id_offset, s.ref_offset, s.alt_offset}) { const char* q = s.strings + off[l]; a[21].add(q, strlen(q) + 1); }
        }
        return VLR_OK;
    }
    void print(const char* pass) const {
        Crc all;
        for (int k = 0; k < kTableArrays; ++k) { const uint8_t w[4] = {(uint8_t)a[k].v, (uint8_t)(a[k].v >> 8), (uint8_t)(a[k].v >> 16), (uint8_t)(a[k].v >> 24)}; all.add(w, 4); }
        printf("%s n_loci=%lld n_obs=%lld checksum=%08x\n", pass, (long long)n_loci, (long long)n_obs, all.v);
    }
};

int run_obs(const char* path) {
    {
        vlr_obs_table* t = nullptr;
        if (int rc = vlr_obs_read(1, &path, 0, kThreads, &t)) return refuse(rc);
        TableDigest d;
        const int rc = d.add(t);
        vlr_obs_table_free(t);
        if (rc) return refuse(rc);
        d.print("whole");
    }
    for (const int64_t chunk : {(int64_t)1, (int64_t)7}) {
        vlr_obs_reader* r = nullptr;
        if (int rc = vlr_obs_reader_open(1, &path, 0, kThreads, &r)) return refuse(rc);
        TableDigest d;
        for (;;) {
            vlr_obs_table* t = nullptr;
            int rc = vlr_obs_reader_next(r, chunk, &t);
            if (rc == VLR_OK && !t) break;
            if (rc == VLR_OK) { rc = d.add(t); vlr_obs_table_free(t); }
            if (rc) { vlr_obs_reader_close(r); return refuse(rc); }
        }
        vlr_obs_reader_close(r);
        d.print(chunk == 1 ? "stream1" : "stream7");
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ calls
int run_calls(const char* path) {
    for (const bool with_ann_af : {false, true}) {
        CallsFile cf;
        if (int rc = open_calls(path, kThreads, cf)) return refuse(rc);
        std::vector<std::string> tag_names;   // every PROB_* entry of the header's dictionary
        std::vector<int> tags;
        for (const std::string& id : cf.h.dict)
            if (id.compare(0, 5, "PROB_") == 0) { tags.push_back((int)tag_names.size()); tag_names.push_back(id); }
        if (int rc = read_call_records(path, cf, tag_names, with_ann_af)) return refuse(rc);
        Crc c;
        int64_t n_variants = 0, n_sums = 0, n_ann = 0, n_af = 0;
        std::vector<VarType> types;
        std::vector<double> sums;
        const TypeFilter all;
        for (const CallRec& r : cf.recs) {
            c.add(r.raw, r.raw_len);
            c.add(&r.pos0, 8);
            c.add(r.ref.c_str(), r.ref.size() + 1);
            for (auto& a : r.alts) c.add(a.c_str(), a.size() + 1);
            c.add(r.event.c_str(), r.event.size() + 1);
            c.add(r.svtype.c_str(), r.svtype.size() + 1);
            c.add(r.svlen.data(), r.svlen.size() * 8);
            if (r.has_end) c.add(&r.end0, 8);
            for (auto& v : r.prob) c.add(v.data(), v.size() * 8);
            std::string err;
            if (!variant_types(r, types, err)) { g_error = err; return refuse(VLR_ERR_INVALID_ARGUMENT); }
            for (auto& v : types) { c.add(&v.kind, 4); c.add(&v.len, 8); n_variants += v.kind >= 0; }
            tags_prob_sum(r, types, tags, all, sums);
            c.add(sums.data(), sums.size() * 8);
            n_sums += (int64_t)sums.size();
            n_ann += r.has_ann;
            if (r.has_af) for (auto& v : r.af) n_af += (int64_t)v.size();
        }
        printf("%s n_records=%lld n_variants=%lld n_sums=%lld checksum=%08x", with_ann_af ? "ann_af" : "plain", (long long)cf.recs.size(), (long long)n_variants,
               (long long)n_sums, c.v);
        if (with_ann_af) printf(" n_ann=%lld n_af=%lld", (long long)n_ann, (long long)n_af);
        printf("\n");
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const bool obs = argc >= 3 && strcmp(argv[1], "obs") == 0;
    if (argc < 3 || (!obs && strcmp(argv[1], "calls") != 0)) {
        fprintf(stderr, "usage: %s obs|calls <file>... | obs|calls <file> ff <begin> <end>\n", argv[0]);
        return 1;
    }
    int worst = 0;
    auto one = [&](const char* path) {
        const int rc = obs ? run_obs(path) : run_calls(path);
        printf("=%d\n", rc);
        fflush(stdout);
        worst = rc > worst ? rc : worst;
    };
    if (argc == 6 && strcmp(argv[3], "ff") == 0) {
        const long begin = atol(argv[4]), end = atol(argv[5]);
        const int fd = open(argv[2], O_RDWR);
        if (fd < 0 || begin < 0 || end < begin) { fprintf(stderr, "cannot damage %s\n", argv[2]); return 1; }
        for (long o = begin; o < end; ++o) {
            uint8_t was = 0;
            const uint8_t ff = 0xff;
            if (pread(fd, &was, 1, (off_t)o) != 1 || pwrite(fd, &ff, 1, (off_t)o) != 1) { fprintf(stderr, "cannot damage %s at %ld\n", argv[2], o); return 1; }
            printf("@%ld\n", o);
            one(argv[2]);
            if (pwrite(fd, &was, 1, (off_t)o) != 1) return 1;
        }
        close(fd);
        return worst;
    }
    for (int i = 2; i < argc; ++i) {
        printf("@%s\n", argv[i]);
        one(argv[i]);
    }
    return worst;
}
