// vlr_hostio.h — what the host units of the front door share: vlr_bgzf.cpp (threads, mapped files, BGZF in and out), vlr_callsfile.cpp
// (calls-file reader and its consumers) and vlr_ingest.cpp (VCF header, observation readers, device reader, writers).  Internal and
// plain host C++: no .hip file includes it, and vlr_ingest_host.cpp links the units against it without the HIP library.
//
// Everything that crosses a unit lives in namespace vlr_hostio, which has hidden visibility: libvlr.so exports what include/vlr.h
// declares.  What is called per value or per record — BCF2 typed values, the record framer, the walk over a record's shared block,
// the float sentinels, parallel_* — is inline here; what is declared here and defined in a unit is called per file, per BGZF member
// or per chunk of records.
//
// The BCF2 container is stated here once: bcf_head (magic, l_text, header text), bcf_frame (l_shared / l_indiv), bcf_walk_shared
// (fixed head, ID, alleles, FILTER, INFO pairs), kBcfFloatMissing / kBcfFloatEndOfVector.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/vlr.h"
#include "vlr_gpuio.h"
#include "vlr_callstats.h"

extern "C" void vlr_set_error(const char* msg);  // vlr_host.cpp: the text behind vlr_last_error()

#define VLR_HIDDEN __attribute__((visibility("hidden")))

namespace vlr_hostio VLR_HIDDEN {

// stage timings of the last vlr_obs_read / vlr_calls_write of this process (vlr_ingest_last_timings) and the same stages summed over
// every call since the last reset (streaming reader / writer): measurement aid, defined in vlr_ingest.cpp
extern double g_ingest_t[16];
extern double g_ingest_total[16];
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int ifail(int code, const char* fmt, ...);   // sets the error text, returns code

// ------------------------------------------------------------------------------------------------ threads (vlr_bgzf.cpp)
int pick_threads(int n);   // n > 0, else VLR_INGEST_THREADS, else the CPUs this process may use
// fn(begin, end, worker) over [0, n) in contiguous ranges
template <typename F>
void parallel_ranges(int64_t n, int n_threads, F&& fn) {
    if (n <= 0) return;
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, n));
    if (T == 1) { fn((int64_t)0, n, 0); return; }
    std::vector<std::thread> th;
    th.reserve(T);
    for (int t = 0; t < T; ++t) {
        const int64_t b = n * t / T, e = n * (t + 1) / T;
        th.emplace_back([&fn, b, e, t] { fn(b, e, t); });
    }
    for (auto& x : th) x.join();
}
// dynamic work items (blocks of very different cost)
template <typename F>
void parallel_items(int64_t n, int n_threads, F&& fn) {
    if (n <= 0) return;
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, n));
    std::atomic<int64_t> next{0};
    auto body = [&](int t) {
        for (;;) {
            const int64_t i = next.fetch_add(1);
            if (i >= n) break;
            fn(i, t);
        }
    };
    if (T == 1) { body(0); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back(body, t);
    for (auto& x : th) x.join();
}

// ------------------------------------------------------------------------------------------------ files, BGZF (vlr_bgzf.cpp)
// an uninitialised byte buffer (std::vector would zero gigabytes on one thread before the workers overwrite them)
struct Blob {
    uint8_t* p = nullptr;
    size_t n = 0;
    Blob() = default;
    Blob(const Blob&) = delete;
    Blob& operator=(const Blob&) = delete;
    bool mapped = false;
    // (unmapping a file of gigabytes walks all its touched pages — 65 ms for the 2 GB of a million-record run: off the caller's thread)
    void release() {
        if (p) {
            if (mapped && n >= ((size_t)64 << 20)) { uint8_t* q = p; const size_t m = n; std::thread([q, m] { munmap(q, m); }).detach(); }
            else if (mapped) munmap(p, n ? n : 1);
            else free(p);
        }
        p = nullptr; n = 0; mapped = false;
    }
    ~Blob() { release(); }
    bool alloc(size_t bytes) {
        release();
        if (bytes >= ((size_t)8 << 20)) {  // gigabytes touched for the first time by all workers at once: 2 MB pages, 512 x fewer faults
            void* q = nullptr;
            if (posix_memalign(&q, (size_t)2 << 20, (bytes + (((size_t)2 << 20) - 1)) & ~(((size_t)2 << 20) - 1)) == 0) {
                (void)madvise(q, bytes, MADV_HUGEPAGE);
                p = (uint8_t*)q; n = bytes;
                return true;
            }
        }
        p = (uint8_t*)malloc(bytes ? bytes : 1); n = p ? bytes : 0; return p != nullptr;
    }
    // the file's pages straight from the page cache (no copy; the inflate workers fault them in side by side)
    bool map_file(const char* path) {
        release();
        const int fd = open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0 || st.st_size <= 0) { close(fd); return false; }
        void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (m == MAP_FAILED) return false;
        (void)madvise(m, (size_t)st.st_size, MADV_WILLNEED);
        p = (uint8_t*)m; n = (size_t)st.st_size; mapped = true;
        return true;
    }
    const uint8_t* data() const { return p; }
    size_t size() const { return n; }
    uint8_t operator[](size_t i) const { return p[i]; }
};

bool read_whole_file(const char* path, Blob& out, std::string& err);

struct BgzfBlock { size_t off, clen; uint32_t isize; size_t out_off; uint32_t crc; };   // crc: CRC32 of the inflated bytes (member trailer)

// all gzip members carry the BGZF extra field `BC` with their total size: index them without inflating
bool bgzf_index(const Blob& raw, std::vector<BgzfBlock>& blocks);
// one BGZF member: raw DEFLATE -> dlen bytes whose CRC32 is `crc`
bool inflate_raw(const uint8_t* src, size_t clen, uint8_t* dst, size_t dlen, uint32_t crc);
// file contents, decompressed: BGZF (parallel), plain gzip (sequential), or as is
bool load_inflated(const char* path, Blob& out_blob, int n_threads, std::string& err);

extern const uint8_t kBgzfEof[28];   // the empty member that ends a BGZF file

// File output behind the streaming calls writer: the compressed members of a chunk are handed to one I/O thread, so that copying
// them into the page cache (tens of milliseconds per hundred megabytes, serial) runs beside the encoding of the next chunk.
struct AsyncSink {
    FILE* f = nullptr;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::vector<std::vector<uint8_t>>> q;
    bool closing = false, failed = false;
    explicit AsyncSink(FILE* file) : f(file) {
        th = std::thread([this] {
            for (;;) {
                std::vector<std::vector<uint8_t>> job;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [this] { return closing || !q.empty(); });
                    if (q.empty()) return;
                    job = std::move(q.front());
                    q.pop_front();
                }
                bool ok = true;
                for (auto& c : job) ok = ok && fwrite(c.data(), 1, c.size(), f) == c.size();
                if (!ok) { std::lock_guard<std::mutex> g(mu); failed = true; }
                cv.notify_all();
            }
        });
    }
    void push(std::vector<std::vector<uint8_t>>&& job) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this] { return q.size() < 3; });   // (bounded: at most three chunks of compressed members in memory)
        q.push_back(std::move(job));
        cv.notify_all();
    }
    bool finish() {   // everything handed over is in the file (or failed)
        { std::lock_guard<std::mutex> g(mu); closing = true; }
        cv.notify_all();
        if (th.joinable()) th.join();
        return !failed;
    }
    ~AsyncSink() { (void)finish(); }
};
// compress the parts, logically concatenated, into BGZF members of 0xff00 bytes in parallel and write the file / append them to an
// open file (a short last member is legal BGZF)
bool write_bgzf_file(const char* path, const std::vector<const std::vector<uint8_t>*>& parts, int n_threads, int level, std::string& err);
bool write_bgzf_stream(FILE* f, const std::vector<const std::vector<uint8_t>*>& parts, int n_threads, int level, bool with_eof, std::string& err, AsyncSink* sink = nullptr);

// ------------------------------------------------------------------------------------------------ VCF header (vlr_ingest.cpp)
struct Header {
    std::string text;
    std::vector<std::string> dict;     // FILTER/INFO/FORMAT ids by dictionary index
    std::vector<std::string> contigs;  // by index
    bool version_ok = false;
};
std::string attr(const std::string& body, const char* key);   // value of key= in the <...> body of a header line
void parse_header(const std::string& text, Header& h);

// ------------------------------------------------------------------------------------------------ the BCF2 container
// Float values: "missing" and "end of vector" are two signalling-NaN bit patterns (VCF 4.3 section 6.3.3), read and written as bits.
constexpr uint32_t kBcfFloatMissing = 0x7F800001u, kBcfFloatEndOfVector = 0x7F800002u;
inline bool bcf_float_missing(uint32_t bits) { return bits == kBcfFloatMissing; }
inline bool bcf_float_end_of_vector(uint32_t bits) { return bits == kBcfFloatEndOfVector; }

// The first n bytes of an inflated stream as the head of a BCF2 file: "BCF\2\2", l_text, the header text.
//   BCF_SHORT    fewer than the nine bytes of magic and l_text: cannot tell
//   BCF_NOT      another magic
//   BCF_PARTIAL  BCF2, and the header takes `need` bytes (magic + l_text + text), more than the n given
//   BCF_OK       `need` as above, the text (trailing NULs stripped) parsed into h
// What a short or foreign stream means, and the error text, is the caller's.
enum BcfHead { BCF_SHORT, BCF_NOT, BCF_PARTIAL, BCF_OK };
BcfHead bcf_head(const uint8_t* d, size_t n, size_t& need, Header& h);

// The record that starts at byte p of d[0, n): its end (8 + l_shared + l_indiv behind p), or false when its eight length bytes or
// its body are not all there.
inline bool bcf_frame(const uint8_t* d, size_t n, size_t p, size_t& end, uint32_t* l_shared = nullptr) {
    if (p + 8 > n) return false;
    uint32_t ls, li;
    memcpy(&ls, d + p, 4); memcpy(&li, d + p + 4, 4);
    const size_t e = p + 8 + (size_t)ls + li;
    if (e > n) return false;
    end = e;
    if (l_shared) *l_shared = ls;
    return true;
}

// ---- BCF2 typed values
struct Typed { int type; uint32_t n; const uint8_t* data; };
inline bool bcf_typed(const uint8_t*& p, const uint8_t* e, Typed& t) {
    if (p >= e) return false;
    const uint8_t b = *p++;
    t.type = b & 0xf;
    t.n = b >> 4;
    if (t.n == 15) {
        Typed l;
        if (!bcf_typed(p, e, l) || l.n != 1) return false;
        if (l.type == 1) t.n = (uint32_t)(int8_t)l.data[0];
        else if (l.type == 2) { int16_t v; memcpy(&v, l.data, 2); t.n = (uint32_t)v; }
        else if (l.type == 3) { int32_t v; memcpy(&v, l.data, 4); t.n = (uint32_t)v; }
        else return false;
    }
    static const int size[16] = {0, 1, 2, 4, 0, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0};
    const size_t bytes = (size_t)t.n * size[t.type];
    if ((size_t)(e - p) < bytes) return false;
    t.data = p;
    p += bytes;
    return true;
}
inline int32_t typed_int(const Typed& t, uint32_t i) {
    if (t.type == 1) return (int8_t)t.data[i];
    if (t.type == 2) { int16_t v; memcpy(&v, t.data + 2 * i, 2); return v; }
    int32_t v; memcpy(&v, t.data + 4 * (size_t)i, 4); return v;
}

// The shared block of the record [rec, end): the fixed 24-byte head into `s`, then ID, the alleles and FILTER, then the INFO entries
// as (dictionary key, typed value) pairs — on_id(value), on_allele(index, value), on_info(key, value).  What a caller does with a
// field is its own; so is the text behind each way a record can be malformed.
struct BcfSite { int32_t contig, pos0; uint32_t n_allele, n_info, n_fmt, n_sample; const uint8_t* shared_end; };
enum BcfWalk { BCF_WALK_OK, BCF_WALK_TRUNCATED, BCF_WALK_BAD_ID, BCF_WALK_BAD_ALLELE, BCF_WALK_BAD_FILTER, BCF_WALK_BAD_INFO };
template <typename OnId, typename OnAllele, typename OnInfo>
inline BcfWalk bcf_walk_shared(const uint8_t* rec, const uint8_t* end, BcfSite& s, OnId&& on_id, OnAllele&& on_allele, OnInfo&& on_info) {
    if (end - rec < 32) return BCF_WALK_TRUNCATED;
    uint32_t l_shared;
    memcpy(&l_shared, rec, 4);
    const uint8_t* p = rec + 8;
    if ((size_t)(end - p) < l_shared) return BCF_WALK_TRUNCATED;
    const uint8_t* se = p + l_shared;
    uint32_t nai, nfs;
    memcpy(&s.contig, p, 4); memcpy(&s.pos0, p + 4, 4); memcpy(&nai, p + 16, 4); memcpy(&nfs, p + 20, 4);
    p += 24;   // (a shared block shorter than its fixed head leaves p behind se: the ID below is refused)
    s.n_allele = nai >> 16; s.n_info = nai & 0xffff; s.n_fmt = nfs >> 24; s.n_sample = nfs & 0xffffff;
    s.shared_end = se;
    Typed t;
    if (!bcf_typed(p, se, t)) return BCF_WALK_BAD_ID;
    on_id(t);
    for (uint32_t a = 0; a < s.n_allele; ++a) {
        if (!bcf_typed(p, se, t) || (t.type != 7 && t.n != 0)) return BCF_WALK_BAD_ALLELE;
        on_allele(a, t);
    }
    if (!bcf_typed(p, se, t)) return BCF_WALK_BAD_FILTER;
    for (uint32_t k = 0; k < s.n_info; ++k) {
        Typed key, val;
        if (!bcf_typed(p, se, key) || key.n != 1 || key.type < 1 || key.type > 3 || !bcf_typed(p, se, val)) return BCF_WALK_BAD_INFO;
        on_info(typed_int(key, 0), val);
    }
    return BCF_WALK_OK;
}

// approx::RelativeEq with its default bounds, as the reference compares probabilities (calls writer, control-fdr)
inline bool relative_eq(double a, double b) {
    if (a == b) return true;
    if (std::isinf(a) || std::isinf(b)) return false;  // (approx::RelativeEq: infinities are equal only to themselves)
    const double d = std::fabs(a - b), eps = std::numeric_limits<double>::epsilon();
    return d <= eps || d <= std::max(std::fabs(a), std::fabs(b)) * eps;
}

// ------------------------------------------------------------------------------------------------ calls file (vlr_callsfile.cpp)
// one record of a calls BCF as its consumers read it
struct CallRec {
    const uint8_t* raw = nullptr;
    size_t raw_len = 0;
    int64_t pos0 = 0;
    std::string ref, event, svtype;
    std::vector<std::string> alts;
    bool has_event = false, has_svlen = false, has_end = false;
    std::vector<int64_t> svlen;      // |SVLEN| per entry, -1 = missing
    int64_t end0 = 0;                // END - 1
    std::vector<std::vector<double>> prob;  // per wanted tag: PHRED values per ALT (NaN = missing), empty = tag absent
    // estimate mutational-burden only (read_call_records(.., with_ann_af = true))
    int32_t contig = -1;
    bool has_ann = false, has_af = false;
    std::string ann;                       // INFO/ANN, entries separated by ','
    std::vector<std::vector<float>> af;    // FORMAT/AF per sample of the file (missing value = NaN, end-of-vector trimmed)
};
struct VarType { int kind = -1; int64_t len = 0; };  // kind < 0: skipped by collect_variants
enum { VK_SNV, VK_MNV, VK_INS, VK_DEL, VK_BND, VK_INV, VK_DUP, VK_REP, VK_REF, VK_METH };
struct TypeFilter { int kind = -1; bool has_range = false; int64_t lo = 0, hi = 0; };
// a calls BCF in memory: header, sample names, records (views into `data`)
struct CallsFile {
    Blob data;
    size_t header_bytes = 0;           // magic + l_text + header text: the first record starts behind them
    Header h;
    std::vector<std::string> samples;  // the columns of the #CHROM line behind FORMAT
    std::vector<CallRec> recs;
};
// load the file and parse its header (bcf_head) and the sample names of the #CHROM line; VLR_OK or the error code (text set)
int open_calls(const char* in_path, int n_threads, CallsFile& f);
// the records of an opened calls file: alleles, the float INFO tags `tag_names` (CallRec::prob in that order), EVENT, SVTYPE, SVLEN,
// END; with_ann_af: INFO/ANN and FORMAT/AF as well
int read_call_records(const char* in_path, CallsFile& f, const std::vector<std::string>& tag_names, bool with_ann_af);
// (type, length) per ALT allele as collect_variants types it (collect_variants.rs:44-304)
bool variant_types(const CallRec& r, std::vector<VarType>& out, std::string& err);
// utils/mod.rs:177-212: ln-sum over the given PROB_* tags per (typed) variant; NaN = None
void tags_prob_sum(const CallRec& r, const std::vector<VarType>& types, const std::vector<int>& tags, const TypeFilter& tf, std::vector<double>& out);

}  // namespace vlr_hostio
