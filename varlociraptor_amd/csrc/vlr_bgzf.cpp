// vlr_bgzf.cpp — threads, mapped files and BGZF in both directions for the host units of the front door (vlr_hostio.h).
// No htslib: BGZF members are located through their BSIZE fields and inflated in parallel (libdeflate when the system has it, else
// zlib); output members are deflated in parallel and, for the streaming calls writer, handed to one I/O thread.  Pure host code.
#include <dlfcn.h>
#include <sched.h>
#include <zlib.h>

#include <cstdarg>

#include "vlr_hostio.h"

namespace vlr_hostio VLR_HIDDEN {

int ifail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    vlr_set_error(buf);
    return code;
}

}  // namespace vlr_hostio

using namespace vlr_hostio;

namespace {
// ------------------------------------------------------------------------------------------------ threads
// CPUs this process may actually use: the affinity mask and the cgroup CPU quota (containers report the host's hardware threads)
int effective_cpus() {
    unsigned h = std::thread::hardware_concurrency();
    int n = (int)(h ? h : 1u);
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::min(n, std::max(1, CPU_COUNT(&set)));
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota> <period>" or "max <period>"
        char q[64];
        long period = 0;
        if (fscanf(f, "%63s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) n = std::min(n, (int)std::max(1L, (atol(q) + period - 1) / period));
        fclose(f);
    } else {
        long quota = -1, period = 0;
        if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%ld", &quota) != 1) quota = -1; fclose(g); }
        if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%ld", &period) != 1) period = 0; fclose(g); }
        if (quota > 0 && period > 0) n = std::min(n, (int)std::max(1L, (quota + period - 1) / period));
    }
    return std::max(1, n);
}
}  // namespace

namespace vlr_hostio VLR_HIDDEN {

int pick_threads(int n) {
    if (n > 0) return n;
    if (const char* ev = getenv("VLR_INGEST_THREADS")) { const int v = atoi(ev); if (v > 0) return v; }
    static const int eff = effective_cpus();
    return std::max(1, std::min(eff, 256));
}

// ------------------------------------------------------------------------------------------------ files, BGZF
bool read_whole_file(const char* path, Blob& out, std::string& err) {
    if (out.map_file(path)) return true;
    FILE* f = fopen(path, "rb");
    if (!f) { err = std::string("cannot open ") + path; return false; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (!out.alloc((size_t)std::max(0L, n))) { fclose(f); err = "out of memory"; return false; }
    const size_t got = n > 0 ? fread(out.p, 1, (size_t)n, f) : 0;
    fclose(f);
    if (got != (size_t)std::max(0L, n)) { err = std::string("short read on ") + path; return false; }
    return true;
}

// all gzip members carry the BGZF extra field `BC` with their total size: index them without inflating
bool bgzf_index(const Blob& raw, std::vector<BgzfBlock>& blocks) {
    size_t p = 0;
    size_t total = 0;
    while (p < raw.size()) {
        if (p + 18 > raw.size() || raw[p] != 0x1f || raw[p + 1] != 0x8b || raw[p + 2] != 8 || !(raw[p + 3] & 4)) return false;
        const unsigned xlen = raw[p + 10] | (raw[p + 11] << 8);
        size_t q = p + 12;
        const size_t xend = q + xlen;
        if (xend > raw.size()) return false;
        long bsize = -1;
        while (q + 4 <= xend) {
            const unsigned slen = raw[q + 2] | (raw[q + 3] << 8);
            if (raw[q] == 'B' && raw[q + 1] == 'C' && slen == 2 && q + 6 <= xend) bsize = (raw[q + 4] | (raw[q + 5] << 8)) + 1;
            q += 4 + slen;
        }
        if (bsize < 0 || p + (size_t)bsize > raw.size() || (size_t)bsize < xlen + 20) return false;
        const size_t cdata = xend, cend = p + (size_t)bsize - 8;
        const uint32_t isize = raw[cend + 4] | (raw[cend + 5] << 8) | (raw[cend + 6] << 16) | ((uint32_t)raw[cend + 7] << 24);
        const uint32_t crc = raw[cend] | (raw[cend + 1] << 8) | (raw[cend + 2] << 16) | ((uint32_t)raw[cend + 3] << 24);
        blocks.push_back({cdata, cend - cdata, isize, total, crc});
        total += isize;
        p += (size_t)bsize;
    }
    return true;
}

}  // namespace vlr_hostio

namespace {
// libdeflate (a system library next to zlib, about twice zlib's inflate rate) is taken through dlopen when it is installed — the
// image carries the runtime library without its header; its C API (v1.x) is declared here.  zlib is the fallback.
struct LibDeflate {
    void* (*alloc_d)() = nullptr;
    int (*decompress)(void*, const void*, size_t, void*, size_t, size_t*) = nullptr;
    void (*free_d)(void*) = nullptr;
    void* (*alloc_c)(int) = nullptr;
    size_t (*compress)(void*, const void*, size_t, void*, size_t) = nullptr;
    size_t (*bound)(void*, size_t) = nullptr;
    void (*free_c)(void*) = nullptr;
    uint32_t (*crc32)(uint32_t, const void*, size_t) = nullptr;
    bool ok = false;
    LibDeflate() {
        if (getenv("VLR_NO_LIBDEFLATE")) return;
        void* h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        alloc_d = (void* (*)())dlsym(h, "libdeflate_alloc_decompressor");
        decompress = (int (*)(void*, const void*, size_t, void*, size_t, size_t*))dlsym(h, "libdeflate_deflate_decompress");
        free_d = (void (*)(void*))dlsym(h, "libdeflate_free_decompressor");
        alloc_c = (void* (*)(int))dlsym(h, "libdeflate_alloc_compressor");
        compress = (size_t (*)(void*, const void*, size_t, void*, size_t))dlsym(h, "libdeflate_deflate_compress");
        bound = (size_t (*)(void*, size_t))dlsym(h, "libdeflate_deflate_compress_bound");
        free_c = (void (*)(void*))dlsym(h, "libdeflate_free_compressor");
        crc32 = (uint32_t (*)(uint32_t, const void*, size_t))dlsym(h, "libdeflate_crc32");
        ok = alloc_d && decompress && free_d && alloc_c && compress && bound && free_c && crc32;
    }
};
const LibDeflate& libdeflate() { static LibDeflate L; return L; }
// a worker's libdeflate objects: one per thread, given back when the thread ends (the pools start new threads for every call)
struct ThreadDecompressor {
    void* d = libdeflate().alloc_d();
    ~ThreadDecompressor() { if (d) libdeflate().free_d(d); }
};
struct ThreadCompressor {
    void* c = nullptr;
    int level = -1;
    void* at(int lv) {
        if (level != lv) { if (c) libdeflate().free_c(c); c = libdeflate().alloc_c(lv); level = lv; }
        return c;
    }
    ~ThreadCompressor() { if (c) libdeflate().free_c(c); }
};

// CRC32 of an inflated member against the value in its trailer (RFC 1952; htslib's bgzf.c checks it for every block it reads)
bool member_crc_ok(const uint8_t* data, size_t n, uint32_t want) {
    const LibDeflate& ld = libdeflate();
    const uint32_t got = ld.ok ? ld.crc32(0, data, n) : (uint32_t)crc32(crc32(0L, Z_NULL, 0), data, (uInt)n);
    return got == want;
}
}  // namespace

namespace vlr_hostio VLR_HIDDEN {

// one BGZF member: raw DEFLATE -> dlen bytes whose CRC32 is `crc`
bool inflate_raw(const uint8_t* src, size_t clen, uint8_t* dst, size_t dlen, uint32_t crc) {
    const LibDeflate& ld = libdeflate();
    if (ld.ok) {
        thread_local ThreadDecompressor dec;
        void* const d = dec.d;
        size_t got = 0;
        if (d && ld.decompress(d, src, clen, dst, dlen, &got) == 0 && got == dlen) return member_crc_ok(dst, dlen, crc);
        // fall through to zlib on any doubt
    }
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<Bytef*>(src); zs.avail_in = (uInt)clen;
    zs.next_out = dst; zs.avail_out = (uInt)dlen;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = (rc == Z_STREAM_END) && zs.total_out == dlen;
    inflateEnd(&zs);
    return ok && member_crc_ok(dst, dlen, crc);
}

// file contents, decompressed: BGZF (parallel), plain gzip (sequential), or as is
bool load_inflated(const char* path, Blob& out_blob, int n_threads, std::string& err) {
    Blob raw;
    const double t0 = now_s();
    if (!read_whole_file(path, raw, err)) return false;
    g_ingest_t[0] += now_s() - t0;
    std::vector<uint8_t> out;
    auto finish = [&](std::vector<uint8_t>& v) { if (!out_blob.alloc(v.size())) { err = "out of memory"; return false; } memcpy(out_blob.p, v.data(), v.size()); return true; };
    if (raw.size() < 2 || raw[0] != 0x1f || raw[1] != 0x8b) { std::swap(out_blob.p, raw.p); std::swap(out_blob.n, raw.n); std::swap(out_blob.mapped, raw.mapped); return true; }
    std::vector<BgzfBlock> blocks;
    if (bgzf_index(raw, blocks)) {
        size_t total = 0;
        for (auto& b : blocks) total += b.isize;
        if (!out_blob.alloc(total)) { err = "out of memory"; return false; }
        std::atomic<bool> bad{false};
        const double t1 = now_s();
        parallel_items((int64_t)blocks.size(), n_threads, [&](int64_t i, int) {
            const BgzfBlock& b = blocks[(size_t)i];
            if (b.isize == 0) return;
            if (!inflate_raw(raw.data() + b.off, b.clen, out_blob.p + b.out_off, b.isize, b.crc)) bad = true;
        });
        g_ingest_t[1] += now_s() - t1;
        if (bad) { err = std::string("corrupt BGZF block in ") + path; return false; }
        return true;
    }
    // generic (multi-member) gzip
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, 15 + 32) != Z_OK) { err = "zlib init failed"; return false; }
    zs.next_in = raw.p; zs.avail_in = 0;
    const uint8_t* const raw_end = raw.p + raw.size();
    out.resize(std::max<size_t>(raw.size() * 4, 1 << 16));
    size_t have = 0;
    for (;;) {
        if (have == out.size()) out.resize(out.size() * 2);
        // zlib counts in 32 bits: hand the input over in pieces (a plain-gzip file above 2 GiB used to end at the first piece)
        if (zs.avail_in == 0 && zs.next_in < raw_end) zs.avail_in = (uInt)std::min<size_t>((size_t)(raw_end - zs.next_in), 0x40000000);
        zs.next_out = out.data() + have; zs.avail_out = (uInt)std::min<size_t>(out.size() - have, 0x7fffffff);
        const int rc = inflate(&zs, Z_NO_FLUSH);
        have = (size_t)(zs.next_out - out.data());
        if (rc == Z_STREAM_END) {
            if (zs.avail_in == 0 && zs.next_in >= raw_end) break;
            if (inflateReset(&zs) != Z_OK) { inflateEnd(&zs); err = "zlib reset failed"; return false; }
            continue;
        }
        if (rc != Z_OK) { inflateEnd(&zs); err = std::string("corrupt gzip stream in ") + path; return false; }
    }
    inflateEnd(&zs);
    out.resize(have);
    return finish(out);
}

}  // namespace vlr_hostio

namespace {
// one BGZF member holding `n` bytes (n <= 0xff00)
void bgzf_deflate_block(const uint8_t* data, size_t n, int level, std::vector<uint8_t>& out) {
    uLong bound = compressBound((uLong)n) + 64;
    const size_t at = out.size();
    size_t clen = 0;
    const LibDeflate& ld = libdeflate();
    if (ld.ok) {
        thread_local ThreadCompressor comp;
        void* const c = comp.at(level);
        if (c) {
            bound = (uLong)ld.bound(c, n) + 64;
            out.resize(at + 18 + bound + 8);
            clen = ld.compress(c, data, n, out.data() + at + 18, bound);
        }
    }
    if (clen == 0 || clen + 26 > 0xffff) {
        bound = compressBound((uLong)n) + 64;
        out.resize(at + 18 + bound + 8);
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
        zs.next_in = const_cast<Bytef*>(data); zs.avail_in = (uInt)n;
        zs.next_out = out.data() + at + 18; zs.avail_out = (uInt)bound;
        deflate(&zs, Z_FINISH);
        clen = zs.total_out;
        deflateEnd(&zs);
    }
    static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    memcpy(out.data() + at, head, 16);
    const unsigned bsize = (unsigned)(clen + 25);
    out[at + 16] = (uint8_t)(bsize & 0xff); out[at + 17] = (uint8_t)(bsize >> 8);
    const uint32_t crc = ld.ok ? ld.crc32(0, data, n) : (uint32_t)crc32(crc32(0L, Z_NULL, 0), data, (uInt)n), isz = (uint32_t)n;
    uint8_t* t = out.data() + at + 18 + clen;
    for (int i = 0; i < 4; ++i) { t[i] = (uint8_t)(crc >> (8 * i)); t[4 + i] = (uint8_t)(isz >> (8 * i)); }
    out.resize(at + 18 + clen + 8);
}
}  // namespace

namespace vlr_hostio VLR_HIDDEN {

const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

bool write_bgzf_file(const char* path, const std::vector<const std::vector<uint8_t>*>& parts, int n_threads, int level, std::string& err) {
    FILE* f = fopen(path, "wb");
    if (!f) { err = std::string("cannot create ") + path; return false; }
    bool ok = write_bgzf_stream(f, parts, n_threads, level, true, err);
    ok = (fclose(f) == 0) && ok;
    if (!ok && err.empty()) err = std::string("write failed on ") + path;
    return ok;
}
// the parts, logically concatenated, as BGZF members appended to an open file (a short last member is legal BGZF)
bool write_bgzf_stream(FILE* f, const std::vector<const std::vector<uint8_t>*>& parts, int n_threads, int level, bool with_eof, std::string& err, AsyncSink* sink) {
    // the parts are logically concatenated; cut into blocks without copying more than one block at a time
    size_t total = 0;
    std::vector<size_t> start;
    for (auto* p : parts) { start.push_back(total); total += p->size(); }
    const size_t B = 0xff00;
    const int64_t nb = (int64_t)((total + B - 1) / B);
    std::vector<std::vector<uint8_t>> comp((size_t)nb);
    parallel_items(nb, n_threads, [&](int64_t bi, int) {
        const size_t b0 = (size_t)bi * B, b1 = std::min(total, b0 + B);
        std::vector<uint8_t> tmp;
        tmp.reserve(b1 - b0);
        size_t k = (size_t)(std::upper_bound(start.begin(), start.end(), b0) - start.begin()) - 1;
        size_t pos = b0;
        while (pos < b1) {
            const std::vector<uint8_t>& P = *parts[k];
            const size_t o = pos - start[k], n = std::min(P.size() - o, b1 - pos);
            tmp.insert(tmp.end(), P.begin() + (long)o, P.begin() + (long)(o + n));
            pos += n;
            ++k;
        }
        bgzf_deflate_block(tmp.data(), tmp.size(), level, comp[(size_t)bi]);
    });
    if (sink) {   // (the streaming writer: the end-of-file member is written by its close, after the sink has drained)
        sink->push(std::move(comp));
        return true;
    }
    bool ok = true;
    for (auto& c : comp) ok = ok && fwrite(c.data(), 1, c.size(), f) == c.size();
    if (with_eof) ok = ok && fwrite(kBgzfEof, 1, 28, f) == 28;
    if (!ok) err = "write failed";
    return ok;
}
}  // namespace vlr_hostio
