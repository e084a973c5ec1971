// vlr_bamstream.h — one BAM file through the device reader (vlr_bamstats.hip: stream_bam) and the reference's contigs through its .fai,
// shared by the passes that consume split BAM records on the device: vlr_bamstats_add_bam, vlr_basepileup_add_bam,
// vlr_indelpileup_add_bam and vlr_fragpileup_add_bam (the three sessions through vlr_bamsession.h).  Internal to the engine's
// translation units.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

struct vlr_dev_file;

namespace vlr_bam {

struct BamStream {
    int device = 0;
    size_t* window = nullptr;   // inflated bytes per split; grown for a record longer than it
    // seconds, accumulated: file read, upload + inflate of the feeds, record split, inflate kernels alone, total; splits that fell back to the serial walk
    double *t_read = nullptr, *t_feed = nullptr, *t_split = nullptr, *t_inflate = nullptr, *t_total = nullptr, *n_serial = nullptr;
    std::function<bool()> done;                                              // true: the caller needs no more records (may be empty)
    std::function<int(const std::vector<std::string>& names)> on_header;     // once per file, the contig names of its header
    // n split records of the file, the first one its record number rec0; view them with vlr_dev_file_split_view
    std::function<int(vlr_dev_file* df, int64_t n, uint64_t rec0, const std::vector<std::string>& names, const char* path, void* stream)> on_chunk;
    // the file ends inside record rec0: empty = an error naming the record; else the callback's return value ends the file
    std::function<int(uint64_t rec0)> on_truncated;
};

int stream_bam(const BamStream& b, const char* path);
int bfail(int code, const char* fmt, ...);
double now_s();

// the reference FASTA through its .fai index: the entries by contig name, and the contigs uploaded so far (device pointer, length)
struct FaiEntry { uint64_t len, off, lb, lw; };
using Fai = std::map<std::string, FaiEntry>;
using Contigs = std::map<std::string, std::pair<uint8_t*, uint64_t>>;

int read_fai(const std::string& fasta, Fai& fai);
// the bases of one contig on the device, once per name; case preserved (bio's IndexedReader) or upper-cased (the reference's buffer
// for realignment hands out upper case).  `bam` names the file whose header asked for it, for the refusal.
int load_contig(const std::string& fasta, const Fai& fai, Contigs& cache, const std::string& name, const char* bam, bool upper_case, std::pair<uint8_t*, uint64_t>& out);

}  // namespace vlr_bam
