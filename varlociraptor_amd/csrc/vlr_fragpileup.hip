// vlr_fragpileup.hip — fragment observations of SNV / MNV candidates from BAM records for gfx950 (vlr_fragpileup_*, include/vlr.h): the
// text of vlr_fragpileup.h over every record of the BAM files streamed through the device reader (vlr_bamstream.h), and the host driver
// of the session.
//
// Member pass, per chunk of split records (one record per thread, as in vlr_basepileup.hip):
//   frag_count_kernel    thread i decodes record i, finds the loci whose window holds its start: cnt[i] = members, and when it is a member
//                        of any locus nbytes[i] = bytes of its QNAME, nxa[i] = alt-locus keys of its XA:Z tag; rejected and bad records go
//                        to integer counters
//   vlr_bam::scan_kernel one workgroup per count array (cnt, nbytes, nxa; vlr_bamsession.h, u32 counts): exclusive prefix sums
//   frag_fill_kernel     thread i builds the members of record i again and writes them at members[base + off[i] ...), its name at
//                        names[name_base + noff[i] ...), its keys at keys[key_base + xoff[i] ...); what would lie behind a capacity is
//                        not written.  It adds the record's members
//                        to the per-locus counters (sums: order-independent)
// so the places of members, names and keys are functions of the record order alone.
// Fragment pass, at vlr_fragpileup_result:
//   vlr_bam::scan_kernel per-locus member counts -> the loci's first slots
//   frag_scatter_kernel  member m takes the next free slot of its locus (an atomic cursor: the placement within a locus is not stable and
//                        need not be, the sort below is on a total key)
//   frag_locus_kernel    one workgroup per locus: the member indices go to LDS, a bitonic sort orders them by (QNAME bytes, record ordinal),
//                        the thread at the first member of each run of equal names forms the fragment's observation (vlr_fp::run_obs), a
//                        prefix sum over the flags of the runs that gave one ranks them in name order, the read positions that count for
//                        major_read_position are sorted in the same LDS array and thread 0 takes their mode; then the indices of the
//                        alt-locus keys of all observations are laid out by a second prefix sum, sorted in that array by (contig hash,
//                        bucket), and thread 0 takes major_alt_locus
//   vlr_bam::scan_kernel per-locus observation counts -> the loci's offsets
//   frag_gather_kernel   one workgroup per locus writes its observations at the offset, in rank order, with VLR_FRAGPILEUP_READPOS_MAJOR
//                        and the alt_locus class (vlr_fp::alt_locus_class)
// No atomic decides a place or an order that reaches the output: the cursors only fill the sort's input.
// A realigning session (vlr_fragpileup_open_realign) adds, per chunk, three more count arrays (evidences, x bytes, y bytes of a record)
// to the same count, scan and fill launches: the fill kernel writes the evidence of every member it flags NEEDS_REALIGN (vlr_fp::
// realign_evidence) at ev[ev_base + eoff[i] ...), the member's index beside it and the session-wide u64 offsets of its two pairs; then
//   indelpileup_gather_kernel  (vlr_pairscore.h, the kernel of the indel session) copies the windows of the chunk's evidences into pair
//                              arrays that accumulate over the session: the records are resident only during their chunk
// and at vlr_fragpileup_result, in front of the fragment pass, once per range of evidences whose pair bytes fit the limit:
//   vlr_ip::score_pairs        edit distance, band, pair HMM (vlr_pairscore.h), indelpileup_collect_kernel the raw scores into the evidences
//   (host)                     vlr_fp::normalize_support over the raw scores
//   frag_apply_kernel          one evidence per thread: vlr_fp::apply_realigned writes the supports into the member and clears the flag
// An evidence's place is a prefix sum over the record order; the ranges only decide which launch scores a pair, not its bytes.
//
// An indel session (vlr_fragpileup_open_indel) is a realigning session whose loci are deletions / insertions with their own alt allele
// windows: the indel kernels of the count and fill bodies (frag_count_indel_kernel, frag_fill_indel_kernel) take the indel arm of vlr_fp::record_members (every member an evidence,
// the overlap bit, a Side record per member at sides[member], first_candidate bounded by the session's longest locus), the fill kernel
// folds the record's CIGAR maxima into its loci (atomic maxima over a total order: order-independent, they decide no place), the gather
// kernel is instantiated with IndelAltWindows, and frag_locus_indel_kernel / frag_gather_indel_kernel apply the validity
// rule of the locus's kind (vlr_fp::make_obs_indel) and carry a vlr_fragpileup_indel_obs beside each observation.  The arrays are
// allocated by such a session alone; the other kernels keep the signatures every session had before (the bodies are shared templates).
//
// A methylation session (vlr_fragpileup_open_methylation; the rule: vlr_methylation.h) has a count and a fill kernel of its own
// (frag_count_meth_kernel, frag_fill_meth_kernel) over vlr_fp::record_members_meth: one record per thread whatever its length, the same
// three count arrays, the same places; nothing of it is compiled into the kernels of the other sessions.  Its members go through the
// fragment pass above unchanged (frag_locus_kernel, frag_gather_kernel): no new LDS, no atomic that decides a place.
//
// LDS of frag_locus_kernel: 4 B index + 2 B rank per member + 2 KiB of scan cells = 26 KiB at VLR_FRAGPILEUP_MAX_MEMBERS = 4096, six
// workgroups per CU by LDS.
// Bounds: a record is read only after vlr_bp::decode checked it; members[k] is written for k < member capacity, names[k] for
// k < name capacity, keys[k] for k < key capacity; perm / tmp / rank / the pair arrays are sized by the member count and every index into
// them is below a locus' count, which sums to it; the output is sized by the scanned observation count; guard bytes behind every one of
// these buffers are checked at the end: the session and each pass own their buffers through a vlr_bam::Buffers, which checks the guards
// of all of them in one call and releases them.  The session's common state, the wiring of a file into the
// device reader and the SNV / MNV loci on the device are vlr_bamsession.h's.
#include <cstring>

#include "vlr_bamsession.h"
#include "vlr_fragpileup.h"
#include "vlr_pairscore.h"
#include "vlr_altvariants.h"

static_assert(sizeof(vlr_indelpileup_hit) == 64, "hit layout");
static_assert(sizeof(vlr_fragpileup_obs) == 56, "observation layout");
static_assert(sizeof(vlr_fragpileup_locus) == 24, "locus record layout");
static_assert(sizeof(vlr_fp::Member) == 72, "member layout");
static_assert(sizeof(vlr_fp::AltKey) == 16, "key layout");
static_assert(sizeof(vlr_fp::Side) == 32, "side record layout");
static_assert(sizeof(vlr_fragpileup_indel_obs) == 24, "indel side record layout");
static_assert(sizeof(vlr_fragpileup_indel_locus) == 16, "indel locus record layout");
static_assert(sizeof(vlr_fragpileup_alt_hit) == 8, "alt hit layout");

namespace vlr_fp {

using vlr_bam::C_BAD;
using vlr_bam::C_FIRST_BAD;
using vlr_bam::C_REJECTED;
using vlr_bam::kScanThreads;
enum { K_MEMBERS = 0, K_NAME = 1, K_XA = 2, K_N = 3, K_EV = 3, K_X = 4, K_Y = 5, K_N_REALIGN = 6 };   // the counts of a record; the last three of a realigning session
constexpr int kThreads = 256;
constexpr int kLocusThreads = 256;
constexpr uint32_t kMax = VLR_FRAGPILEUP_MAX_MEMBERS;
constexpr uint32_t kSentinel = 0xffffffffu;
constexpr uint16_t kNoRank = 0xffffu;

// what the fill kernel of a realigning session needs beyond the members' arguments (on = false: every other session)
struct EvFill {
    bool on;
    Realign ra;
    const uint64_t *eoff, *xoff, *yoff;     // the chunk's scanned evidence / x byte / y byte offsets per record
    uint64_t ev0, cap, n_ev;                // evidences in front of the chunk, the capacity, the chunk's evidences
    uint64_t x0, y0, x_bytes, y_bytes;      // pair bytes in front of the chunk, the chunk's
    vlr_indelpileup_hit* hits;              // [cap]
    uint32_t* member;                       // [cap] the member of an evidence
    uint64_t *gx, *gy;                      // [2 * cap + 1] session-wide offsets of the pairs
    vlr_ip::Src* src;                       // [n_ev] chunk-local
};

// what the fill kernel of an indel session needs beyond that (on = false: every other session)
struct IndelFill {
    bool on;
    int64_t max_locus_len;
    uint64_t member_cap;
    Side* sides;                            // [member_cap] parallel to the members
    uint32_t *max_del, *max_ins;            // [n_loci]
    unsigned long long* max_clip;           // [n_loci] clip << 32 | l_seq (vlr_fp::clip_frac_greater)
};

// the windows of an indel candidate's evidence in the fragment session: the alt allele window is the locus's own (vlr_bp::Loci::alt_bases
// at base_off), computed by the caller as for vlr_indelpileup_open
struct IndelAltWindows {
    vlr_bp::Loci L;
    const uint8_t* const* ctg;
    Realign ra;
    __device__ int64_t n_loci() const { return L.n; }
    __device__ int32_t ref_id(uint32_t locus) const { return L.ref_id[locus]; }
    __device__ const uint8_t* contig(int32_t ref_id) const { return ctg[ref_id]; }
    __device__ int64_t contig_len(int32_t ref_id) const { return ra.ctg_len[ref_id]; }
    __device__ uint32_t alt_len(uint32_t locus, int64_t) const { return (uint32_t)(L.base_off[locus + 1] - L.base_off[locus]); }
    __device__ uint8_t alt_byte(uint32_t locus, const uint8_t*, int64_t, uint32_t k) const { return L.alt_bases[L.base_off[locus] + k]; }
};

// the windows of a realigned SNV / MNV evidence: the alt allele window is the contig with the locus bytes replaced (vlr_fp::alt_window)
struct SnvWindows {
    vlr_bp::Loci L;
    const uint8_t* const* ctg;
    Realign ra;
    __device__ int64_t n_loci() const { return L.n; }
    __device__ int32_t ref_id(uint32_t locus) const { return L.ref_id[locus]; }
    __device__ const uint8_t* contig(int32_t ref_id) const { return ctg[ref_id]; }
    __device__ int64_t contig_len(int32_t ref_id) const { return ra.ctg_len[ref_id]; }
    __device__ uint32_t alt_len(uint32_t locus, int64_t contig_len) const { int64_t b, e; alt_window(L, (int64_t)locus, contig_len, ra.window, &b, &e); return (uint32_t)(e - b); }
    __device__ uint8_t alt_byte(uint32_t locus, const uint8_t* contig, int64_t contig_len, uint32_t k) const {
        int64_t b, e;
        alt_window(L, (int64_t)locus, contig_len, ra.window, &b, &e);
        return alt_window_byte(L, (int64_t)locus, contig, contig_len, b, k);
    }
};

// one evidence per thread: the normalised supports (or the evidence's status) into its member
__global__ __launch_bounds__(kThreads) void frag_apply_kernel(const vlr_indelpileup_hit* __restrict__ hits, const uint32_t* __restrict__ member, const double* __restrict__ norm,
                                                              uint64_t n_ev, uint64_t member_cap, Member* __restrict__ members) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_ev) return;
    const uint32_t m = member[e];
    if ((uint64_t)m >= member_cap) return;
    apply_realigned(members[m], hits[e], norm[2 * e], norm[2 * e + 1]);
}

// The bodies of the member pass.  kRealign: a realigning session; kIndel (with kRealign): an indel session.  The kernels below keep the
// signatures and names every session had before; the indel session has kernels of its own with the arguments only it needs.
template <bool kRealign, bool kIndel>
__device__ __forceinline__ void frag_count_body(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                              vlr_bp::Tables t, vlr_bp::Loci L, int realign, int64_t window, uint64_t coeff,
                                                              uint32_t* __restrict__ cnt, uint32_t* __restrict__ nbytes, uint32_t* __restrict__ nxa,
                                                              unsigned long long* __restrict__ counters, Realign ra, uint32_t* __restrict__ nev,
                                                              uint32_t* __restrict__ nxb, uint32_t* __restrict__ nyb, int64_t max_locus_len,
                                                              const uint64_t* __restrict__ comp_off = nullptr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = starts[i], end = starts[i + 1];
    const Indel ia{max_locus_len, nullptr};
    const RecMembers r = record_members(t, L, base + o, end - o, rec0 + (uint64_t)i, realign != 0, window, coeff, nullptr, 0, 0, nullptr, 0, nullptr, 0,
                                        kRealign ? &ra : nullptr, nullptr, 0, kIndel ? &ia : nullptr, comp_off);
    cnt[i] = r.n_members;
    nbytes[i] = r.name_bytes;
    nxa[i] = r.n_xa;
    if constexpr (kRealign) { nev[i] = r.n_ev; nxb[i] = r.x_bytes; nyb[i] = r.y_bytes; }
    if (r.cls == vlr_bp::REC_REJECTED) atomicAdd(&counters[C_REJECTED], 1ull);
    if (r.cls == vlr_bp::REC_BAD) { atomicAdd(&counters[C_BAD], 1ull); atomicMin(&counters[C_FIRST_BAD], (unsigned long long)(rec0 + (uint64_t)i)); }
}

template <bool kRealign, bool kIndel>
__device__ __forceinline__ void frag_fill_body(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                             vlr_bp::Tables t, vlr_bp::Loci L, int realign, int64_t window, uint64_t coeff,
                                                             const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ nbytes, const uint64_t* __restrict__ off,
                                                             const uint64_t* __restrict__ noff, const uint64_t* __restrict__ xoff, uint64_t member0, uint64_t member_cap,
                                                             uint64_t name0, uint64_t name_cap, uint64_t key0, uint64_t key_cap, Member* __restrict__ members,
                                                             uint8_t* __restrict__ names, AltKey* __restrict__ keys, uint32_t* __restrict__ locus_cnt, EvFill ev, IndelFill in,
                                                             const uint64_t* __restrict__ comp_off = nullptr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // the end of the chunk's pairs, for the last evidence's windows (index 2 * (ev0 + n_ev) <= 2 * capacity: the arrays hold one more)
    if (kRealign && i == 0 && ev.on) { ev.gx[2 * (ev.ev0 + ev.n_ev)] = ev.x0 + ev.x_bytes; ev.gy[2 * (ev.ev0 + ev.n_ev)] = ev.y0 + ev.y_bytes; }
    if (i >= n || cnt[i] == 0) return;
    const uint64_t first = member0 + off[i];
    if (first >= member_cap) return;
    const uint64_t room = member_cap - first;
    const uint64_t name_at = name0 + noff[i];
    uint8_t* name_dst = name_at + (uint64_t)nbytes[i] <= name_cap ? names + name_at : nullptr;
    const uint64_t key_at = key0 + xoff[i];
    const uint64_t key_room = key_at < key_cap ? key_cap - key_at : 0;
    const uint64_t o = starts[i], end = starts[i + 1];
    // (a realigning fill runs only when every member and every evidence of the chunk fits its buffer)
    const uint64_t e_first = kRealign && ev.on ? ev.ev0 + ev.eoff[i] : 0;
    const uint64_t e_room = kRealign && ev.on && e_first < ev.cap ? ev.cap - e_first : 0;
    // (first < member_cap == in.member_cap: the Side records of the record's members lie at sides[first ...) below the same room)
    const Indel ia{in.max_locus_len, kIndel && in.on && first < in.member_cap ? in.sides + first : nullptr};
    // an indel session realigns every member: its record_members takes the indel arm only with the Realign (ev.on); without it (an
    // overflow: nothing more is kept) the members are not written either
    if (kIndel && !(ev.on && in.on)) return;
    const RecMembers r = record_members(t, L, base + o, end - o, rec0 + (uint64_t)i, realign != 0, window, coeff, members + first, room, name_at, name_dst, key_at,
                                        key_room ? keys + key_at : nullptr, key_room, kRealign && ev.on ? &ev.ra : nullptr, e_room ? ev.hits + e_first : nullptr, e_room,
                                        kIndel ? &ia : nullptr, comp_off);
    const uint64_t written = std::min<uint64_t>(r.n_members, room);
    if (kRealign && e_room) {   // the evidences of the record: their members, the offsets of their pairs, where their read windows come from
        uint64_t x = ev.x0 + ev.xoff[i], y = ev.y0 + ev.yoff[i], e = 0;
        for (uint64_t k = 0; k < written && e < r.n_ev && e < e_room && ev.eoff[i] + e < ev.n_ev; ++k) {
            const Member& m = members[first + k];
            if (!kIndel && (!(m.bits & M_ENCLOSING) || !(m.status & VLR_BASEPILEUP_HIT_NEEDS_REALIGN))) continue;
            const vlr_indelpileup_hit h = ev.hits[e_first + e];
            uint64_t alt = 0;
            if (kIndel) { if (!h.status && (int64_t)h.locus < L.n) alt = L.base_off[h.locus + 1] - L.base_off[h.locus]; }
            else if (!h.status) { int64_t ab, ae; alt_window(L, (int64_t)h.locus, ev.ra.ctg_len[L.ref_id[h.locus]], ev.ra.window, &ab, &ae); alt = (uint64_t)(ae - ab); }
            const uint64_t pr = 2 * (e_first + e);
            ev.member[e_first + e] = (uint32_t)(first + k);
            ev.gx[pr] = x; x += h.ref_len;
            ev.gx[pr + 1] = x; x += alt;
            ev.gy[pr] = y; y += h.read_len;
            ev.gy[pr + 1] = y; y += h.read_len;
            ev.src[ev.eoff[i] + e] = vlr_ip::Src{o + r.seq_off, o + r.qual_off, r.l_seq, 0u};
            ++e;
        }
    }
    for (uint64_t k = 0; k < written; ++k) {
        const uint32_t li = members[first + k].locus;
        if ((int64_t)li < L.n) atomicAdd(&locus_cnt[li], 1u);
        if (kIndel && in.on && (int64_t)li < L.n) {   // the record's CIGAR maxima into the locus: maxima over total orders
            if (r.max_del) atomicMax(&in.max_del[li], r.max_del);
            if (r.max_ins) atomicMax(&in.max_ins[li], r.max_ins);
            if (r.max_clip && r.l_seq) {
                const unsigned long long mine = ((unsigned long long)r.max_clip << 32) | (unsigned long long)r.l_seq;
                unsigned long long seen = in.max_clip[li];
                while (clip_frac_greater(mine, seen)) {
                    const unsigned long long was = atomicCAS(&in.max_clip[li], seen, mine);
                    if (was == seen) break;
                    seen = was;
                }
            }
        }
    }
}

// kRealign: the instance of a realigning session; the other instance is the kernel every session had before
template <bool kRealign>
__global__ __launch_bounds__(kThreads) void frag_count_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                              vlr_bp::Tables t, vlr_bp::Loci L, int realign, int64_t window, uint64_t coeff,
                                                              uint32_t* __restrict__ cnt, uint32_t* __restrict__ nbytes, uint32_t* __restrict__ nxa,
                                                              unsigned long long* __restrict__ counters, Realign ra, uint32_t* __restrict__ nev,
                                                              uint32_t* __restrict__ nxb, uint32_t* __restrict__ nyb) {
    frag_count_body<kRealign, false>(base, starts, n, rec0, t, L, realign, window, coeff, cnt, nbytes, nxa, counters, ra, nev, nxb, nyb, 0);
}
__global__ __launch_bounds__(kThreads) void frag_count_indel_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                                    vlr_bp::Tables t, vlr_bp::Loci L, int realign, int64_t window, uint64_t coeff,
                                                                    uint32_t* __restrict__ cnt, uint32_t* __restrict__ nbytes, uint32_t* __restrict__ nxa,
                                                                    unsigned long long* __restrict__ counters, Realign ra, uint32_t* __restrict__ nev,
                                                                    uint32_t* __restrict__ nxb, uint32_t* __restrict__ nyb, int64_t max_locus_len) {
    frag_count_body<true, true>(base, starts, n, rec0, t, L, realign, window, coeff, cnt, nbytes, nxa, counters, ra, nev, nxb, nyb, max_locus_len);
}

template <bool kRealign>
__global__ __launch_bounds__(kThreads) void frag_fill_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                             vlr_bp::Tables t, vlr_bp::Loci L, int realign, int64_t window, uint64_t coeff,
                                                             const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ nbytes, const uint64_t* __restrict__ off,
                                                             const uint64_t* __restrict__ noff, const uint64_t* __restrict__ xoff, uint64_t member0, uint64_t member_cap,
                                                             uint64_t name0, uint64_t name_cap, uint64_t key0, uint64_t key_cap, Member* __restrict__ members,
                                                             uint8_t* __restrict__ names, AltKey* __restrict__ keys, uint32_t* __restrict__ locus_cnt, EvFill ev) {
    frag_fill_body<kRealign, false>(base, starts, n, rec0, t, L, realign, window, coeff, cnt, nbytes, off, noff, xoff, member0, member_cap, name0, name_cap, key0, key_cap,
                                    members, names, keys, locus_cnt, ev, IndelFill{});
}
__global__ __launch_bounds__(kThreads) void frag_fill_indel_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                                   vlr_bp::Tables t, vlr_bp::Loci L, int realign, int64_t window, uint64_t coeff,
                                                                   const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ nbytes, const uint64_t* __restrict__ off,
                                                                   const uint64_t* __restrict__ noff, const uint64_t* __restrict__ xoff, uint64_t member0, uint64_t member_cap,
                                                                   uint64_t name0, uint64_t name_cap, uint64_t key0, uint64_t key_cap, Member* __restrict__ members,
                                                                   uint8_t* __restrict__ names, AltKey* __restrict__ keys, uint32_t* __restrict__ locus_cnt, EvFill ev,
                                                                   IndelFill in) {
    frag_fill_body<true, true>(base, starts, n, rec0, t, L, realign, window, coeff, cnt, nbytes, off, noff, xoff, member0, member_cap, name0, name_cap, key0, key_cap,
                               members, names, keys, locus_cnt, ev, in);
}

// The member pass of a realigning session with vlr_fragpileup_set_alt_variants: the realigning instances of the two bodies with the
// loci's competitor offsets, so that an MNV with a competitor realigns every enclosing record (vlr_fp::record_members).  The x and y
// bytes they count stay those of the evidence's own two pairs: the competitors' pairs exist only while a range is scored.
__global__ __launch_bounds__(kThreads) void frag_count_alt_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                                  vlr_bp::Tables t, vlr_bp::Loci L, int realign, int64_t window, uint64_t coeff,
                                                                  uint32_t* __restrict__ cnt, uint32_t* __restrict__ nbytes, uint32_t* __restrict__ nxa,
                                                                  unsigned long long* __restrict__ counters, Realign ra, uint32_t* __restrict__ nev,
                                                                  uint32_t* __restrict__ nxb, uint32_t* __restrict__ nyb, const uint64_t* __restrict__ comp_off) {
    frag_count_body<true, false>(base, starts, n, rec0, t, L, realign, window, coeff, cnt, nbytes, nxa, counters, ra, nev, nxb, nyb, 0, comp_off);
}
__global__ __launch_bounds__(kThreads) void frag_fill_alt_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                                 vlr_bp::Tables t, vlr_bp::Loci L, int realign, int64_t window, uint64_t coeff,
                                                                 const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ nbytes, const uint64_t* __restrict__ off,
                                                                 const uint64_t* __restrict__ noff, const uint64_t* __restrict__ xoff, uint64_t member0, uint64_t member_cap,
                                                                 uint64_t name0, uint64_t name_cap, uint64_t key0, uint64_t key_cap, Member* __restrict__ members,
                                                                 uint8_t* __restrict__ names, AltKey* __restrict__ keys, uint32_t* __restrict__ locus_cnt, EvFill ev,
                                                                 const uint64_t* __restrict__ comp_off) {
    frag_fill_body<true, false>(base, starts, n, rec0, t, L, realign, window, coeff, cnt, nbytes, off, noff, xoff, member0, member_cap, name0, name_cap, key0, key_cap,
                                members, names, keys, locus_cnt, ev, IndelFill{}, comp_off);
}

// The passes of a range of evidences in a session with competitors (vlr_altvariants.h has their text and their bounds).
// One wave per evidence: its windows into its 2 + K pairs.  gx / gy: the session-wide offsets of the evidences' own two pairs
// (at 2 * e), xb / yb / yq the session's pair arrays; pair_base[n_ev + 1], xoff / yoff [n_pairs + 1]: the range's, from the host.
__global__ __launch_bounds__(vlr_ip::kThreads) void frag_alt_expand_kernel(uint64_t n_ev, const vlr_indelpileup_hit* __restrict__ hits, vlr_av::Table tab,
                                                                           const uint64_t* __restrict__ gx, const uint64_t* __restrict__ gy, const uint8_t* __restrict__ xb,
                                                                           const uint8_t* __restrict__ yb, const uint8_t* __restrict__ yq,
                                                                           const uint32_t* __restrict__ pair_base, const uint32_t* __restrict__ xoff,
                                                                           const uint32_t* __restrict__ yoff, uint8_t* __restrict__ x, uint8_t* __restrict__ y,
                                                                           uint8_t* __restrict__ q) {
    const uint64_t e = (uint64_t)blockIdx.x * (vlr_ip::kThreads / 64) + (threadIdx.x >> 6);
    if (e >= n_ev) return;
    const vlr_indelpileup_hit h = hits[e];
    if (h.status || (int64_t)h.locus >= tab.n_loci) return;   // (an evidence with a status: its pairs are empty)
    const uint32_t p0 = pair_base[e], k = pair_base[e + 1] - p0 - 2u;
    const uint64_t x0 = gx[2 * e], x1 = gx[2 * e + 1], x2 = gx[2 * e + 2], y0 = gy[2 * e], y1 = gy[2 * e + 1];
    vlr_av::expand_evidence(threadIdx.x & 63u, 64u, tab, h.locus, k, xb + x0, (uint32_t)(x1 - x0), (uint32_t)(x2 - x1), yb + y0, yq + y0, (uint32_t)(y1 - y0), xoff, yoff, p0,
                            x, y, q);
}

// One evidence per thread: the tied set of its reference side.  keep / klx / kly [n_pairs]: the flag and the bytes of a kept pair
// (0 otherwise), the three count arrays of the compaction's scan; band[n_pairs].
__global__ __launch_bounds__(kThreads) void frag_alt_select_kernel(uint64_t n_ev, const uint32_t* __restrict__ pair_base, const int32_t* __restrict__ dist,
                                                                   const uint32_t* __restrict__ xoff, const uint32_t* __restrict__ yoff, int fast, uint32_t* __restrict__ keep,
                                                                   uint32_t* __restrict__ klx, uint32_t* __restrict__ kly, int32_t* __restrict__ band) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_ev) return;
    const uint32_t p0 = pair_base[e], np = pair_base[e + 1] - p0;
    if (np < 2u || np > (uint32_t)vlr_av::kMaxPairs) return;
    const vlr_av::Selected s = vlr_av::select(dist + p0, np - 2u);
    for (uint32_t j = 0; j < np; ++j) {
        const uint32_t p = p0 + j, on = (s.keep >> j) & 1u;
        keep[p] = on;
        klx[p] = on ? xoff[p + 1] - xoff[p] : 0u;
        kly[p] = on ? yoff[p + 1] - yoff[p] : 0u;
        band[p] = vlr_av::band_of(dist[p], fast != 0);
    }
}

// One wave per pair: a kept pair into the compacted batch, at the places the scans gave it (slot / cx_at / cy_at [n_pairs]).
__global__ __launch_bounds__(vlr_ip::kThreads) void frag_alt_compact_kernel(uint64_t n_pairs, const uint32_t* __restrict__ keep, const uint64_t* __restrict__ slot,
                                                                            const uint64_t* __restrict__ cx_at, const uint64_t* __restrict__ cy_at,
                                                                            const uint32_t* __restrict__ xoff, const uint32_t* __restrict__ yoff, const uint8_t* __restrict__ x,
                                                                            const uint8_t* __restrict__ y, const uint8_t* __restrict__ q, const int32_t* __restrict__ band,
                                                                            uint64_t n_kept, uint64_t x_total, uint64_t y_total, uint32_t* __restrict__ cxoff,
                                                                            uint32_t* __restrict__ cyoff, int32_t* __restrict__ cband, uint8_t* __restrict__ cx,
                                                                            uint8_t* __restrict__ cy, uint8_t* __restrict__ cq) {
    const uint64_t p = (uint64_t)blockIdx.x * (vlr_ip::kThreads / 64) + (threadIdx.x >> 6);
    if (p >= n_pairs || !keep[p]) return;
    vlr_av::compact_pair(threadIdx.x & 63u, 64u, xoff, yoff, x, y, q, (uint32_t)p, band[p], slot[p], cx_at[p], cy_at[p], n_kept, x_total, y_total, cxoff, cyoff, cband, cx, cy,
                         cq);
}

// One evidence per thread: the winner of its tied set into the evidence (ln_ref, dist_ref, ln_alt, dist_alt) and its side record.
__global__ __launch_bounds__(kThreads) void frag_alt_collect_kernel(uint64_t n_ev, uint64_t hit0, uint64_t capacity, const uint32_t* __restrict__ pair_base,
                                                                    const int32_t* __restrict__ dist, const uint64_t* __restrict__ slot, const double* __restrict__ lnp,
                                                                    uint64_t n_kept, vlr_indelpileup_hit* __restrict__ hits, vlr_fragpileup_alt_hit* __restrict__ alt) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_ev || hit0 + e >= capacity) return;
    const uint32_t p0 = pair_base[e], np = pair_base[e + 1] - p0;
    if (np < 2u || np > (uint32_t)vlr_av::kMaxPairs) return;
    vlr_av::collect_evidence(dist + p0, np - 2u, slot + p0, lnp, n_kept, hits + hit0 + e, alt + hit0 + e);
}

// The member pass of a methylation session: the count and the fill of frag_count_body / frag_fill_body without evidences, over
// record_members_meth.  The same bounds: members[k] for k < member_cap, names below name_cap, keys below key_cap.
__global__ __launch_bounds__(kThreads) void frag_count_meth_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                                   vlr_bp::Tables t, vlr_bp::Loci L, Meth me, int64_t window, uint64_t coeff, uint32_t* __restrict__ cnt,
                                                                   uint32_t* __restrict__ nbytes, uint32_t* __restrict__ nxa, unsigned long long* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = starts[i], end = starts[i + 1];
    const RecMembers r = record_members_meth(t, L, me, base + o, end - o, rec0 + (uint64_t)i, window, coeff, nullptr, 0, 0, nullptr, 0, nullptr, 0);
    cnt[i] = r.n_members;
    nbytes[i] = r.name_bytes;
    nxa[i] = r.n_xa;
    if (r.cls == vlr_bp::REC_REJECTED) atomicAdd(&counters[C_REJECTED], 1ull);
    if (r.cls == vlr_bp::REC_BAD) { atomicAdd(&counters[C_BAD], 1ull); atomicMin(&counters[C_FIRST_BAD], (unsigned long long)(rec0 + (uint64_t)i)); }
}

__global__ __launch_bounds__(kThreads) void frag_fill_meth_kernel(const uint8_t* __restrict__ base, const uint64_t* __restrict__ starts, int64_t n, uint64_t rec0,
                                                                  vlr_bp::Tables t, vlr_bp::Loci L, Meth me, int64_t window, uint64_t coeff, const uint32_t* __restrict__ cnt,
                                                                  const uint32_t* __restrict__ nbytes, const uint64_t* __restrict__ off, const uint64_t* __restrict__ noff,
                                                                  const uint64_t* __restrict__ xoff, uint64_t member0, uint64_t member_cap, uint64_t name0, uint64_t name_cap,
                                                                  uint64_t key0, uint64_t key_cap, Member* __restrict__ members, uint8_t* __restrict__ names,
                                                                  AltKey* __restrict__ keys, uint32_t* __restrict__ locus_cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || cnt[i] == 0) return;
    const uint64_t first = member0 + off[i];
    if (first >= member_cap) return;
    const uint64_t room = member_cap - first;
    const uint64_t name_at = name0 + noff[i];
    uint8_t* name_dst = name_at + (uint64_t)nbytes[i] <= name_cap ? names + name_at : nullptr;
    const uint64_t key_at = key0 + xoff[i];
    const uint64_t key_room = key_at < key_cap ? key_cap - key_at : 0;
    const uint64_t o = starts[i], end = starts[i + 1];
    const RecMembers r = record_members_meth(t, L, me, base + o, end - o, rec0 + (uint64_t)i, window, coeff, members + first, room, name_at, name_dst, key_at,
                                             key_room ? keys + key_at : nullptr, key_room);
    const uint64_t written = std::min<uint64_t>(r.n_members, room);
    for (uint64_t k = 0; k < written; ++k) {
        const uint32_t li = members[first + k].locus;
        if ((int64_t)li < L.n) atomicAdd(&locus_cnt[li], 1u);
    }
}

__global__ __launch_bounds__(kThreads) void frag_scatter_kernel(const Member* __restrict__ members, uint64_t n_members, int64_t n_loci, const uint64_t* __restrict__ locus_off,
                                                                const uint32_t* __restrict__ locus_cnt, uint32_t* __restrict__ cursor, uint32_t* __restrict__ perm) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_members) return;
    const uint32_t li = members[m].locus;
    if ((int64_t)li >= n_loci) return;
    const uint32_t k = atomicAdd(&cursor[li], 1u);
    const uint64_t slot = locus_off[li] + k;
    if (k < locus_cnt[li] && slot < n_members) perm[slot] = (uint32_t)m;
}

// a <= b in the sort's order; the sentinel is the greatest element
__device__ inline bool idx_less(const Member* __restrict__ M, const uint8_t* __restrict__ names, uint32_t a, uint32_t b) {
    if (a == kSentinel) return false;
    if (b == kSentinel) return true;
    return member_less(names, M[a], M[b]);
}

// bitonic sort of v[0 .. P), P a power of two, ascending by `less`
template <class Less>
__device__ inline void bitonic(uint32_t* v, uint32_t P, Less less) {
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += kLocusThreads) {
                const uint32_t x = i ^ j;
                if (x > i) {
                    const uint32_t a = v[i], b = v[x];
                    const bool up = (i & k) == 0;
                    if (up ? less(b, a) : less(a, b)) { v[i] = b; v[x] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// what the fragment pass of an indel session needs beyond the members (the kIndel instances of the two kernels below)
struct IndelPass {
    const Side* sides;                      // parallel to the members
    vlr_bp::Loci L;                         // kind, start, len of the loci
    int has_insert_size;
    vlr_fragpileup_indel_obs* tmpx;         // parallel to tmp
    vlr_fragpileup_indel_obs* outx;         // parallel to the output
};

template <bool kIndel>
__device__ __forceinline__ void frag_locus_body(const Member* __restrict__ M, const uint8_t* __restrict__ names, const AltKey* __restrict__ keys,
                                                                   const uint32_t* __restrict__ perm, const uint64_t* __restrict__ locus_off,
                                                                   const uint32_t* __restrict__ locus_cnt, uint32_t max_mapq, vlr_fragpileup_obs* tmp, uint32_t* pair_left,
                                                                   uint32_t* pair_right, uint16_t* __restrict__ rank_out, uint32_t* __restrict__ n_obs,
                                                                   uint32_t* __restrict__ major, AltKey* __restrict__ major_key, uint32_t* __restrict__ have_major_key,
                                                                   uint32_t* __restrict__ lstatus, IndelPass ip) {
    __shared__ uint32_t idx[kMax];
    __shared__ uint16_t rnk[kMax];
    __shared__ uint32_t part[2][kLocusThreads];
    const uint32_t l = blockIdx.x, t = threadIdx.x;
    const uint32_t n = locus_cnt[l];
    const uint64_t base = locus_off[l];
    if (n == 0 || n > kMax) {   // (uniform over the workgroup)
        if (t == 0) {
            n_obs[l] = 0; major[l] = VLR_BASEPILEUP_NO_READ_POSITION; have_major_key[l] = 0;
            lstatus[l] = n > kMax ? VLR_FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS : 0u;
        }
        return;
    }
    uint32_t P = 1;
    while (P < n) P <<= 1;
    for (uint32_t i = t; i < P; i += kLocusThreads) idx[i] = i < n ? perm[base + i] : kSentinel;
    __syncthreads();
    bitonic(idx, P, [&](uint32_t a, uint32_t b) { return idx_less(M, names, a, b); });
    // the fragment of every run of equal names
    for (uint32_t i = t; i < n; i += kLocusThreads) {
        uint16_t flag = 0;
        if (i == 0 || compare_names(names, M[idx[i - 1]], M[idx[i]]) != 0) {
            vlr_fragpileup_obs o;
            uint32_t ml, mr;
            if constexpr (kIndel) {
                vlr_fragpileup_indel_obs x;
                if (run_obs_indel(M, ip.sides, names, idx, i, n, ip.L.kind[l], ip.L.start[l], (int64_t)ip.L.len[l], ip.has_insert_size != 0, max_mapq, o, x, &ml, &mr)) {
                    tmp[base + i] = o; ip.tmpx[base + i] = x; pair_left[base + i] = ml; pair_right[base + i] = mr; flag = 1;
                }
            } else if (run_obs(M, names, idx, i, n, max_mapq, o, &ml, &mr)) { tmp[base + i] = o; pair_left[base + i] = ml; pair_right[base + i] = mr; flag = 1; }
        }
        rnk[i] = flag;
    }
    __syncthreads();
    // ranks in name order: exclusive prefix sum of the flags
    const uint32_t per = (n + kLocusThreads - 1) / kLocusThreads;
    const uint32_t lo = std::min(t * per, n), hi = std::min(lo + per, n);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += rnk[i];
    part[0][t] = sum;
    __syncthreads();
    int cur = 0;
    for (uint32_t d = 1; d < (uint32_t)kLocusThreads; d <<= 1) {
        part[cur ^ 1][t] = part[cur][t] + (t >= d ? part[cur][t - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    uint32_t run = part[cur][t] - sum;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint16_t f = rnk[i];
        rnk[i] = f ? (uint16_t)run : kNoRank;
        run += f;
    }
    const uint32_t total = part[cur][kLocusThreads - 1];
    __syncthreads();
    // major_read_position: the read positions that count, sorted; the others are sentinels behind them
    for (uint32_t i = t; i < P; i += kLocusThreads) {
        uint32_t key = kSentinel;
        if (i < n) {
            rank_out[base + i] = rnk[i];
            if (rnk[i] != kNoRank && counts_for_major(tmp[base + i])) key = tmp[base + i].read_position;
        }
        idx[i] = key;
    }
    __syncthreads();
    bitonic(idx, P, [](uint32_t a, uint32_t b) { return a < b; });
    uint32_t major_pos = VLR_BASEPILEUP_NO_READ_POSITION;
    if (t == 0) {
        uint32_t m = 0;
        while (m < n && idx[m] != kSentinel) ++m;
        bool found = false;
        const uint32_t v = major_of_sorted(idx, m, &found);
        if (found) major_pos = v;
    }
    __syncthreads();
    // major_alt_locus: the pool indices of the keys of all observations, laid out in name order by a prefix sum, sorted by key
    uint32_t ksum = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        if (rnk[i] == kNoRank) continue;
        const uint32_t mr = pair_right[base + i];
        ksum = std::min(ksum + M[pair_left[base + i]].xa_n, kMax + 1u);
        if (mr != kSentinel) ksum = std::min(ksum + M[mr].xa_n, kMax + 1u);
    }
    part[0][t] = ksum;
    __syncthreads();
    cur = 0;
    for (uint32_t d = 1; d < (uint32_t)kLocusThreads; d <<= 1) {
        part[cur ^ 1][t] = part[cur][t] + (t >= d ? part[cur][t - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    const uint32_t n_keys = part[cur][kLocusThreads - 1];   // (every slice sum is capped at kMax + 1: no overflow, and exact up to kMax)
    if (n_keys > kMax) {   // (uniform)
        if (t == 0) { n_obs[l] = 0; major[l] = VLR_BASEPILEUP_NO_READ_POSITION; have_major_key[l] = 0; lstatus[l] = VLR_FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI; }
        return;
    }
    uint32_t PK = 1;
    while (PK < n_keys) PK <<= 1;
    for (uint32_t i = t; i < PK; i += kLocusThreads) idx[i] = kSentinel;
    __syncthreads();
    uint32_t at = part[cur][t] - ksum;
    for (uint32_t i = lo; i < hi; ++i) {
        if (rnk[i] == kNoRank) continue;
        const Member& ml = M[pair_left[base + i]];
        for (uint32_t k = 0; k < ml.xa_n && at < kMax; ++k) idx[at++] = (uint32_t)(ml.xa_off + k);
        const uint32_t mr = pair_right[base + i];
        if (mr != kSentinel) for (uint32_t k = 0; k < M[mr].xa_n && at < kMax; ++k) idx[at++] = (uint32_t)(M[mr].xa_off + k);
    }
    __syncthreads();
    bitonic(idx, PK, [&](uint32_t a, uint32_t b) { return a != kSentinel && (b == kSentinel || key_less(keys[a], keys[b])); });
    if (t == 0) {
        const int64_t at_major = major_key_of_sorted(keys, idx, n_keys);
        n_obs[l] = total;
        major[l] = major_pos;
        if (at_major >= 0) major_key[l] = keys[idx[at_major]];
        have_major_key[l] = at_major >= 0 ? 1u : 0u;
        lstatus[l] = 0;
    }
}

template <bool kIndel>
__device__ __forceinline__ void frag_gather_body(const Member* __restrict__ M, const AltKey* __restrict__ keys, const vlr_fragpileup_obs* __restrict__ tmp,
                                                                    const uint32_t* __restrict__ pair_left, const uint32_t* __restrict__ pair_right,
                                                                    const uint16_t* __restrict__ rank, const uint64_t* __restrict__ locus_off,
                                                                    const uint32_t* __restrict__ locus_cnt, const uint32_t* __restrict__ n_obs, const uint64_t* __restrict__ obs_off,
                                                                    const uint32_t* __restrict__ major, const AltKey* __restrict__ major_key,
                                                                    const uint32_t* __restrict__ have_major_key, uint64_t out_cap, vlr_fragpileup_obs* __restrict__ out, IndelPass ip) {
    const uint32_t l = blockIdx.x;
    const uint32_t n = locus_cnt[l];
    if (n == 0 || n > kMax || n_obs[l] == 0) return;
    const uint64_t base = locus_off[l], at = obs_off[l];
    const uint32_t mj = major[l];
    const bool have = have_major_key[l] != 0;
    const AltKey mk = major_key[l];
    for (uint32_t i = threadIdx.x; i < n; i += kLocusThreads) {
        const uint16_t r = rank[base + i];
        if (r == kNoRank || (uint32_t)r >= n_obs[l] || at + r >= out_cap) continue;
        vlr_fragpileup_obs o = tmp[base + i];
        // ReadObservation::process: Major where the observation has a read position equal to the major one
        if (mj != VLR_BASEPILEUP_NO_READ_POSITION && o.status == 0 && o.read_position == mj) o.bits |= VLR_FRAGPILEUP_READPOS_MAJOR;
        const uint32_t mr = pair_right[base + i];
        o.alt_locus = alt_locus_class(keys, M[pair_left[base + i]], mr != kSentinel ? &M[mr] : nullptr, have, mk);
        out[at + r] = o;
        if constexpr (kIndel) ip.outx[at + r] = ip.tmpx[base + i];
    }
}

__global__ __launch_bounds__(kLocusThreads) void frag_locus_kernel(const Member* __restrict__ M, const uint8_t* __restrict__ names, const AltKey* __restrict__ keys,
                                                                   const uint32_t* __restrict__ perm, const uint64_t* __restrict__ locus_off,
                                                                   const uint32_t* __restrict__ locus_cnt, uint32_t max_mapq, vlr_fragpileup_obs* tmp, uint32_t* pair_left,
                                                                   uint32_t* pair_right, uint16_t* __restrict__ rank_out, uint32_t* __restrict__ n_obs,
                                                                   uint32_t* __restrict__ major, AltKey* __restrict__ major_key, uint32_t* __restrict__ have_major_key,
                                                                   uint32_t* __restrict__ lstatus) {
    frag_locus_body<false>(M, names, keys, perm, locus_off, locus_cnt, max_mapq, tmp, pair_left, pair_right, rank_out, n_obs, major, major_key, have_major_key, lstatus,
                           IndelPass{});
}
__global__ __launch_bounds__(kLocusThreads) void frag_locus_indel_kernel(const Member* __restrict__ M, const uint8_t* __restrict__ names, const AltKey* __restrict__ keys,
                                                                         const uint32_t* __restrict__ perm, const uint64_t* __restrict__ locus_off,
                                                                         const uint32_t* __restrict__ locus_cnt, uint32_t max_mapq, vlr_fragpileup_obs* tmp,
                                                                         uint32_t* pair_left, uint32_t* pair_right, uint16_t* __restrict__ rank_out,
                                                                         uint32_t* __restrict__ n_obs, uint32_t* __restrict__ major, AltKey* __restrict__ major_key,
                                                                         uint32_t* __restrict__ have_major_key, uint32_t* __restrict__ lstatus, IndelPass ip) {
    frag_locus_body<true>(M, names, keys, perm, locus_off, locus_cnt, max_mapq, tmp, pair_left, pair_right, rank_out, n_obs, major, major_key, have_major_key, lstatus, ip);
}

__global__ __launch_bounds__(kLocusThreads) void frag_gather_kernel(const Member* __restrict__ M, const AltKey* __restrict__ keys, const vlr_fragpileup_obs* __restrict__ tmp,
                                                                    const uint32_t* __restrict__ pair_left, const uint32_t* __restrict__ pair_right,
                                                                    const uint16_t* __restrict__ rank, const uint64_t* __restrict__ locus_off,
                                                                    const uint32_t* __restrict__ locus_cnt, const uint32_t* __restrict__ n_obs, const uint64_t* __restrict__ obs_off,
                                                                    const uint32_t* __restrict__ major, const AltKey* __restrict__ major_key,
                                                                    const uint32_t* __restrict__ have_major_key, uint64_t out_cap, vlr_fragpileup_obs* __restrict__ out) {
    frag_gather_body<false>(M, keys, tmp, pair_left, pair_right, rank, locus_off, locus_cnt, n_obs, obs_off, major, major_key, have_major_key, out_cap, out, IndelPass{});
}
__global__ __launch_bounds__(kLocusThreads) void frag_gather_indel_kernel(const Member* __restrict__ M, const AltKey* __restrict__ keys, const vlr_fragpileup_obs* __restrict__ tmp,
                                                                          const uint32_t* __restrict__ pair_left, const uint32_t* __restrict__ pair_right,
                                                                          const uint16_t* __restrict__ rank, const uint64_t* __restrict__ locus_off,
                                                                          const uint32_t* __restrict__ locus_cnt, const uint32_t* __restrict__ n_obs,
                                                                          const uint64_t* __restrict__ obs_off, const uint32_t* __restrict__ major,
                                                                          const AltKey* __restrict__ major_key, const uint32_t* __restrict__ have_major_key, uint64_t out_cap,
                                                                          vlr_fragpileup_obs* __restrict__ out, IndelPass ip) {
    frag_gather_body<true>(M, keys, tmp, pair_left, pair_right, rank, locus_off, locus_cnt, n_obs, obs_off, major, major_key, have_major_key, out_cap, out, ip);
}

}  // namespace vlr_fp

struct vlr_fragpileup : vlr_bam::Session {
    int realign = 0;
    int64_t n_loci = 0;
    int64_t win = 0;
    uint32_t max_mapq = 0;
    uint64_t member_cap = 0, name_cap = 0, key_cap = 0, coeff = 1;
    // device state (the record arrays of the base: [K_N][rec_cap] u32 counts and their offsets; d_total[K_N])
    vlr_bp::DeviceLoci dl;
    vlr_bam::Buffers buf;                // owns every d_ below but d_src, which grows
    vlr_fp::Member* d_members = nullptr;
    uint8_t* d_names = nullptr;
    vlr_fp::AltKey *d_keys = nullptr, *d_major_key = nullptr;
    uint32_t* d_have_key = nullptr;
    uint32_t *d_lcnt = nullptr, *d_cursor = nullptr, *d_nobs = nullptr, *d_major = nullptr, *d_lstatus = nullptr;
    uint64_t *d_loff = nullptr, *d_obsoff = nullptr;
    // host state
    uint64_t n_members = 0, n_name_bytes = 0, n_keys = 0;
    std::vector<vlr_fragpileup_obs> obs;
    std::vector<vlr_fragpileup_locus> locus_rec;
    int64_t n_too_deep = 0;
    double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // a realigning session (vlr_fragpileup_open_realign)
    bool realigning = false;
    int k_n = vlr_fp::K_N;               // count arrays per record
    int rl_window = 64;
    vlr_ip::ScoreParams score;
    std::vector<int32_t> h_ref_id;       // of the loci
    std::vector<int64_t> h_end;          // start + len of the loci
    vlr_ip::ContigTable ctg;
    uint64_t ev_cap = 0, x_cap = 0, y_cap = 0, pair_byte_limit = vlr_ip::kPairByteLimit;
    vlr_indelpileup_hit* d_ev = nullptr; uint32_t* d_evm = nullptr; uint64_t *d_gx = nullptr, *d_gy = nullptr;
    uint8_t *d_xb = nullptr, *d_yb = nullptr, *d_yq = nullptr;
    vlr_ip::Src* d_src = nullptr; size_t src_cap = 0;
    uint64_t n_ev = 0, x_total = 0, y_total = 0;   // evidences and pair bytes the input produced so far
    bool ev_overflow = false;
    int64_t n_ranges = 0;
    std::vector<vlr_indelpileup_hit> ev;           // the scored evidences, record-major
    double rt[4] = {0, 0, 0, 0};
    vlr_fp::Realign ra() const { return vlr_fp::Realign{rl_window, (int64_t)ctg.h_len.size() - 1, ctg.d_len}; }
    // an indel session (vlr_fragpileup_open_indel): a realigning session with these beside it
    bool indel = false;
    int has_insert_size = 0;
    int64_t max_locus_len = 0;
    vlr_fp::Side* d_sides = nullptr;                 // [member_cap]
    uint32_t *d_max_del = nullptr, *d_max_ins = nullptr; unsigned long long* d_max_clip = nullptr;   // [n_loci]
    std::vector<vlr_fragpileup_indel_obs> obsx;      // parallel to obs
    std::vector<vlr_fragpileup_indel_locus> locusx;  // [n_loci]
    // a methylation session (vlr_fragpileup_open_methylation)
    bool meth = false;
    vlr_fp::Meth me{0, {nullptr, nullptr}};
    double* d_meth_tables = nullptr;                 // ln_meth[256], ln_unmeth[256]
    // a session with vlr_fragpileup_set_alt_variants: the competitor table (host and device) and what the scoring says of it
    bool alt_set = false, bam_added = false;
    uint64_t alt_limit = 0;                          // the longest competitor window the session takes
    std::vector<uint64_t> h_comp_off, h_comp_boff;
    uint64_t *d_comp_off = nullptr, *d_comp_boff = nullptr; uint8_t* d_comp_bases = nullptr;
    std::vector<vlr_fragpileup_alt_hit> alt_hits;    // parallel to ev
    int64_t n_edit_pairs = 0, n_hmm_pairs = 0, n_loci_with_comp = 0;
    vlr_av::Table alt_table() const { return vlr_av::Table{n_loci, d_comp_off, d_comp_boff, d_comp_bases}; }
    vlr_fp::IndelFill indel_fill() const { return vlr_fp::IndelFill{indel, max_locus_len, member_cap, d_sides, d_max_del, d_max_ins, d_max_clip}; }
};

namespace vlr_fp {
using vlr_bam::bfail;
using vlr_bam::now_s;

// a realigning session: the contig table of a file; every locus must lie inside its contig
int on_header(vlr_fragpileup* s, const std::vector<std::string>& names, const char* path) {
    const int rc = s->ctg.on_header(s->h_ref_id, names, path);
    if (rc != VLR_OK) return rc;
    for (size_t k = 0; k < s->h_ref_id.size(); ++k) {
        const int64_t end = s->h_end[k];
        if (end > s->ctg.h_len[(size_t)s->h_ref_id[k]])
            return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: locus %zu ends at %lld, behind the %lld bases of its contig in the reference", path, k, (long long)end,
                         (long long)s->ctg.h_len[(size_t)s->h_ref_id[k]]);
    }
    return VLR_OK;
}

int run_chunk(vlr_fragpileup* s, vlr_dev_file* df, int64_t n, hipStream_t st) {
    const uint8_t* d_base; const uint64_t* d_starts;
    int rc = vlr_dev_file_split_view(df, &d_base, &d_starts);
    if (rc != VLR_OK || (rc = vlr_bam::reserve_records<uint32_t>(*s, n, s->k_n, st)) != VLR_OK) return rc;
    const double t0 = now_s();
    const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
    const uint64_t rec0 = s->n_records;
    const size_t stride = s->rec_cap;
    uint32_t *d_cnt = (uint32_t*)s->d_cnt, *d_nbytes = d_cnt + K_NAME * stride, *d_nxa = d_cnt + K_XA * stride;
    if (s->meth)
        hipLaunchKernelGGL(frag_count_meth_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->me, s->win, s->coeff, d_cnt, d_nbytes,
                           d_nxa, s->d_counters);
    else if (s->indel)
        hipLaunchKernelGGL(frag_count_indel_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->realign, s->win, s->coeff,
                           d_cnt, d_nbytes, d_nxa, s->d_counters, s->ra(), d_cnt + K_EV * stride, d_cnt + K_X * stride, d_cnt + K_Y * stride, s->max_locus_len);
    else if (s->realigning && s->alt_set)
        hipLaunchKernelGGL(frag_count_alt_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->realign, s->win, s->coeff, d_cnt,
                           d_nbytes, d_nxa, s->d_counters, s->ra(), d_cnt + K_EV * stride, d_cnt + K_X * stride, d_cnt + K_Y * stride, s->d_comp_off);
    else if (s->realigning)
        hipLaunchKernelGGL(frag_count_kernel<true>, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->realign, s->win, s->coeff, d_cnt,
                           d_nbytes, d_nxa, s->d_counters, s->ra(), d_cnt + K_EV * stride, d_cnt + K_X * stride, d_cnt + K_Y * stride);
    else
        hipLaunchKernelGGL(frag_count_kernel<false>, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->realign, s->win, s->coeff, d_cnt,
                           d_nbytes, d_nxa, s->d_counters, Realign{0, 0, nullptr}, nullptr, nullptr, nullptr);
    uint64_t total[K_N_REALIGN] = {0, 0, 0, 0, 0, 0};
    if ((rc = vlr_bam::scan_records<uint32_t>(*s, n, s->k_n, total, st)) != VLR_OK) return rc;
    // once a buffer has overflowed nothing more is written: the session only counts on
    const bool fits = s->n_members <= s->member_cap && s->n_name_bytes <= s->name_cap && s->n_keys <= s->key_cap;
    // the evidences of the chunk are written when all of them, and all its members, fit (counted, not written, otherwise)
    if (s->realigning && (s->n_ev + total[K_EV] > s->ev_cap || s->x_total + total[K_X] > s->x_cap || s->y_total + total[K_Y] > s->y_cap)) s->ev_overflow = true;
    EvFill ev{};
    ev.on = s->realigning && total[K_EV] > 0 && !s->ev_overflow && fits && s->n_members + total[K_MEMBERS] <= s->member_cap;
    if (ev.on) {
        if ((rc = vlr_bam::grow(s->d_src, s->src_cap, (size_t)total[K_EV])) != VLR_OK) return rc;
        ev.ra = s->ra();
        ev.eoff = s->d_off + K_EV * stride; ev.xoff = s->d_off + K_X * stride; ev.yoff = s->d_off + K_Y * stride;
        ev.ev0 = s->n_ev; ev.cap = s->ev_cap; ev.n_ev = total[K_EV];
        ev.x0 = s->x_total; ev.y0 = s->y_total; ev.x_bytes = total[K_X]; ev.y_bytes = total[K_Y];
        ev.hits = s->d_ev; ev.member = s->d_evm; ev.gx = s->d_gx; ev.gy = s->d_gy; ev.src = s->d_src;
    }
    if (total[K_MEMBERS] && fits && s->n_members < s->member_cap) {
        if (s->meth)
            hipLaunchKernelGGL(frag_fill_meth_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->me, s->win, s->coeff, d_cnt, d_nbytes,
                               s->d_off, s->d_off + K_NAME * stride, s->d_off + K_XA * stride, s->n_members, s->member_cap, s->n_name_bytes, s->name_cap, s->n_keys, s->key_cap,
                               s->d_members, s->d_names, s->d_keys, s->d_lcnt);
        else if (s->indel)
            hipLaunchKernelGGL(frag_fill_indel_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->realign, s->win, s->coeff, d_cnt,
                               d_nbytes, s->d_off, s->d_off + K_NAME * stride, s->d_off + K_XA * stride, s->n_members, s->member_cap, s->n_name_bytes, s->name_cap, s->n_keys,
                               s->key_cap, s->d_members, s->d_names, s->d_keys, s->d_lcnt, ev, s->indel_fill());
        else if (s->realigning && s->alt_set)
            hipLaunchKernelGGL(frag_fill_alt_kernel, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->realign, s->win, s->coeff, d_cnt, d_nbytes,
                               s->d_off, s->d_off + K_NAME * stride, s->d_off + K_XA * stride, s->n_members, s->member_cap, s->n_name_bytes, s->name_cap, s->n_keys, s->key_cap,
                               s->d_members, s->d_names, s->d_keys, s->d_lcnt, ev, s->d_comp_off);
        else if (s->realigning)
            hipLaunchKernelGGL(frag_fill_kernel<true>, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->realign, s->win, s->coeff, d_cnt, d_nbytes,
                               s->d_off, s->d_off + K_NAME * stride, s->d_off + K_XA * stride, s->n_members, s->member_cap, s->n_name_bytes, s->name_cap, s->n_keys, s->key_cap,
                               s->d_members, s->d_names, s->d_keys, s->d_lcnt, ev);
        else
            hipLaunchKernelGGL(frag_fill_kernel<false>, dim3(blocks), dim3(kThreads), 0, st, d_base, d_starts, n, rec0, s->dl.tables, s->dl.loci, s->realign, s->win, s->coeff, d_cnt, d_nbytes,
                               s->d_off, s->d_off + K_NAME * stride, s->d_off + K_XA * stride, s->n_members, s->member_cap, s->n_name_bytes, s->name_cap, s->n_keys, s->key_cap,
                               s->d_members, s->d_names, s->d_keys, s->d_lcnt, ev);
        VLR_HIP_OK(hipStreamSynchronize(st));
        VLR_HIP_OK(hipGetLastError());
        if (ev.on) {   // the windows of the chunk's evidences, while its records are resident
            double tg = now_s();
            const unsigned waves_per_block = vlr_ip::kThreads / 64;
            const dim3 grid((unsigned)((ev.n_ev + waves_per_block - 1) / waves_per_block));
            if (s->indel)
                hipLaunchKernelGGL((vlr_ip::indelpileup_gather_kernel<IndelAltWindows, uint64_t>), grid, dim3(vlr_ip::kThreads), 0, st, d_base, ev.n_ev, s->d_ev + ev.ev0,
                                   IndelAltWindows{s->dl.loci, s->ctg.d_ctg, ev.ra}, s->d_src, s->d_gx + 2 * ev.ev0, s->d_gy + 2 * ev.ev0, s->d_xb, s->d_yb, s->d_yq);
            else
                hipLaunchKernelGGL((vlr_ip::indelpileup_gather_kernel<SnvWindows, uint64_t>), grid, dim3(vlr_ip::kThreads), 0, st, d_base, ev.n_ev, s->d_ev + ev.ev0,
                                   SnvWindows{s->dl.loci, s->ctg.d_ctg, ev.ra}, s->d_src, s->d_gx + 2 * ev.ev0, s->d_gy + 2 * ev.ev0, s->d_xb, s->d_yb, s->d_yq);
            if ((rc = vlr_ip::sync_stage(st, s->rt[0], tg)) != VLR_OK) return rc;
        }
    }
    if (s->realigning) { s->n_ev += total[K_EV]; s->x_total += total[K_X]; s->y_total += total[K_Y]; }
    s->n_members += total[K_MEMBERS];
    s->n_name_bytes += total[K_NAME];
    s->n_keys += total[K_XA];
    s->n_records += (uint64_t)n;
    s->t[3] += now_s() - t0;
    return VLR_OK;
}


// the normalised supports of the scored evidences (s->ev) into their members
int apply_pass(vlr_fragpileup* s, vlr_bam::Buffers& scratch, hipStream_t st, double& t0) {
    const size_t ne = s->ev.size();
    double* d_norm = nullptr;
    std::vector<double> norm(2 * ne);
    for (size_t e = 0; e < ne; ++e) {
        norm[2 * e] = s->ev[e].ln_ref; norm[2 * e + 1] = s->ev[e].ln_alt;
        normalize_support(&norm[2 * e], &norm[2 * e + 1]);
    }
    int rc;
    if ((rc = scratch.guarded(d_norm, 2 * ne)) != VLR_OK) return rc;
    VLR_HIP_OK(hipMemcpy(d_norm, norm.data(), 2 * ne * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(frag_apply_kernel, dim3((unsigned)((ne + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, s->d_ev, s->d_evm, d_norm, (uint64_t)ne,
                       std::min<uint64_t>(s->n_members, s->member_cap), s->d_members);
    return vlr_ip::sync_stage(st, s->rt[3], t0);
}

// The realignment of the session's evidences: scored in ranges of evidences whose pair bytes fit pair_byte_limit, normalised on the
// host, written into their members.
int realign_pass(vlr_fragpileup* s) {
    const size_t ne = (size_t)s->n_ev;
    std::vector<uint64_t> gx(2 * ne + 1), gy(2 * ne + 1);
    VLR_HIP_OK(hipMemcpy(gx.data(), s->d_gx, gx.size() * 8, hipMemcpyDeviceToHost));
    VLR_HIP_OK(hipMemcpy(gy.data(), s->d_gy, gy.size() * 8, hipMemcpyDeviceToHost));
    // (the offsets came from the device: nothing below trusts them beyond what the buffers hold)
    gx[2 * ne] = s->x_total; gy[2 * ne] = s->y_total;
    for (size_t p = 0; p < 2 * ne; ++p)
        if (gx[p] > gx[p + 1] || gy[p] > gy[p + 1] || gx[p + 1] > s->x_cap || gy[p + 1] > s->y_cap) return bfail(VLR_ERR_HIP, "vlr_fragpileup_result: the pair offsets of evidence %zu are not ascending", p / 2);
    uint32_t *d_xoff = nullptr, *d_yoff = nullptr; int32_t *d_band = nullptr, *d_dist = nullptr; double* d_lnp = nullptr;
    std::vector<uint32_t> xo, yo;
    vlr_bam::Buffers scratch;
    auto body = [&]() -> int {
        int rc;
        hipStream_t st = 0;
        for (size_t e0 = 0; e0 < ne;) {
            size_t e1 = e0 + 1;
            while (e1 < ne && gx[2 * (e1 + 1)] - gx[2 * e0] <= s->pair_byte_limit && gy[2 * (e1 + 1)] - gy[2 * e0] <= s->pair_byte_limit) ++e1;
            const size_t np = 2 * (e1 - e0);
            if (gx[2 * e1] - gx[2 * e0] >= (1ull << 32) || gy[2 * e1] - gy[2 * e0] >= (1ull << 32)) return bfail(VLR_ERR_UNSUPPORTED, "evidence %zu: its windows take 4 GiB or more", e0);
            if (!d_xoff) {   // sized once, by the first (largest possible) range: at most all pairs
                if ((rc = scratch.guarded(d_xoff, 2 * ne + 1)) != VLR_OK || (rc = scratch.guarded(d_yoff, 2 * ne + 1)) != VLR_OK ||
                    (rc = scratch.guarded(d_band, 2 * ne)) != VLR_OK || (rc = scratch.guarded(d_dist, 2 * ne)) != VLR_OK || (rc = scratch.guarded(d_lnp, 2 * ne)) != VLR_OK)
                    return rc;
            }
            xo.resize(np + 1); yo.resize(np + 1);
            for (size_t p = 0; p <= np; ++p) { xo[p] = (uint32_t)(gx[2 * e0 + p] - gx[2 * e0]); yo[p] = (uint32_t)(gy[2 * e0 + p] - gy[2 * e0]); }
            double t0 = now_s();
            VLR_HIP_OK(hipMemcpy(d_xoff, xo.data(), (np + 1) * 4, hipMemcpyHostToDevice));
            VLR_HIP_OK(hipMemcpy(d_yoff, yo.data(), (np + 1) * 4, hipMemcpyHostToDevice));
            VLR_HIP_OK(hipMemset(d_band, 0xff, np * 4));   // -1: no band
            if ((rc = vlr_ip::score_pairs(s->score, np, d_xoff, s->d_xb + gx[2 * e0], d_yoff, s->d_yb + gy[2 * e0], s->d_yq + gy[2 * e0], d_band, d_dist, d_lnp, st, s->rt[1],
                                          s->rt[2], t0)) != VLR_OK)
                return rc;
            hipLaunchKernelGGL(vlr_ip::indelpileup_collect_kernel, dim3((unsigned)((e1 - e0 + vlr_ip::kThreads - 1) / vlr_ip::kThreads)), dim3(vlr_ip::kThreads), 0, st, d_lnp, d_dist,
                               (uint64_t)(e1 - e0), (uint64_t)e0, (uint64_t)ne, s->d_ev);
            if ((rc = vlr_ip::sync_stage(st, s->rt[3], t0)) != VLR_OK) return rc;
            ++s->n_ranges;
            e0 = e1;
        }
        double t0 = now_s();
        s->ev.resize(ne);
        VLR_HIP_OK(hipMemcpy(s->ev.data(), s->d_ev, ne * sizeof(vlr_indelpileup_hit), hipMemcpyDeviceToHost));
        if ((rc = apply_pass(s, scratch, st, t0)) != VLR_OK) return rc;
        bool ok = true;
        rc = scratch.guards_intact(&ok);
        if (rc == VLR_OK && !ok) s->status |= VLR_FRAGPILEUP_GUARD_DAMAGED;
        return rc;
    };
    const int rc = body();
    scratch.free();
    return rc;
}

// The realignment of a session with competitors (vlr_fragpileup_set_alt_variants): per range of evidences whose EXPANDED pair bytes fit
// pair_byte_limit (an evidence whose own pairs exceed it is a range of its own) the windows are expanded into 2 + K pairs, all go
// through the edit-distance kernel, the select kernel marks the tied set and the alt pair, three scans (kept pairs, their x bytes,
// their y bytes) place them, the compact kernel copies them, the pair HMM of the mode runs over the compacted batch alone and the
// collect kernel takes the winner.  seconds: [1] expand + edit distance + select, [2] compaction + pair HMM, [3] collect and apply.
int realign_pass_alt(vlr_fragpileup* s) {
    const size_t ne = (size_t)s->n_ev;
    std::vector<uint64_t> gx(2 * ne + 1), gy(2 * ne + 1);
    VLR_HIP_OK(hipMemcpy(gx.data(), s->d_gx, gx.size() * 8, hipMemcpyDeviceToHost));
    VLR_HIP_OK(hipMemcpy(gy.data(), s->d_gy, gy.size() * 8, hipMemcpyDeviceToHost));
    gx[2 * ne] = s->x_total; gy[2 * ne] = s->y_total;
    for (size_t p = 0; p < 2 * ne; ++p)
        if (gx[p] > gx[p + 1] || gy[p] > gy[p + 1] || gx[p + 1] > s->x_cap || gy[p + 1] > s->y_cap) return bfail(VLR_ERR_HIP, "vlr_fragpileup_result: the pair offsets of evidence %zu are not ascending", p / 2);
    // the evidences as the fill pass wrote them: locus and status decide an evidence's pairs
    std::vector<vlr_indelpileup_hit> hv(ne);
    VLR_HIP_OK(hipMemcpy(hv.data(), s->d_ev, ne * sizeof(vlr_indelpileup_hit), hipMemcpyDeviceToHost));
    const vlr_av::Table ht{s->n_loci, s->h_comp_off.data(), s->h_comp_boff.data(), nullptr};
    // per evidence: its pairs and their bytes (vlr_av::layout_evidence), as running sums
    std::vector<uint64_t> pb(ne + 1, 0), ex(ne + 1, 0), ey(ne + 1, 0);
    uint32_t xl[vlr_av::kMaxPairs], yl[vlr_av::kMaxPairs];
    for (size_t e = 0; e < ne; ++e) {
        const vlr_indelpileup_hit& h = hv[e];
        if ((int64_t)h.locus >= s->n_loci) return bfail(VLR_ERR_HIP, "vlr_fragpileup_result: evidence %zu names locus %u of %lld", e, h.locus, (long long)s->n_loci);
        const uint64_t ref_len = gx[2 * e + 1] - gx[2 * e], alt_len = gx[2 * e + 2] - gx[2 * e + 1], read_len = gy[2 * e + 1] - gy[2 * e];
        const uint32_t np = vlr_av::layout_evidence(ht, h.locus, h.status == 0, (uint32_t)ref_len, (uint32_t)alt_len, (uint32_t)read_len, xl, yl);
        uint64_t sx = 0, sy = 0;
        for (uint32_t j = 0; j < np; ++j) { sx += xl[j]; sy += yl[j]; }
        pb[e + 1] = pb[e] + np; ex[e + 1] = ex[e] + sx; ey[e + 1] = ey[e] + sy;
    }
    // the ranges, and the largest of each quantity over them: the scratch is sized once
    std::vector<size_t> cut{0};
    size_t max_ev = 0; uint64_t max_np = 0, max_x = 0, max_y = 0;
    for (size_t e0 = 0; e0 < ne;) {
        size_t e1 = e0 + 1;
        while (e1 < ne && ex[e1 + 1] - ex[e0] <= s->pair_byte_limit && ey[e1 + 1] - ey[e0] <= s->pair_byte_limit) ++e1;
        if (ex[e1] - ex[e0] >= (1ull << 32) || ey[e1] - ey[e0] >= (1ull << 32) || pb[e1] - pb[e0] >= (1ull << 31))
            return bfail(VLR_ERR_UNSUPPORTED, "evidence %zu: its windows take 4 GiB or more", e0);
        max_ev = std::max(max_ev, e1 - e0); max_np = std::max(max_np, pb[e1] - pb[e0]); max_x = std::max(max_x, ex[e1] - ex[e0]); max_y = std::max(max_y, ey[e1] - ey[e0]);
        cut.push_back(e1);
        e0 = e1;
    }
    const size_t NP = (size_t)max_np;
    uint32_t *d_pb = nullptr, *d_xoff = nullptr, *d_yoff = nullptr, *d_cxoff = nullptr, *d_cyoff = nullptr, *d_keep = nullptr;
    int32_t *d_band = nullptr, *d_dist = nullptr, *d_cband = nullptr;
    uint64_t *d_koff = nullptr, *d_ktotal = nullptr;
    uint8_t *d_x = nullptr, *d_y = nullptr, *d_q = nullptr, *d_cx = nullptr, *d_cy = nullptr, *d_cq = nullptr;
    double* d_lnp = nullptr;
    vlr_fragpileup_alt_hit* d_alt = nullptr;
    vlr_bam::Buffers scratch;
    auto body = [&]() -> int {
        int rc = VLR_OK;
        hipStream_t st = 0;
        auto step = [&](int r) { if (rc == VLR_OK) rc = r; };
        step(scratch.guarded(d_pb, max_ev + 1)); step(scratch.guarded(d_xoff, NP + 1)); step(scratch.guarded(d_yoff, NP + 1));
        step(scratch.guarded(d_cxoff, NP + 1)); step(scratch.guarded(d_cyoff, NP + 1));
        step(scratch.guarded(d_keep, 3 * NP)); step(scratch.guarded(d_koff, 3 * NP)); step(scratch.guarded(d_ktotal, 3));
        step(scratch.guarded(d_band, NP)); step(scratch.guarded(d_dist, NP)); step(scratch.guarded(d_cband, NP)); step(scratch.guarded(d_lnp, NP));
        step(scratch.guarded(d_x, (size_t)max_x)); step(scratch.guarded(d_y, (size_t)max_y)); step(scratch.guarded(d_q, (size_t)max_y));
        step(scratch.guarded(d_cx, (size_t)max_x)); step(scratch.guarded(d_cy, (size_t)max_y)); step(scratch.guarded(d_cq, (size_t)max_y));
        step(scratch.guarded(d_alt, ne));
        if (rc != VLR_OK) return rc;
        VLR_HIP_OK(hipMemset(d_alt, 0, ne * sizeof(vlr_fragpileup_alt_hit)));
        std::vector<uint32_t> hpb, xo, yo;
        const unsigned wpb = vlr_ip::kThreads / 64;
        for (size_t c = 0; c + 1 < cut.size(); ++c) {
            const size_t e0 = cut[c], e1 = cut[c + 1], n = e1 - e0, np = (size_t)(pb[e1] - pb[e0]);
            hpb.resize(n + 1); xo.assign(np + 1, 0); yo.assign(np + 1, 0);
            for (size_t e = e0; e < e1; ++e) {
                const vlr_indelpileup_hit& h = hv[e];
                const uint32_t k = vlr_av::layout_evidence(ht, h.locus, h.status == 0, (uint32_t)(gx[2 * e + 1] - gx[2 * e]), (uint32_t)(gx[2 * e + 2] - gx[2 * e + 1]),
                                                           (uint32_t)(gy[2 * e + 1] - gy[2 * e]), xl, yl);
                const size_t p0 = (size_t)(pb[e] - pb[e0]);
                hpb[e - e0] = (uint32_t)p0;
                for (uint32_t j = 0; j < k; ++j) { xo[p0 + j + 1] = xo[p0 + j] + xl[j]; yo[p0 + j + 1] = yo[p0 + j] + yl[j]; }
            }
            hpb[n] = (uint32_t)np;
            double t0 = now_s();
            VLR_HIP_OK(hipMemcpy(d_pb, hpb.data(), (n + 1) * 4, hipMemcpyHostToDevice));
            VLR_HIP_OK(hipMemcpy(d_xoff, xo.data(), (np + 1) * 4, hipMemcpyHostToDevice));
            VLR_HIP_OK(hipMemcpy(d_yoff, yo.data(), (np + 1) * 4, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(frag_alt_expand_kernel, dim3((unsigned)((n + wpb - 1) / wpb)), dim3(vlr_ip::kThreads), 0, st, (uint64_t)n, s->d_ev + e0, s->alt_table(),
                               s->d_gx + 2 * e0, s->d_gy + 2 * e0, s->d_xb, s->d_yb, s->d_yq, d_pb, d_xoff, d_yoff, d_x, d_y, d_q);
            vlr_realign_batch_desc b;
            b.n_pairs = (int64_t)np;
            b.x_offset = d_xoff; b.x_bases = d_x; b.y_offset = d_yoff; b.y_bases = d_y; b.y_quals = d_q;
            b.max_edit_dist = nullptr;
            for (int k = 0; k < 4; ++k) b.gap[k] = s->score.gap[k];
            hipError_t he = (hipError_t)vlr_launch_edit_kernel(&b, d_dist, nullptr, nullptr, (void*)st);
            if (he != hipSuccess) return bfail(VLR_ERR_HIP, "edit-distance kernel launch: %s", hipGetErrorString(he));
            hipLaunchKernelGGL(frag_alt_select_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (uint64_t)n, d_pb, d_dist, d_xoff, d_yoff,
                               s->score.mode == VLR_INDELPILEUP_FAST ? 1 : 0, d_keep, d_keep + NP, d_keep + 2 * NP, d_band);
            hipLaunchKernelGGL(vlr_bam::scan_kernel<uint32_t>, dim3(3), dim3(kScanThreads), 0, st, d_keep, (int64_t)np, (int64_t)NP, d_koff, d_ktotal);
            uint64_t tot[3] = {0, 0, 0};
            VLR_HIP_OK(hipMemcpyAsync(tot, d_ktotal, sizeof(tot), hipMemcpyDeviceToHost, st));
            if ((rc = vlr_ip::sync_stage(st, s->rt[1], t0)) != VLR_OK) return rc;
            if (tot[0] > np || tot[1] > xo[np] || tot[2] > yo[np]) return bfail(VLR_ERR_HIP, "vlr_fragpileup_result: the compaction keeps more than the range holds");
            hipLaunchKernelGGL(frag_alt_compact_kernel, dim3((unsigned)((np + wpb - 1) / wpb)), dim3(vlr_ip::kThreads), 0, st, (uint64_t)np, d_keep, d_koff, d_koff + NP,
                               d_koff + 2 * NP, d_xoff, d_yoff, d_x, d_y, d_q, d_band, tot[0], tot[1], tot[2], d_cxoff, d_cyoff, d_cband, d_cx, d_cy, d_cq);
            b.n_pairs = (int64_t)tot[0];
            b.x_offset = d_cxoff; b.x_bases = d_cx; b.y_offset = d_cyoff; b.y_bases = d_cy; b.y_quals = d_cq;
            b.max_edit_dist = d_cband;
            if ((rc = vlr_ip::score_hmm(s->score, b, d_lnp, st)) != VLR_OK || (rc = vlr_ip::sync_stage(st, s->rt[2], t0)) != VLR_OK) return rc;
            hipLaunchKernelGGL(frag_alt_collect_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (uint64_t)n, (uint64_t)e0, (uint64_t)ne, d_pb,
                               d_dist, d_koff, d_lnp, tot[0], s->d_ev, d_alt);
            if ((rc = vlr_ip::sync_stage(st, s->rt[3], t0)) != VLR_OK) return rc;
            s->n_edit_pairs += (int64_t)np; s->n_hmm_pairs += (int64_t)tot[0];
            ++s->n_ranges;
        }
        double t0 = now_s();
        s->ev.resize(ne); s->alt_hits.resize(ne);
        VLR_HIP_OK(hipMemcpy(s->ev.data(), s->d_ev, ne * sizeof(vlr_indelpileup_hit), hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(s->alt_hits.data(), d_alt, ne * sizeof(vlr_fragpileup_alt_hit), hipMemcpyDeviceToHost));
        if ((rc = apply_pass(s, scratch, st, t0)) != VLR_OK) return rc;
        bool ok = true;
        rc = scratch.guards_intact(&ok);
        if (rc == VLR_OK && !ok) s->status |= VLR_FRAGPILEUP_GUARD_DAMAGED;
        return rc;
    };
    const int rc = body();
    scratch.free();
    return rc;
}

int fragment_pass(vlr_fragpileup* s) {
    const size_t nm = (size_t)s->n_members, nl = (size_t)s->n_loci;
    uint32_t *d_perm = nullptr, *d_left = nullptr, *d_right = nullptr; uint16_t* d_rank = nullptr; vlr_fragpileup_obs *d_tmp = nullptr, *d_out = nullptr;
    vlr_fragpileup_indel_obs *d_tmpx = nullptr, *d_outx = nullptr;   // an indel session: beside d_tmp and d_out
    vlr_bam::Buffers scratch;
    int rc = VLR_OK;
    auto step = [&](int r) { if (rc == VLR_OK) rc = r; };
    if (s->indel) step(scratch.guarded(d_tmpx, nm));
    step(scratch.guarded(d_perm, nm));
    step(scratch.guarded(d_rank, nm));
    step(scratch.guarded(d_left, nm));
    step(scratch.guarded(d_right, nm));
    step(scratch.guarded(d_tmp, nm));
    auto body = [&]() -> int {
        uint64_t total_obs = 0;
        hipLaunchKernelGGL(vlr_bam::scan_kernel<uint32_t>, dim3(1), dim3(kScanThreads), 0, 0, s->d_lcnt, (int64_t)nl, (int64_t)0, s->d_loff, s->d_total);
        hipLaunchKernelGGL(frag_scatter_kernel, dim3((unsigned)((nm + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, s->d_members, (uint64_t)nm, s->n_loci, s->d_loff,
                           s->d_lcnt, s->d_cursor, d_perm);
        IndelPass ip{s->d_sides, s->dl.loci, s->has_insert_size, d_tmpx, nullptr};
        if (s->indel)
            hipLaunchKernelGGL(frag_locus_indel_kernel, dim3((unsigned)nl), dim3(kLocusThreads), 0, 0, s->d_members, s->d_names, s->d_keys, d_perm, s->d_loff, s->d_lcnt, s->max_mapq,
                               d_tmp, d_left, d_right, d_rank, s->d_nobs, s->d_major, s->d_major_key, s->d_have_key, s->d_lstatus, ip);
        else
            hipLaunchKernelGGL(frag_locus_kernel, dim3((unsigned)nl), dim3(kLocusThreads), 0, 0, s->d_members, s->d_names, s->d_keys, d_perm, s->d_loff, s->d_lcnt, s->max_mapq,
                               d_tmp, d_left, d_right, d_rank, s->d_nobs, s->d_major, s->d_major_key, s->d_have_key, s->d_lstatus);
        hipLaunchKernelGGL(vlr_bam::scan_kernel<uint32_t>, dim3(1), dim3(kScanThreads), 0, 0, s->d_nobs, (int64_t)nl, (int64_t)0, s->d_obsoff, s->d_total + 1);
        VLR_HIP_OK(hipDeviceSynchronize());
        VLR_HIP_OK(hipGetLastError());
        VLR_HIP_OK(hipMemcpy(&total_obs, s->d_total + 1, 8, hipMemcpyDeviceToHost));
        if (total_obs > nm) return bfail(VLR_ERR_HIP, "vlr_fragpileup_result: more observations than members");
        // the output is sized by the observations, not by the members
        int r = scratch.guarded(d_out, (size_t)total_obs);
        if (r != VLR_OK) return r;
        if (s->indel && (r = scratch.guarded(d_outx, (size_t)total_obs)) != VLR_OK) return r;
        ip.outx = d_outx;
        if (s->indel)
            hipLaunchKernelGGL(frag_gather_indel_kernel, dim3((unsigned)nl), dim3(kLocusThreads), 0, 0, s->d_members, s->d_keys, d_tmp, d_left, d_right, d_rank, s->d_loff, s->d_lcnt,
                               s->d_nobs, s->d_obsoff, s->d_major, s->d_major_key, s->d_have_key, total_obs, d_out, ip);
        else
            hipLaunchKernelGGL(frag_gather_kernel, dim3((unsigned)nl), dim3(kLocusThreads), 0, 0, s->d_members, s->d_keys, d_tmp, d_left, d_right, d_rank, s->d_loff, s->d_lcnt,
                               s->d_nobs, s->d_obsoff, s->d_major, s->d_major_key, s->d_have_key, total_obs, d_out);
        VLR_HIP_OK(hipDeviceSynchronize());
        VLR_HIP_OK(hipGetLastError());
        bool ok = true;
        if ((r = scratch.guards_intact(&ok)) != VLR_OK) return r;
        if (!ok) s->status |= VLR_FRAGPILEUP_GUARD_DAMAGED;
        const double t1 = now_s();
        s->obs.resize((size_t)total_obs);
        if (total_obs) VLR_HIP_OK(hipMemcpy(s->obs.data(), d_out, (size_t)total_obs * sizeof(vlr_fragpileup_obs), hipMemcpyDeviceToHost));
        std::vector<uint32_t> lcnt(nl), nobs(nl), major(nl), lst(nl);
        std::vector<uint64_t> ooff(nl);
        VLR_HIP_OK(hipMemcpy(lcnt.data(), s->d_lcnt, nl * 4, hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(nobs.data(), s->d_nobs, nl * 4, hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(major.data(), s->d_major, nl * 4, hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(lst.data(), s->d_lstatus, nl * 4, hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(ooff.data(), s->d_obsoff, nl * 8, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < nl; ++k) {
            s->locus_rec[k] = vlr_fragpileup_locus{(int64_t)ooff[k], lcnt[k], nobs[k], major[k], lst[k]};
            if (lst[k]) ++s->n_too_deep;
        }
        if (s->indel) {
            s->obsx.resize((size_t)total_obs);
            if (total_obs) VLR_HIP_OK(hipMemcpy(s->obsx.data(), d_outx, (size_t)total_obs * sizeof(vlr_fragpileup_indel_obs), hipMemcpyDeviceToHost));
        }
        s->t[7] += now_s() - t1;
        return VLR_OK;
    };
    if (rc == VLR_OK) rc = body();
    scratch.free();
    return rc;
}

// the per-locus CIGAR maxima of an indel session, to the host
int read_maxima(vlr_fragpileup* s) {
    const size_t nl = (size_t)s->n_loci;
    std::vector<uint32_t> md(nl), mi(nl);
    std::vector<unsigned long long> mc(nl);
    if (nl) {
        VLR_HIP_OK(hipMemcpy(md.data(), s->d_max_del, nl * 4, hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(mi.data(), s->d_max_ins, nl * 4, hipMemcpyDeviceToHost));
        VLR_HIP_OK(hipMemcpy(mc.data(), s->d_max_clip, nl * 8, hipMemcpyDeviceToHost));
    }
    for (size_t k = 0; k < nl; ++k) s->locusx[k] = vlr_fragpileup_indel_locus{md[k], mi[k], (uint32_t)(mc[k] >> 32), (uint32_t)(mc[k] & 0xffffffffull)};
    return VLR_OK;
}

}  // namespace vlr_fp

namespace vlr_fp {

// what vlr_fragpileup_open_realign gives beyond vlr_fragpileup_open
struct RealignOpen { const char* fasta; int window; vlr_ip::ScoreParams score; int64_t evidence_capacity, pair_byte_limit; };
// what vlr_fragpileup_open_indel gives beyond that: the loci's alt allele windows lie at alt_bases[alt_offset[k] .. alt_offset[k + 1])
struct IndelOpen { const uint64_t* alt_offset; int has_insert_size; };

// the deletion / insertion loci of an indel session: kind, interval, order, the limits; base_off = alt_offset
int check_indel_loci(const char* api, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int32_t* len, const uint8_t* kind, const uint64_t* alt_offset,
                     int realign_window, std::vector<uint64_t>& base_off, int64_t* max_locus_len, uint64_t* max_alt_len) {
    const uint64_t alt_limit = (uint64_t)VLR_FRAGPILEUP_MAX_INDEL_LEN + 2ull * ((uint64_t)realign_window * 3 / 2);
    base_off.assign((size_t)n_loci + 1, 0);
    *max_locus_len = 1; *max_alt_len = 0;
    for (int64_t k = 0; k < n_loci; ++k) {
        if ((kind[k] != VLR_INDELPILEUP_DELETION && kind[k] != VLR_INDELPILEUP_INSERTION) || ref_id[k] < 0 || start[k] < 0 || len[k] < 1 ||
            (kind[k] == VLR_INDELPILEUP_INSERTION && len[k] != 1) || alt_offset[k + 1] < alt_offset[k] || (k == 0 && alt_offset[0] != 0))
            return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: locus %lld: kind %d over %d bases (a deletion or an insertion; an insertion has 1), or its alt window's offsets", api,
                         (long long)k, (int)kind[k], (int)len[k]);
        if (len[k] > VLR_FRAGPILEUP_MAX_INDEL_LEN || alt_offset[k + 1] - alt_offset[k] > alt_limit)
            return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: locus %lld is %d bases long with an alt window of %llu: a session takes at most %d and %llu", api, (long long)k, (int)len[k],
                         (unsigned long long)(alt_offset[k + 1] - alt_offset[k]), VLR_FRAGPILEUP_MAX_INDEL_LEN, (unsigned long long)alt_limit);
        if (k > 0 && (ref_id[k] < ref_id[k - 1] || (ref_id[k] == ref_id[k - 1] && start[k] < start[k - 1])))
            return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: loci are not sorted by (ref_id, start) at %lld", api, (long long)k);
        base_off[(size_t)k + 1] = alt_offset[k + 1];
        *max_locus_len = std::max<int64_t>(*max_locus_len, len[k]);
        *max_alt_len = std::max<uint64_t>(*max_alt_len, alt_offset[k + 1] - alt_offset[k]);
    }
    return VLR_OK;
}

int open_impl(const char* api, int device, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int32_t* len, const uint8_t* kind, const uint8_t* ref_bases,
              const uint8_t* alt_bases, int realign_indel_reads, int64_t window, int max_mapq, int max_read_len, int64_t member_capacity, int64_t name_capacity,
              int64_t key_capacity, int64_t window_bytes, const RealignOpen* ro, vlr_fragpileup** out, const IndelOpen* io = nullptr, int meth_readtype = -1) {
    if (!out || n_loci < 0 || n_loci > 0x7fffffff || member_capacity < 0 || member_capacity > 0x7fffffff || name_capacity < 0 || key_capacity < 0 || key_capacity > 0x7fffffff ||
        window_bytes < 0 || window < 0 ||
        window > ((int64_t)1 << 40) || max_mapq < 0 || max_mapq > 255 || (n_loci > 0 && (!ref_id || !start || !len || !kind || !ref_bases || !alt_bases)))
        return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: bad argument", api);
    if (max_read_len <= 0) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: max_read_len must be positive", api);
    *out = nullptr;
    std::vector<uint64_t> base_off;
    int64_t max_locus_len = 0; uint64_t max_alt_len = 0;
    int rc = io != nullptr && ro != nullptr ? check_indel_loci(api, n_loci, ref_id, start, len, kind, io->alt_offset, ro->window, base_off, &max_locus_len, &max_alt_len)
                                            : vlr_bp::check_snv_mnv_loci(api, n_loci, ref_id, start, len, kind, base_off);
    if (rc != VLR_OK || (rc = vlr_bam::use_device(device)) != VLR_OK) return rc;
    vlr_fragpileup* s = new vlr_fragpileup();
    s->realign = realign_indel_reads ? 1 : 0;
    s->n_loci = n_loci;
    s->win = window;
    s->max_mapq = (uint32_t)max_mapq;
    s->member_cap = (uint64_t)member_capacity;
    s->name_cap = (uint64_t)name_capacity;
    s->key_cap = (uint64_t)key_capacity;
    s->coeff = 10ull * (uint64_t)max_read_len;
    s->locus_rec.assign((size_t)n_loci, vlr_fragpileup_locus{0, 0, 0, VLR_BASEPILEUP_NO_READ_POSITION, 0});
    const size_t nl = (size_t)n_loci;
    vlr_bam::Buffers& buf = s->buf;
    auto step = [&](int r) { if (rc == VLR_OK) rc = r; };
    if (ro != nullptr) {
        s->realigning = true;
        s->k_n = K_N_REALIGN;
        s->rl_window = ro->window;
        s->score = ro->score;
        s->h_ref_id.assign(ref_id, ref_id + n_loci);
        for (int64_t k = 0; k < n_loci; ++k) s->h_end.push_back(start[k] + (int64_t)len[k]);
        s->ctg.fasta = ro->fasta;
        s->ev_cap = (uint64_t)ro->evidence_capacity;
        if (ro->pair_byte_limit > 0 && (uint64_t)ro->pair_byte_limit < vlr_ip::kPairByteLimit) s->pair_byte_limit = (uint64_t)ro->pair_byte_limit;
        // an evidence's pairs: a ref window of at most 2 rw bases and an alt window of at most 2 rw + the locus; a read window of at most
        // 2 * window <= 128 bases, twice
        const uint64_t rw = (uint64_t)ro->window * 3 / 2;
        s->x_cap = s->ev_cap * (4 * rw + VLR_BASEPILEUP_MAX_LEN);
        if (io != nullptr) {   // an indel session: a ref window of at most 2 rw bases and the longest of the loci's own alt windows
            s->indel = true;
            s->has_insert_size = io->has_insert_size ? 1 : 0;
            s->max_locus_len = max_locus_len;
            s->x_cap = s->ev_cap * (2 * rw + max_alt_len);
            s->locusx.assign((size_t)n_loci, vlr_fragpileup_indel_locus{0, 0, 0, 0});
            step(buf.guarded(s->d_sides, (size_t)s->member_cap));
            step(buf.zeros(s->d_max_del, nl)); step(buf.zeros(s->d_max_ins, nl)); step(buf.zeros(s->d_max_clip, nl));
        }
        s->y_cap = s->ev_cap * 2 * (uint64_t)vlr_ip::kMaxPatternLen;
        step(vlr_bam::read_fai(s->ctg.fasta, s->ctg.fai));
        const size_t n_off = 2 * (size_t)s->ev_cap + 1;   // the pair offsets of the evidences and their end
        step(buf.guarded(s->d_ev, (size_t)s->ev_cap));
        step(buf.guarded(s->d_evm, (size_t)s->ev_cap));
        step(buf.guarded(s->d_gx, n_off));
        step(buf.guarded(s->d_gy, n_off));
        step(buf.guarded(s->d_xb, (size_t)s->x_cap));
        step(buf.guarded(s->d_yb, (size_t)s->y_cap));
        step(buf.guarded(s->d_yq, (size_t)s->y_cap));
        // offsets nobody wrote read as empty windows
        if (rc == VLR_OK && (hipMemset(s->d_gx, 0, n_off * 8) != hipSuccess || hipMemset(s->d_gy, 0, n_off * 8) != hipSuccess))
            rc = bfail(VLR_ERR_HIP, "%s: hipMemset of the pair offsets failed", api);
    }
    step(vlr_bam::open_session(*s, device, window_bytes, s->k_n));
    step(s->dl.upload(n_loci, ref_id, start, len, kind, base_off, ref_bases, alt_bases));
    step(buf.zeros(s->d_major_key, nl)); step(buf.zeros(s->d_have_key, nl));
    step(buf.zeros(s->d_lcnt, nl)); step(buf.zeros(s->d_cursor, nl)); step(buf.zeros(s->d_nobs, nl)); step(buf.zeros(s->d_major, nl)); step(buf.zeros(s->d_lstatus, nl));
    step(buf.zeros(s->d_loff, nl)); step(buf.zeros(s->d_obsoff, nl));
    step(buf.guarded(s->d_members, (size_t)s->member_cap));
    step(buf.guarded(s->d_names, (size_t)s->name_cap));
    step(buf.guarded(s->d_keys, (size_t)s->key_cap));
    if (meth_readtype >= 0) {   // a methylation session: the two tables of annotated reads, filled here with libm
        s->meth = true;
        std::vector<double> tab(512);
        fill_meth_tables(tab.data(), tab.data() + 256);
        step(buf.guarded(s->d_meth_tables, 512));
        if (rc == VLR_OK && hipMemcpy(s->d_meth_tables, tab.data(), 512 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            rc = bfail(VLR_ERR_HIP, "%s: hipMemcpy of the methylation tables failed", api);
        s->me = Meth{meth_readtype == VLR_METH_ANNOTATED ? 1 : 0, MethTables{s->d_meth_tables, s->d_meth_tables + 256}};
    }
    if (rc != VLR_OK) { vlr_fragpileup_close(s); return rc; }
    *out = s;
    return VLR_OK;
}

}  // namespace vlr_fp

extern "C" {

int vlr_fragpileup_open(int device, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int32_t* len, const uint8_t* kind,
                        const uint8_t* ref_bases, const uint8_t* alt_bases, int realign_indel_reads, int64_t window, int max_mapq, int max_read_len,
                        int64_t member_capacity, int64_t name_capacity, int64_t key_capacity, int64_t window_bytes, vlr_fragpileup** out) {
    return vlr_fp::open_impl("vlr_fragpileup_open", device, n_loci, ref_id, start, len, kind, ref_bases, alt_bases, realign_indel_reads, window, max_mapq, max_read_len,
                             member_capacity, name_capacity, key_capacity, window_bytes, nullptr, out);
}

int vlr_fragpileup_open_realign(int device, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int32_t* len, const uint8_t* kind,
                                const uint8_t* ref_bases, const uint8_t* alt_bases, int realign_indel_reads, int64_t window, int max_mapq,
                                int max_read_len, int64_t member_capacity, int64_t name_capacity, int64_t key_capacity, int64_t window_bytes, const char* fasta_path,
                                int realign_window, int mode, const double gap[4], const double* hop, int64_t evidence_capacity,
                                int64_t pair_byte_limit, vlr_fragpileup** out) {
    using namespace vlr_fp;
    if (!fasta_path || !gap || evidence_capacity < 0 || evidence_capacity > 0x7fffffff || pair_byte_limit < 0)
        return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_open_realign: bad argument");
    RealignOpen ro{fasta_path, realign_window, vlr_ip::ScoreParams(), evidence_capacity, pair_byte_limit};
    const int rc = vlr_ip::check_score_params("vlr_fragpileup_open_realign", realign_window, mode, gap, hop, ro.score);
    if (rc != VLR_OK) return rc;
    return open_impl("vlr_fragpileup_open_realign", device, n_loci, ref_id, start, len, kind, ref_bases, alt_bases, realign_indel_reads, window, max_mapq, max_read_len,
                     member_capacity, name_capacity, key_capacity, window_bytes, &ro, out);
}

int vlr_fragpileup_add_bam(vlr_fragpileup* s, const char* bam_path) {
    if (!s) return vlr_bam::bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_add_bam: null");
    std::function<int(const std::vector<std::string>&)> on_header;
    if (s->realigning) on_header = [s, bam_path](const std::vector<std::string>& names) { return vlr_fp::on_header(s, names, bam_path); };
    const int rc = vlr_bam::add_bam(*s, bam_path, "vlr_fragpileup_add_bam", {&s->t[0], &s->t[1], &s->t[2], &s->t[6], &s->t[5]}, on_header,
                                    [s](vlr_dev_file* df, int64_t n, hipStream_t st) { return vlr_fp::run_chunk(s, df, n, st); });
    // (vlr_fragpileup_set_alt_variants: a file that could not be added and gave no record does not count as the first one)
    if (rc == VLR_OK || s->n_records > 0) s->bam_added = true;
    return rc;
}

int vlr_fragpileup_result(vlr_fragpileup* s, vlr_fragpileup_counts* r) {
    using namespace vlr_fp;
    if (!s || !r) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_result: null");
    VLR_HIP_OK(hipSetDevice(s->device));
    if (!s->collected) {
        bool ok = true;
        int rc = vlr_bam::read_counters(*s);
        if (rc == VLR_OK) rc = s->buf.guards_intact(&ok);
        if (rc == VLR_OK && s->indel) rc = read_maxima(s);
        if (rc != VLR_OK) return rc;
        if (!ok) s->status |= VLR_FRAGPILEUP_GUARD_DAMAGED;
        if (vlr_bam::bad_record_seen(*s)) s->status |= VLR_FRAGPILEUP_BAD_RECORD;
        if (s->n_members > s->member_cap) s->status |= VLR_FRAGPILEUP_MEMBER_OVERFLOW;
        if (s->n_name_bytes > s->name_cap) s->status |= VLR_FRAGPILEUP_NAME_OVERFLOW;
        if (s->n_keys > s->key_cap) s->status |= VLR_FRAGPILEUP_KEY_OVERFLOW;
        if (s->ev_overflow) s->status |= VLR_FRAGPILEUP_EVIDENCE_OVERFLOW;
        if (!(s->status & (VLR_FRAGPILEUP_MEMBER_OVERFLOW | VLR_FRAGPILEUP_NAME_OVERFLOW | VLR_FRAGPILEUP_KEY_OVERFLOW | VLR_FRAGPILEUP_EVIDENCE_OVERFLOW | VLR_FRAGPILEUP_GUARD_DAMAGED)) &&
            s->n_members && s->n_loci) {
            if (s->realigning && s->n_ev && (rc = s->alt_set ? realign_pass_alt(s) : realign_pass(s)) != VLR_OK) return rc;
            if (s->status & VLR_FRAGPILEUP_GUARD_DAMAGED) { s->collected = true; return vlr_fragpileup_result(s, r); }
            const double t0 = now_s();
            rc = fragment_pass(s);
            if (rc != VLR_OK) return rc;
            s->t[4] += now_s() - t0 - s->t[7];
        }
        s->collected = true;
    }
    const bool over = (s->status & (VLR_FRAGPILEUP_MEMBER_OVERFLOW | VLR_FRAGPILEUP_NAME_OVERFLOW | VLR_FRAGPILEUP_KEY_OVERFLOW | VLR_FRAGPILEUP_EVIDENCE_OVERFLOW)) != 0;
    r->n_obs = (int64_t)s->obs.size();
    r->n_members = over ? 0 : (int64_t)s->n_members;
    r->n_records = (int64_t)s->n_records;
    r->n_rejected = (int64_t)s->counters[C_REJECTED];
    r->n_loci_too_deep = s->n_too_deep;
    r->status = s->status;
    r->needed_members = (int64_t)s->n_members;
    r->needed_name_bytes = (int64_t)s->n_name_bytes;
    r->needed_keys = (int64_t)s->n_keys;
    r->first_bad_record = vlr_bam::first_bad_record(*s);
    for (int k = 0; k < 8; ++k) r->seconds[k] = s->t[k];
    return VLR_OK;
}

int vlr_fragpileup_read(vlr_fragpileup* s, vlr_fragpileup_obs* obs, int64_t n_obs, vlr_fragpileup_locus* loci, int64_t n_loci) {
    using namespace vlr_fp;
    if (!s || !s->collected) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_read: call vlr_fragpileup_result first");
    if (n_obs != (int64_t)s->obs.size() || n_loci != s->n_loci || (n_obs > 0 && !obs) || (n_loci > 0 && !loci))
        return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_read: sizes differ from vlr_fragpileup_result and the loci given at open");
    if (n_obs) memcpy(obs, s->obs.data(), (size_t)n_obs * sizeof(vlr_fragpileup_obs));
    if (n_loci) memcpy(loci, s->locus_rec.data(), (size_t)n_loci * sizeof(vlr_fragpileup_locus));
    return VLR_OK;
}

int vlr_fragpileup_realign_result(vlr_fragpileup* s, vlr_fragpileup_realign_counts* r) {
    using namespace vlr_fp;
    if (!s || !r || !s->collected) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_realign_result: call vlr_fragpileup_result first");
    if (!s->realigning) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_realign_result: the session was not opened with vlr_fragpileup_open_realign");
    r->n_evidences = (int64_t)s->ev.size();
    r->needed_evidences = (int64_t)s->n_ev;
    r->x_bytes = s->ev_overflow ? 0 : (int64_t)s->x_total;
    r->y_bytes = s->ev_overflow ? 0 : (int64_t)s->y_total;
    r->n_ranges = s->n_ranges;
    for (int k = 0; k < 4; ++k) r->seconds[k] = s->rt[k];
    return VLR_OK;
}

int vlr_fragpileup_read_realigned(vlr_fragpileup* s, vlr_indelpileup_hit* hits, int64_t n) {
    using namespace vlr_fp;
    if (!s || !s->collected || !s->realigning) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_read_realigned: call vlr_fragpileup_result on a realigning session first");
    if (n != (int64_t)s->ev.size() || (n > 0 && !hits)) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_read_realigned: size differs from vlr_fragpileup_realign_result");
    if (n) memcpy(hits, s->ev.data(), (size_t)n * sizeof(vlr_indelpileup_hit));
    return VLR_OK;
}

int vlr_fragpileup_open_indel(int device, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int64_t* end, const uint8_t* kind,
                              const uint64_t* alt_offset, const uint8_t* alt_bases, int64_t window, int max_mapq, int max_read_len,
                              int64_t member_capacity, int64_t name_capacity, int64_t key_capacity, int64_t window_bytes, const char* fasta_path,
                              int realign_window, int mode, const double gap[4], const double* hop, int64_t evidence_capacity,
                              int64_t pair_byte_limit, int has_insert_size, vlr_fragpileup** out) {
    using namespace vlr_fp;
    if (!fasta_path || !gap || evidence_capacity < 0 || evidence_capacity > 0x7fffffff || pair_byte_limit < 0 || n_loci < 0 || n_loci > 0x7fffffff ||
        (n_loci > 0 && (!start || !end || !alt_offset || !alt_bases)))
        return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_open_indel: bad argument");
    RealignOpen ro{fasta_path, realign_window, vlr_ip::ScoreParams(), evidence_capacity, pair_byte_limit};
    const int rc = vlr_ip::check_score_params("vlr_fragpileup_open_indel", realign_window, mode, gap, hop, ro.score);
    if (rc != VLR_OK) return rc;
    // the loci as the session's tables hold them: len = end - start (the limit is checked on the 64-bit value)
    std::vector<int32_t> len((size_t)n_loci);
    for (int64_t k = 0; k < n_loci; ++k) {
        const int64_t l = end[k] - start[k];
        if (start[k] < 0 || l < 1 || l > VLR_FRAGPILEUP_MAX_INDEL_LEN)
            return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_open_indel: locus %lld [%lld, %lld) is empty or longer than the %d bases a session takes", (long long)k,
                         (long long)start[k], (long long)end[k], VLR_FRAGPILEUP_MAX_INDEL_LEN);
        len[(size_t)k] = (int32_t)l;
    }
    const IndelOpen io{alt_offset, has_insert_size};
    // (an indel session has no ref allele bytes: Loci::ref_bases is never read by an indel arm — base_off is the ALT offsets, so the alt windows
    // stand in for them rather than a null pointer.  Nothing may read ref_bases of such a session.)
    return open_impl("vlr_fragpileup_open_indel", device, n_loci, ref_id, start, len.data(), kind, alt_bases, alt_bases, 1, window, max_mapq, max_read_len,
                     member_capacity, name_capacity, key_capacity, window_bytes, &ro, out, &io);
}

int vlr_fragpileup_set_alt_variants(vlr_fragpileup* s, const uint64_t* comp_offset, const uint64_t* comp_base_offset, const uint8_t* comp_bases) {
    using namespace vlr_fp;
    const char* api = "vlr_fragpileup_set_alt_variants";
    if (!s || !comp_offset) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: null", api);
    if (!s->realigning) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: the session was not opened with vlr_fragpileup_open_realign or vlr_fragpileup_open_indel", api);
    if (s->alt_set) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: the session has its competitors already", api);
    if (s->bam_added) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: called after vlr_fragpileup_add_bam", api);
    // (the offsets are walked only as far as they proved ascending: check_table stops at the first entry that is not)
    const uint64_t limit = (uint64_t)VLR_FRAGPILEUP_MAX_INDEL_LEN + 2ull * ((uint64_t)s->rl_window * 3 / 2);
    if (comp_offset[0] != 0) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: comp_offset[0] is not 0", api);
    for (int64_t l = 0; l < s->n_loci; ++l) {
        if (comp_offset[l + 1] < comp_offset[l]) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: locus %lld: the competitor offsets descend", api, (long long)l);
        if (comp_offset[l + 1] - comp_offset[l] > (uint64_t)VLR_FRAGPILEUP_MAX_ALT_VARIANTS)
            return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: locus %lld has %llu competitors: a session takes at most %d", api, (long long)l,
                         (unsigned long long)(comp_offset[l + 1] - comp_offset[l]), VLR_FRAGPILEUP_MAX_ALT_VARIANTS);
    }
    const uint64_t n_comp = comp_offset[s->n_loci];
    if (n_comp > 0 && (!comp_base_offset || !comp_bases)) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: null", api);
    int64_t where = 0;
    const int bad = n_comp > 0 ? vlr_av::check_table(s->n_loci, comp_offset, comp_base_offset, limit, &where) : 0;
    if (bad == 3)
        return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: competitor %lld has a window of %llu bases: a session takes 1 .. %llu", api, (long long)where,
                     (unsigned long long)(comp_base_offset[where + 1] - comp_base_offset[where]), (unsigned long long)limit);
    if (bad) return bfail(VLR_ERR_INVALID_ARGUMENT, "%s: competitor %lld: the window offsets descend or do not start at 0", api, (long long)where);
    VLR_HIP_OK(hipSetDevice(s->device));
    std::vector<uint64_t> boff(1, 0);
    if (n_comp) boff.assign(comp_base_offset, comp_base_offset + n_comp + 1);
    const uint8_t none = 0;
    int rc;
    if ((rc = s->buf.upload(s->d_comp_off, comp_offset, (size_t)s->n_loci + 1)) != VLR_OK || (rc = s->buf.upload(s->d_comp_boff, boff.data(), boff.size())) != VLR_OK ||
        (rc = s->buf.upload(s->d_comp_bases, n_comp ? comp_bases : &none, n_comp ? (size_t)boff[n_comp] : 1)) != VLR_OK)
        return rc;
    s->h_comp_off.assign(comp_offset, comp_offset + s->n_loci + 1);
    s->h_comp_boff = boff;
    s->alt_limit = limit;
    for (int64_t l = 0; l < s->n_loci; ++l) if (comp_offset[l + 1] > comp_offset[l]) ++s->n_loci_with_comp;
    s->alt_set = true;
    return VLR_OK;
}

int vlr_fragpileup_alt_result(vlr_fragpileup* s, vlr_fragpileup_alt_counts* r) {
    using namespace vlr_fp;
    if (!s || !r || !s->collected || !s->alt_set) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_alt_result: call vlr_fragpileup_result on a session with vlr_fragpileup_set_alt_variants first");
    r->n_edit_pairs = s->n_edit_pairs;
    r->n_hmm_pairs = s->n_hmm_pairs;
    r->n_competitors = (int64_t)s->h_comp_off[(size_t)s->n_loci];
    r->n_loci_with_competitors = s->n_loci_with_comp;
    return VLR_OK;
}

int vlr_fragpileup_read_alt_variants(vlr_fragpileup* s, vlr_fragpileup_alt_hit* out, int64_t n) {
    using namespace vlr_fp;
    if (!s || !s->collected || !s->alt_set) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_read_alt_variants: call vlr_fragpileup_result on a session with vlr_fragpileup_set_alt_variants first");
    if (n != (int64_t)s->alt_hits.size() || (n > 0 && !out)) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_read_alt_variants: size differs from vlr_fragpileup_realign_result");
    if (n) memcpy(out, s->alt_hits.data(), (size_t)n * sizeof(vlr_fragpileup_alt_hit));
    return VLR_OK;
}

int vlr_fragpileup_read_indel(vlr_fragpileup* s, vlr_fragpileup_indel_obs* extra_obs, int64_t n_obs, vlr_fragpileup_indel_locus* extra_loci, int64_t n_loci) {
    using namespace vlr_fp;
    if (!s || !s->collected || !s->indel) return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_read_indel: call vlr_fragpileup_result on a session of vlr_fragpileup_open_indel first");
    if (n_obs != (int64_t)s->obsx.size() || n_loci != s->n_loci || (n_obs > 0 && !extra_obs) || (n_loci > 0 && !extra_loci))
        return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_read_indel: sizes differ from vlr_fragpileup_result and the loci given at open");
    if (n_obs) memcpy(extra_obs, s->obsx.data(), (size_t)n_obs * sizeof(vlr_fragpileup_indel_obs));
    if (n_loci) memcpy(extra_loci, s->locusx.data(), (size_t)n_loci * sizeof(vlr_fragpileup_indel_locus));
    return VLR_OK;
}

int vlr_fragpileup_open_methylation(int device, int64_t n_loci, const int32_t* ref_id, const int64_t* start, int readtype, int64_t window, int max_mapq,
                                    int max_read_len, int64_t member_capacity, int64_t name_capacity, int64_t key_capacity, int64_t window_bytes,
                                    vlr_fragpileup** out) {
    using namespace vlr_fp;
    if (n_loci < 0 || n_loci > 0x7fffffff || (n_loci > 0 && (!ref_id || !start)) || (readtype != VLR_METH_CONVERTED && readtype != VLR_METH_ANNOTATED))
        return bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_fragpileup_open_methylation: bad argument (readtype: VLR_METH_CONVERTED or VLR_METH_ANNOTATED)");
    // the loci as the session's tables hold them: one base each; kind and the allele bytes are never read by the methylation kernels
    const size_t nl = (size_t)n_loci;
    const std::vector<int32_t> len(nl, 1);
    const std::vector<uint8_t> kind(nl, (uint8_t)VLR_BASEPILEUP_SNV), bases(nl ? nl : 1, (uint8_t)'N');
    return open_impl("vlr_fragpileup_open_methylation", device, n_loci, ref_id, start, len.data(), kind.data(), bases.data(), bases.data(), 0, window, max_mapq, max_read_len,
                     member_capacity, name_capacity, key_capacity, window_bytes, nullptr, out, nullptr, readtype);
}

int vlr_methylation_tables(double ln_meth[256], double ln_unmeth[256]) {
    if (!ln_meth || !ln_unmeth) return vlr_bam::bfail(VLR_ERR_INVALID_ARGUMENT, "vlr_methylation_tables: null");
    vlr_fp::fill_meth_tables(ln_meth, ln_unmeth);
    return VLR_OK;
}

void vlr_fragpileup_close(vlr_fragpileup* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    vlr_bam::close_session(*s);
    s->dl.free();
    s->ctg.free();
    s->buf.free();
    if (s->d_src) (void)hipFree(s->d_src);
    delete s;
}

}  // extern "C"

