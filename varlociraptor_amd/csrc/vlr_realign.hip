// vlr_realign.hip — gfx950 kernels of the read-vs-allele pair HMM ("next" row #1): the producer of
// prob_alt / prob_ref in `varlociraptor preprocess variants`.
//
// What is computed: bio::stats::pairhmm::PairHMM::prob_related (third-party crate, restated in
// oracle/vlr_realign_oracle.cpp — see its header for what is and is not pinned) over the reference's emission model
//   ReadVsAlleleEmission / ReadEmission        /root/reference/src/variants/evidence/realignment/pairhmm.rs:296-455
//   GapParams, semiglobal start/end            pairhmm.rs:119-205
//   band = edit distance of the hit + EDIT_BAND realignment/mod.rs:519-537, pairhmm.rs:20
// for a batch of (allele window x, read window y) pairs.
//
// How: one wave64 per pair, anti-diagonal wavefront.  Lane l owns read rows 2l and 2l+1 (the reference limits a read window
// to 128 bases, EditDistanceCalculation::max_pattern_len, edit_distance.rs:145-147); at step d a row j works on column
// i = d - j.  The three forward states and the running minimum edit distance of a cell live in registers; a row needs the
// previous step's cell of the row above (wave_shr:1 DPP shift, or its own lane's other register), which one step later is
// its top-left neighbour — no LDS, no barriers.  Arithmetic is linear-space f64 (the reference works in log space): a cell
// costs 3 multiplies + 4 FMAs instead of ~5 exp/log1p; every lane keeps a power-of-two scale for its two rows (rows deep in
// an unrelated read are hundreds of orders of magnitude below the first ones) that is aligned when neighbours exchange cells.
// No MFMA (a recurrence, not a contraction); HBM traffic is the two sequences and the qualities, a few hundred bytes per pair.
//
// How the file is organised: every piece exists once.
//   the wavefront    Window (a pair's sequences, the length check), Wave<PAIRS> (which lanes form a pair, the value of the lane
//                    above), AlleleStream (the allele bases travelling down the lanes), row_base / row_qual: all five kernels
//   the summing HMM  Emission (linear row constants), Scaled<NS> (the states that carry a lane's scale) with exchange / rescale /
//                    finish, in_band / band_dist and the step loop `forward`; a model supplies the states of one cell — ExactModel
//                    (3 states; vlr_realign_kernel, vlr_realign_kernel2), HomopolyModel (5 states; vlr_homopoly_kernel)
//   on the same wavefront, with their own cells: vlr_edit_kernel (integers), vlr_pathhmm_kernel (max-plus, log space)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/vlr.h"

namespace vlr {

// the batch (CSR over pairs): front part of the argument struct of every kernel
struct PairArgs {
    int64_t n_pairs;
    const uint32_t* x_offset;
    const uint8_t* x_bases;
    const uint32_t* y_offset;
    const uint8_t* y_bases;
};
struct RealignArgs : PairArgs {
    const uint8_t* y_quals;
    const int32_t* max_edit_dist;
    double pn, pnx, pny, pgx, pgy, pgxe, pgye;  // linear: P(no gap), P(leave x-gap), P(leave y-gap), gap opens, extends
    double* ln_prob;
};

__device__ __forceinline__ int up(int b) { return (b >= 'a' && b <= 'z') ? b - 32 : b; }

// ---- the wavefront -----------------------------------------------------------------------------------------------------
// value of lane l-1 (lane 0: zero — bound_ctrl supplies it, no copy of an edge value into the destination first)
__device__ __forceinline__ double shr1z(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// value of lane l-1 (lane 0: `edge`)
__device__ __forceinline__ unsigned shr1(unsigned v, unsigned edge) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)edge, (int)v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ double shr1d(double v, double edge) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(__double2loint(edge), lo, 0x138, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), hi, 0x138, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

constexpr unsigned kBig = 0x3fffffffu;  // "unreachable" edit distance (adding one cannot wrap)

// the sequences of one pair
struct Window {
    uint32_t x0, y0;
    int len_x, len_y;
    __device__ __forceinline__ bool scored() const { return !(len_y > 128 || len_y <= 0 || len_x <= 0); }
};
__device__ __forceinline__ Window window_of(const PairArgs& a, const int64_t pair) {
    Window w;
    w.x0 = a.x_offset[pair]; w.y0 = a.y_offset[pair];
    w.len_x = (int)(a.x_offset[pair + 1] - w.x0); w.len_y = (int)(a.y_offset[pair + 1] - w.y0);
    return w;
}
// the ln probability of a window that is not scored (true: lane 0 has written it): -inf for an empty sequence, NaN for a read
// window above 128 bases
__device__ __forceinline__ bool unscored(const Window& w, const int lane, double* ln_prob) {
    if (w.scored()) return false;
    if (lane == 0) *ln_prob = (w.len_x <= 0 || w.len_y <= 0) ? -__builtin_huge_val() : __builtin_nan("");
    return true;
}

// Which lanes work on a pair.  One pair per wave: all 64, lane l owns rows 2l and 2l+1.  Two pairs per wave: lanes 0-31 the
// first, lanes 32-63 the second; everything that is wave-uniform per pair with one pair (lengths, band, owner lane, step count)
// is per half, and the wave_shr:1 shifts cross the half boundary, so lane 32 takes the edge value instead of lane 31's.
template <int PAIRS>
struct Wave {
    static constexpr int kChunk = 64 / PAIRS;  // lanes of a pair = allele bases per load
    int half, hl;                              // which pair of the wave, lane within the pair
    bool edge;                                 // the lane of row 0 of its pair
    __device__ __forceinline__ explicit Wave(const int lane) : half(PAIRS == 2 ? lane >> 5 : 0), hl(PAIRS == 2 ? lane & 31 : lane), edge(hl == 0) {}
    // value of the lane above; the lane of row 0 gets `e` / zero
    __device__ __forceinline__ unsigned above(const unsigned v, const unsigned e) const {
        const unsigned s = shr1(v, e);
        return PAIRS == 2 ? (edge ? e : s) : s;
    }
    __device__ __forceinline__ double above(const double v, const double e) const {
        const double s = shr1d(v, e);
        return PAIRS == 2 ? (edge ? e : s) : s;
    }
    __device__ __forceinline__ double above(const double v) const {
        const double s = shr1z(v);
        return PAIRS == 2 ? (edge ? 0.0 : s) : s;
    }
    // steps of the wave: those of its longer pair
    __device__ __forceinline__ int steps(const int nsteps) const {
        if (PAIRS == 1) return nsteps;
        const int ns0 = __builtin_amdgcn_readlane(nsteps, 0), ns1 = __builtin_amdgcn_readlane(nsteps, 32);
        return ns0 > ns1 ? ns0 : ns1;
    }
};

// x bases travel with the wavefront: row 2l works on column d - 2l, row 2l+1 on the column row 2l had one step earlier, and
// row 2l's column is the one row 2(l-1)+1 had one step earlier.  So every base is loaded once (one per lane of the pair at a
// time, lane-contiguous), enters at the lane of row 0 and moves down the lanes by one DPP shift per step; columns outside the
// allele carry 0.  b0 / b1: the bases of the columns the lane's two rows work on.
template <int PAIRS>
struct AlleleStream {
    const uint8_t* x_bases;
    uint32_t x0;
    int len_x;
    int chunk = 0, b0 = 0, b1 = 0;
    __device__ __forceinline__ AlleleStream(const PairArgs& a, const Window& w) : x_bases(a.x_bases), x0(w.x0), len_x(w.len_x) {}
    __device__ __forceinline__ void advance(const Wave<PAIRS>& w, const int d) {
        constexpr int kMask = Wave<PAIRS>::kChunk - 1;
        if ((d & kMask) == 0) {
            const int i = d + w.hl;
            chunk = (i < len_x) ? up(x_bases[x0 + i]) : 0;
        }
        int xnew = __builtin_amdgcn_readlane(chunk, d & kMask);
        if (PAIRS == 2) {
            const int xn1 = __builtin_amdgcn_readlane(chunk, 32 + (d & kMask));
            xnew = w.half ? xn1 : xnew;
        }
        const int prev1 = b1;
        b1 = b0;
        b0 = (int)w.above((unsigned)prev1 /* lane l-1's row-1 base of the previous step */, (unsigned)xnew);
    }
};

// base (upper case) and quality of read row j; rows beyond the read: 0
__device__ __forceinline__ int row_base(const PairArgs& a, const Window& w, const int j) { return j < w.len_y ? up(a.y_bases[w.y0 + j]) : 0; }
__device__ __forceinline__ int row_qual(const uint8_t* y_quals, const Window& w, const int j) { return j < w.len_y ? y_quals[w.y0 + j] : 0; }
__device__ __forceinline__ double ln_miscall(const int q) { return -(double)q * 2.302585092994046 / 10.0; }  // P(miscall) = 10^(-q/10)

// ---- the summing pair HMM ----------------------------------------------------------------------------------------------
// per-row emission constants (ReadEmission::new, pairhmm.rs:406-428; PROB_CONFUSION pairhmm.rs:22-24).  Rows beyond the
// read get zero emissions: every state of such a row stays exactly zero without a select in the loop.
struct Emission {
    int yb[2];
    double match[2], mis[2], ins[2];
};
__device__ __forceinline__ Emission emission_rows(const RealignArgs& a, const Window& w, const int hl) {
    Emission e;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j = 2 * hl + r;
        const bool rowon = j < w.len_y;
        e.yb[r] = row_base(a, w, j);
        const double mis = exp(ln_miscall(row_qual(a.y_quals, w, j)));
        e.match[r] = rowon ? 1.0 - mis : 0.0;
        e.mis[r] = rowon ? mis * 0.3333 : 0.0;
        e.ins[r] = rowon ? mis : 0.0;
    }
    return e;
}

// Scaling.  Every lane stores its states and its total with a factor 2^scale of its own: rows deep in the read carry far
// smaller numbers than the first rows.
//   * own states only shrink from step to step (every factor of the recurrence is at most one), by at most 2^-50 per step for
//     qualities up to 93 (a gap open times the insertion emission; a Q93 mismatch is 2^-35): the check every 8 steps (`rescale`),
//     which brings a lane whose largest state left 2^+-200 back to ~1, keeps them above 2^-600;
//   * what can GROW is what the lane above hands down: deep rows of a read swing by hundreds of binary orders between adjacent
//     columns, and a lane that has just brought tiny lead-in cells up to ~1 may be handed the bulk, 2^1000 and more above them,
//     at the next step.  So the exchange looks at what arrives BEFORE it is multiplied: if it would land above 2^200 in this
//     lane's units the lane lowers its own scale first so that it lands at ~1 (its own states, then more than 200 binary
//     orders below, keep their exact values or, beyond the range of f64, are flushed to zero).
// With that no state exceeds ~2^203 and nothing that carries weight falls below 2^-600: no overflow, no NaN, for read windows
// of up to 128 bases and qualities up to 93 (include/vlr.h).  All factors are powers of two, so scaling never rounds.  Every
// per-lane decision depends on the lane's own values alone (never on what the wave-wide ballots say), so two pairs per wave
// give the bits of one pair per wave.
constexpr int kScaleHi = 200;
// exponent by which a lane lowers its scale before it takes `mi` (largest incoming state, in the units of the lane above) times 2^dsc
__device__ __forceinline__ int incoming_excess(double mi, int dsc) {
    int ei = 0;
    (void)__builtin_frexp(mi, &ei);
    const int ein = ei + dsc;
    return (mi > 0.0 && dsc != 0 && ein > kScaleHi) ? ein : 0;
}
// 2^-e for the lane's own states: exactly zero once they would leave the range of f64
__device__ __forceinline__ double down_factor(int e) { return __builtin_ldexp(1.0, e > 1100 ? -1100 : -e); }
// factor for incoming states: finite for empty input of any scale difference, zero for what lies 2^1100 below this lane
__device__ __forceinline__ double align_factor(int dsc) { return __builtin_ldexp(1.0, dsc > 1000 ? 1000 : dsc < -1100 ? -1100 : dsc); }

enum { kM, kX, kY, kP, kQ };  // states of a cell: match, gap in y (x_i alone), gap in x (y_j alone); homopolymer model: HopY, HopX

// what of a lane carries its scale: NS states for each of its two rows, twice, and the sum of the last row
template <int NS>
struct Scaled {
    double left[NS][2];  // the cell each row computed at the previous step (its "left" neighbour now) ...
    double diag[NS][2];  // ... and of the row above one step earlier (the "top-left" neighbour now)
    double total = 0.0;  // sum over columns of the last row's states (free end gap in x)
    int scale = 0;       // all of the above carry a factor 2^scale
    __device__ __forceinline__ Scaled() {
#pragma unroll
        for (int k = 0; k < NS; ++k) { left[k][0] = left[k][1] = 0.0; diag[k][0] = diag[k][1] = 0.0; }
    }
    __device__ __forceinline__ void times(const double f) {
#pragma unroll
        for (int k = 0; k < NS; ++k) { left[k][0] *= f; left[k][1] *= f; diag[k][0] *= f; diag[k][1] *= f; }
        total *= f;
    }
};

// `top` [.][0] holds the previous step's cells of the last row of the lane above, stored with that lane's power-of-two scale:
// bring them to this lane's.  A lane that holds nothing yet (rows not reached, or everything outside the band) simply adopts the
// scale of the lane above.  Skipped altogether while all lanes agree (the common case: scales only move in `rescale`).
template <int PAIRS, int NS>
__device__ __forceinline__ void exchange(Scaled<NS>& s, const Wave<PAIRS>& w, double (&top)[NS][2]) {
    const int nb = (int)w.above((unsigned)s.scale, (unsigned)s.scale);
    if (__ballot(s.scale != nb)) {
        double mass = s.total, mi = top[0][0];
#pragma unroll
        for (int k = 0; k < NS; ++k) mass += (s.left[k][0] + s.left[k][1]) + (s.diag[k][0] + s.diag[k][1]);
#pragma unroll
        for (int k = 1; k < NS; ++k) mi = fmax(mi, top[k][0]);
        if (mass == 0.0) s.scale = nb;
        int dsc = s.scale - nb;
        const int over = incoming_excess(mi, dsc);
        if (over) {  // (per lane) make room for what arrives
            s.times(down_factor(over));
            s.scale -= over; dsc -= over;
        }
        const double f = align_factor(dsc);
#pragma unroll
        for (int k = 0; k < NS; ++k) top[k][0] *= f;
    }
}

// underflow guard, every 8 steps: a lane's own states shrink by at most 2^-50 per step (see kScaleHi above), 2^-400
// between two checks.  When the lane's largest state has left 2^+-200 it is brought back to ~1 (exact), unless what the
// lane has collected for the result already outweighs anything its states can still add.  Growth between two checks
// comes only from the lane above and is handled where it arrives (the exchange), not here.
template <int NS>
__device__ __forceinline__ void rescale(Scaled<NS>& s, const int d) {
    if ((d & 7) != 7) return;
    double mx = fmax(fmax(s.left[0][0], s.left[0][1]), fmax(s.diag[0][0], s.diag[0][1]));
#pragma unroll
    for (int k = 1; k < NS; ++k) mx = fmax(mx, fmax(fmax(s.left[k][0], s.left[k][1]), fmax(s.diag[k][0], s.diag[k][1])));
    int ex = 0;
    (void)__builtin_frexp(mx, &ex);
    // (scaled DOWN as well: the mass of a lane grows again when the wavefront reaches the columns the read aligns to)
    const bool resc = mx > 0.0 && (ex > 200 || (ex < -200 && !(s.total > mx * 0x1p60)));
    if (__ballot(resc)) {
        const int sh0 = -ex > 1000 ? 1000 : -ex < -1000 ? -1000 : -ex;
        const int sh = resc ? sh0 : 0;
        s.times(__builtin_ldexp(1.0, sh));
        s.scale += sh;
    }
}

// the lane that owns the last row holds the sum
template <int PAIRS, int NS>
__device__ __forceinline__ void finish(const Scaled<NS>& s, const Wave<PAIRS>& w, const int last_row, double* ln_prob) {
    const int owner = 32 * w.half + (last_row >> 1);
    const double total = __shfl(s.total, owner);
    const int scale = __shfl(s.scale, owner);
    if (w.edge) {
        const double p = (total > 0.0) ? log(total) - (double)scale * 0.6931471805599453 : -__builtin_huge_val();
        *ln_prob = p > 0.0 ? 0.0 : p;  // "sum of paths can exceed probability 1.0"
    }
}

// The band: a cell is kept while the smallest running minimum edit distance of its top-left, top and left neighbours is within
// the pair's bound ...
__device__ __forceinline__ bool in_band(const int med_max, const unsigned etl, const unsigned eu, const unsigned el) {
    return !(min(etl, min(eu, el)) > (unsigned)med_max);
}
// ... and then has this running minimum itself
__device__ __forceinline__ unsigned band_dist(const bool is_match, const unsigned etl, const unsigned eu, const unsigned el) {
    return min(min(is_match ? etl : etl + 1u, min(eu + 1u, el + 1u)), kBig);
}

// one row of a lane at one step: row r of the lane on column i; `start`: its top-left neighbour is the virtual start row
struct Row {
    int r, i;
    bool is_match, start;
};

// A model gives the states of one cell.  cell(row, em, s, top, c): c[] <- the states of the lane's row from its top-left (s.diag),
// left (s.left) and top (`top`) neighbours: cells outside the matrix are exactly zero by construction (rows start from zero
// states, the row above is zero before its first column).  enter_column(b): the lane's row 0 moves on to a column of base b, its
// row 1 to the column row 0 had.  sum(c): what a cell of the last row adds to the result.
struct ExactModel {
    static constexpr int NS = 3;
    const RealignArgs& a;
    __device__ __forceinline__ void enter_column(int) {}
    __device__ __forceinline__ void cell(const Row& row, const Emission& em, const Scaled<NS>& s, const double (&top)[NS][2], double (&c)[NS]) const {
        const int r = row.r;
        const double emit = row.is_match ? em.match[r] : em.mis[r];
        c[kM] = emit * (a.pn * s.diag[kM][r] + a.pny * s.diag[kX][r] + a.pnx * s.diag[kY][r]);
        c[kX] = a.pgy * s.left[kM][r] + a.pgye * s.left[kX][r];        // gap in y: x_i alone (prob_emit_x = 1)
        c[kY] = em.ins[r] * (a.pgx * top[kM][r] + a.pgxe * top[kY][r]);  // gap in x: y_j alone
    }
    __device__ __forceinline__ static double sum(const double (&c)[NS]) { return (c[kM] + c[kX]) + c[kY]; }
};

// One pair on the lanes of `w`: the step loop of the summing kernels.
template <int PAIRS, class Model>
__device__ __forceinline__ void forward(const RealignArgs& a, Model model, const Wave<PAIRS>& w, const Window& win, const int64_t pair) {
    constexpr int NS = Model::NS;
    const int med_max = a.max_edit_dist ? a.max_edit_dist[pair] : -1;
    const bool banded = med_max >= 0;
    const Emission em = emission_rows(a, win, w.hl);
    Scaled<NS> s;
    unsigned E1[2] = {kBig, kBig}, Et[2] = {kBig, kBig};  // running minimum edit distance of the cells of s.left, s.diag
    const int last_row = win.len_y - 1;
    const int lr = last_row & 1;             // which of its two rows the owner lane sums (uniform per pair)
    const bool owner_lane = w.hl == (last_row >> 1);
    const int nsteps = w.steps(win.len_x + win.len_y - 1);
    AlleleStream<PAIRS> xs(a, win);
    for (int d = 0; d < nsteps; ++d) {
        xs.advance(w, d);
        model.enter_column(xs.b0);
        // top neighbour = previous step's cell of row j-1.  Row -1 is the virtual start row: as "top" (same column) it is
        // empty, as "top-left" (previous column) it carries the free start mass one with edit distance zero.
        double top[NS][2];
        unsigned Eu[2];
#pragma unroll
        for (int k = 0; k < NS; ++k) top[k][0] = w.above(s.left[k][1]);
        Eu[0] = w.above(E1[1], kBig);
        exchange(s, w, top);
#pragma unroll
        for (int k = 0; k < NS; ++k) top[k][1] = s.left[k][0];
        Eu[1] = E1[0];
        // virtual start row: the top-left neighbour of row 0 holds mass one in every column (free start gap in x)
        if (w.edge) { s.diag[kM][0] = __builtin_ldexp(1.0, s.scale); Et[0] = 0u; }
        double n[NS][2], last = 0.0;
        unsigned En[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const Row row = {r, d - (2 * w.hl + r), (r == 0 ? xs.b0 : xs.b1) == em.yb[r], r == 0 && w.edge};
            // beyond the last column and outside the band a row keeps nothing.  A branch, not selects: a wave skips the cells of a
            // row that is live in none of its lanes (the last steps of a banded pair)
            const bool incol = (unsigned)row.i < (unsigned)win.len_x;
            double c[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) c[k] = 0.0;
            En[r] = kBig;
            if constexpr (PAIRS == 1) {  // `banded` is uniform: the band has a branch of its own
                bool live = incol;
                if (banded) {
                    live = incol && in_band(med_max, Et[r], Eu[r], E1[r]);
                    En[r] = live ? band_dist(row.is_match, Et[r], Eu[r], E1[r]) : kBig;
                }
                if (live) model.cell(row, em, s, top, c);
            } else {  // `banded` differs between the halves: one branch for the band's integers and the cell
                const bool inside = in_band(med_max, Et[r], Eu[r], E1[r]);
                if (incol && (!banded || inside)) {
                    En[r] = banded ? band_dist(row.is_match, Et[r], Eu[r], E1[r]) : kBig;
                    model.cell(row, em, s, top, c);
                }
            }
#pragma unroll
            for (int k = 0; k < NS; ++k) n[k][r] = c[k];
            if (r == lr) last = Model::sum(c);
        }
        s.total += owner_lane ? last : 0.0;  // (zero outside the columns of the allele)
        // this step's "top" of a row is its "top-left" at the next step
#pragma unroll
        for (int k = 0; k < NS; ++k) { s.diag[k][0] = top[k][0]; s.diag[k][1] = top[k][1]; s.left[k][0] = n[k][0]; s.left[k][1] = n[k][1]; }
#pragma unroll
        for (int r = 0; r < 2; ++r) { Et[r] = Eu[r]; E1[r] = En[r]; }
        rescale(s, d);
    }
    finish(s, w, last_row, &a.ln_prob[pair]);
}

// one pair per wave, and the length check that goes with it
template <class Model>
__device__ __forceinline__ void forward_one(const RealignArgs& a, const Model& model, const int64_t pair, const Window& win, const int lane) {
    if (unscored(win, lane, &a.ln_prob[pair])) return;
    forward(a, model, Wave<1>(lane), win, pair);
}

__global__ void __launch_bounds__(64) vlr_realign_kernel(RealignArgs a) {
    const int64_t pair = blockIdx.x;
    if (pair >= a.n_pairs) return;
    forward_one(a, ExactModel{a}, pair, window_of(a, pair), threadIdx.x);
}

// Two pairs per wave: a read window of at most 64 bases occupies 32 lanes.  Workgroup w takes the pairs 2w and 2w + 1 — the
// reference and the alt allele of one read are adjacent in a batch and share the read window — and, when both windows are
// short, runs them side by side (Wave<2>).  Same arithmetic per cell in the same order: results are bit-identical to the
// one-pair kernel, which VLR_REALIGN_SINGLE selects (compared in tests/test_gpu_realign_guard.py).
__global__ void __launch_bounds__(64) vlr_realign_kernel2(RealignArgs a) {
    const int64_t pair0 = 2 * (int64_t)blockIdx.x;
    if (pair0 >= a.n_pairs) return;
    const int lane = threadIdx.x;
    const bool have2 = pair0 + 1 < a.n_pairs;
    const Window w0 = window_of(a, pair0);
    const Window w1 = have2 ? window_of(a, pair0 + 1) : Window{0u, 0u, 0, 0};
    if (!(have2 && w0.scored() && w1.scored() && w0.len_y <= 64 && w1.len_y <= 64)) {  // (uniform) one after the other
        forward_one(a, ExactModel{a}, pair0, w0, lane);
        if (have2) forward_one(a, ExactModel{a}, pair0 + 1, w1, lane);
        return;
    }
    const Wave<2> w(lane);
    forward(a, ExactModel{a}, w, w.half ? w1 : w0, pair0 + w.half);
}

// ---- `homopolymer` realignment mode --------------------------------------------------------------------------------------
// HomopolyPairHMMRealigner::calculate_prob_allele (realignment/mod.rs:680-730): bio's HomopolyPairHMM::prob_related with the
// reference's HopParams (pairhmm.rs:207-295) — the pair HMM above plus, per base, hop states that emit one more copy of the
// homopolymer base in the read (HopX_b: y_j == b alone, emitted like a matching base — oracle/vlr_realign_oracle.cpp says on which
// evidence) or in the allele (HopY_b: x_i == b alone), entered from the match state of
// the same base and left to a match state only.  Restated in oracle/vlr_realign_oracle.cpp (vlro_homopoly_prob_related, PARITY
// UNPINNED: the recursion lives in the un-vendored crate bio) with all fourteen states spelled out; here the model is folded:
// the match state of a cell is the one of its allele base x_i, so of the four HopX_b / HopY_b / Match_b at most one each is
// non-zero per cell — HopX needs y_j == x_i, HopY needs x_i == x_{i-1} — and a cell carries five values {M, X, Y, P, Q}
// (X = x_i alone after a gap open, Y = y_j alone, P = HopY, Q = HopX).  The transition out of a match or hop state depends on the
// base of the PREVIOUS column (1 - (gap_x + gap_y + hop_x(b') + hop_y(b')), 1 - hop_extend(b')): the per-base constants sit in a
// 5 x 8 table in LDS (row 4: any other base, no hops), row 0 of a lane looks up the base entering its column, row 1 inherits
// what row 0 held one step earlier.  Same wavefront, scaling and band as the exact model (`forward`); one pair per wave only.
struct HomopolyArgs {
    RealignArgs r;
    double hx[4], hy[4], hxe[4], hye[4];  // linear: start / extend a homopolymer run in the read (x gap) / in the allele (y gap)
};
__device__ __forceinline__ int base_index(int b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4; }

struct HomopolyModel {
    static constexpr int NS = 5;
    const RealignArgs& a;
    const double (*tab)[8];  // {hop_x, hop_y, hop_x_extend, hop_y_extend, match->match, leave hop x, leave hop y, -} per base
    // per-base constants of the column each row works on (c*) and of the column before it (p*: what the top-left cell leaves with)
    double chx[2] = {0.0, 0.0}, chy[2] = {0.0, 0.0}, chxe[2] = {0.0, 0.0}, chye[2] = {0.0, 0.0};
    double ctm[2], clx[2] = {1.0, 1.0}, cly[2] = {1.0, 1.0};
    double ptm[2], plx[2] = {1.0, 1.0}, ply[2] = {1.0, 1.0};
    int xc[2] = {0, 0}, xp[2] = {0, 0};  // the bases of those two columns
    __device__ __forceinline__ HomopolyModel(const RealignArgs& a_, const double (*tab_)[8]) : a(a_), tab(tab_) { ctm[0] = ctm[1] = ptm[0] = ptm[1] = a.pn; }
    // constants: row 1 inherits row 0's of the previous step (same column), row 0 looks its new base up
    __device__ __forceinline__ void enter_column(const int b) {
        xp[1] = xc[1]; xp[0] = xc[0]; xc[1] = xc[0]; xc[0] = b;
        ptm[1] = ctm[1]; plx[1] = clx[1]; ply[1] = cly[1];
        chx[1] = chx[0]; chy[1] = chy[0]; chxe[1] = chxe[0]; chye[1] = chye[0]; ctm[1] = ctm[0]; clx[1] = clx[0]; cly[1] = cly[0];
        ptm[0] = ctm[0]; plx[0] = clx[0]; ply[0] = cly[0];
        const double* t = tab[base_index(b)];
        chx[0] = t[0]; chy[0] = t[1]; chxe[0] = t[2]; chye[0] = t[3]; ctm[0] = t[4]; clx[0] = t[5]; cly[0] = t[6];
    }
    __device__ __forceinline__ void cell(const Row& row, const Emission& em, const Scaled<NS>& s, const double (&top)[NS][2], double (&c)[NS]) const {
        const int r = row.r;
        const bool is_match = row.is_match, run = xc[r] == xp[r] && row.i > 0;  // run: x_i == x_{i-1}
        const double emit = is_match ? em.match[r] : em.mis[r];
        const double tm = row.start ? a.pn : ptm[r];  // the virtual start row is left with 1 - (gap_x + gap_y)
        c[kM] = emit * ((tm * s.diag[kM][r] + a.pny * s.diag[kX][r] + a.pnx * s.diag[kY][r]) + (ply[r] * s.diag[kP][r] + plx[r] * s.diag[kQ][r]));
        c[kX] = a.pgy * s.left[kM][r] + a.pgye * s.left[kX][r];
        c[kY] = em.ins[r] * (a.pgx * top[kM][r] + a.pgxe * top[kY][r]);
        c[kP] = run ? chy[r] * s.left[kM][r] + chye[r] * s.left[kP][r] : 0.0;                           // x_i == x_{i-1} alone
        c[kQ] = is_match ? em.match[r] * (chx[r] * top[kM][r] + chxe[r] * top[kQ][r]) : 0.0;           // y_j == x_i alone, emitted like a matching base
    }
    __device__ __forceinline__ static double sum(const double (&c)[NS]) { return ((c[kM] + c[kX]) + c[kY]) + (c[kP] + c[kQ]); }
};

__global__ void __launch_bounds__(64) vlr_homopoly_kernel(HomopolyArgs h) {
    const RealignArgs& a = h.r;
    const int64_t pair = blockIdx.x;
    if (pair >= a.n_pairs) return;
    const int lane = threadIdx.x;
    __shared__ double tab[5][8];
    if (lane < 5) {
        const bool acgt = lane < 4;
        const int b = acgt ? lane : 0;
        const double hx = acgt ? h.hx[b] : 0.0, hy = acgt ? h.hy[b] : 0.0, hxe = acgt ? h.hxe[b] : 0.0, hye = acgt ? h.hye[b] : 0.0;
        tab[lane][0] = hx; tab[lane][1] = hy; tab[lane][2] = hxe; tab[lane][3] = hye;
        tab[lane][4] = 1.0 - (((a.pgx + a.pgy) + hx) + hy);
        tab[lane][5] = 1.0 - hxe; tab[lane][6] = 1.0 - hye; tab[lane][7] = 0.0;
    }
    __syncthreads();
    forward_one(a, HomopolyModel(a, tab), pair, window_of(a, pair), lane);
}

// ---- edit-distance pre-filter ----------------------------------------------------------------------------------------
// EditDistanceCalculation::calc_best_hit (edit_distance.rs:164-260; bio Myers `find_all_lazy`): the smallest semiglobal edit
// distance of the read window against the allele window (free start and end in the allele), the first allele position at
// which an alignment with that distance ends, and the number of such end positions.  The pair HMM is banded to
// distance + EDIT_BAND (realignment/mod.rs:519-537).  Same wavefront as the pair HMM, integers only: lane l owns rows 2l and
// 2l+1, a cell is min(top-left + mismatch, top + 1, left + 1); row -1 is all zero (free start), column -1 of row j is j + 1.
struct EditArgs : PairArgs {
    int32_t* dist;
    int32_t* end;
    int32_t* n_hits;
};

__global__ void __launch_bounds__(64) vlr_edit_kernel(EditArgs a) {
    const int64_t pair = blockIdx.x;
    if (pair >= a.n_pairs) return;
    const int lane = threadIdx.x;
    const Wave<1> w(lane);
    const Window win = window_of(a, pair);
    const int len_x = win.len_x;
    if (!win.scored()) {
        if (lane == 0) { a.dist[pair] = -1; if (a.end) a.end[pair] = -1; if (a.n_hits) a.n_hits[pair] = 0; }
        return;
    }
    int yb[2];
    unsigned E1[2], Et[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j = 2 * lane + r;
        yb[r] = row_base(a, win, j);
        E1[r] = (unsigned)(j + 1);  // the cell left of column 0 of row j
        Et[r] = (unsigned)j;        // (j-1, -1)
    }
    const int last_row = win.len_y - 1;
    const int lr = last_row & 1;
    const bool owner_lane = lane == (last_row >> 1);
    unsigned best = kBig;
    int best_end = 0, nbest = 0;
    const int nsteps = len_x + win.len_y - 1;
    AlleleStream<1> xs(a, win);
    for (int d = 0; d < nsteps; ++d) {
        xs.advance(w, d);
        unsigned Eu[2];
        Eu[0] = w.above(E1[1], 0u);  // row -1 for lane 0: zero in every column
        Eu[1] = E1[0];
        if (lane == 0) Et[0] = 0u;
        unsigned En[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = d - (2 * lane + r);
            const bool incol = (unsigned)i < (unsigned)len_x;
            const int xb = r == 0 ? xs.b0 : xs.b1;
            const unsigned e = min(Et[r] + (xb == yb[r] ? 0u : 1u), min(Eu[r], E1[r]) + 1u);
            En[r] = incol ? e : E1[r];  // before its first column a row keeps the value left of column 0
        }
        {
            const int i = d - last_row;
            const bool hit = owner_lane && (unsigned)i < (unsigned)len_x;
            const unsigned e = En[lr];
            if (hit && e < best) { best = e; best_end = i + 1; nbest = 0; }
            if (hit && e == best) nbest += 1;
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) { Et[r] = Eu[r]; E1[r] = En[r]; }
    }
    if (owner_lane) {
        a.dist[pair] = (int32_t)best;
        if (a.end) a.end[pair] = best_end;
        if (a.n_hits) a.n_hits[pair] = nbest;
    }
}

// ---- `fast` realignment mode -------------------------------------------------------------------------------------------
// PathHMMRealigner::calculate_prob_allele (realignment/mod.rs:547-678): instead of summing over all alignments, the path
// probability of the optimal edit-distance alignments of the best hits (bio Myers traceback, edit_distance.rs:164-260) — transition
// terms by the previous operation (no_gap / close_gap / gap open / extend-or-reopen, mod.rs:560-584), emissions of the
// ReadVsAlleleEmission model — and the best of them.  Which of several co-optimal alignments the crate's traceback returns is
// not specified by the reference; this kernel takes the BEST path probability over ALL alignments of minimal semiglobal edit
// distance (an upper bound of, and with a unique optimal alignment equal to, the reference's value).
// Same wavefront as the pair HMM, in max-plus form over (edit distance, ln probability) pairs ordered lexicographically
// (smaller distance first, then larger probability) per state {match, deletion, insertion}: adds and compares only, log space,
// no scaling.  Cell (j, i) = read bases 0..j and allele bases ..i consumed; row -1 is the free start in every column.
struct PathArgs : PairArgs {
    const uint8_t* y_quals;
    double no_gap, close_x, close_y, gap_x, gap_y, reopen_x, reopen_y;  // ln; reopen_* = ln(extend + close * open) (mod.rs:576-584)
    double* ln_prob;
};
struct DP { unsigned d; double p; };
__device__ __forceinline__ DP dp_best(DP a, DP b) {
    const bool ta = (a.d < b.d) | ((a.d == b.d) & (a.p > b.p));
    DP r; r.d = ta ? a.d : b.d; r.p = ta ? a.p : b.p; return r;
}
__device__ __forceinline__ DP dp_step(DP a, unsigned cost, double lp) {  // unreachable stays unreachable
    DP r; r.d = a.d >= kBig ? kBig : a.d + cost; r.p = a.d >= kBig ? -__builtin_huge_val() : a.p + lp; return r;
}
__device__ __forceinline__ DP dp_above(const Wave<1>& w, DP v) { DP r; r.d = w.above(v.d, kBig); r.p = w.above(v.p, -__builtin_huge_val()); return r; }

__global__ void __launch_bounds__(64) vlr_pathhmm_kernel(PathArgs a) {
    const int64_t pair = blockIdx.x;
    if (pair >= a.n_pairs) return;
    const int lane = threadIdx.x;
    const Wave<1> w(lane);
    const Window win = window_of(a, pair);
    const int len_x = win.len_x;
    const double NINF = -__builtin_huge_val();
    if (unscored(win, lane, &a.ln_prob[pair])) return;
    int yb[2];
    double l_match[2], l_mis[2], l_ins[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j = 2 * lane + r;
        yb[r] = row_base(a, win, j);
        const double lm = ln_miscall(row_qual(a.y_quals, win, j));  // ln P(miscall)
        l_ins[r] = lm;
        l_mis[r] = lm + log(0.3333);                               // PROB_CONFUSION, pairhmm.rs:22-24
        l_match[r] = (lm < -0.693) ? log1p(-exp(lm)) : log(-expm1(lm));
    }
    // column -1: read bases inserted before the first allele base — insertion chain from the start (prev None: gap_x, mod.rs:640-647)
    // pre[j] = gap_x + ins_0 + sum_{k=1..j} (reopen_x + ins_k): inclusive prefix sums over the rows (two per lane)
    double pre[2];
    {
        const double t0 = (lane == 0 ? a.gap_x : a.reopen_x) + l_ins[0], t1 = a.reopen_x + l_ins[1];
        double s = t0 + t1;  // lane sum
        double inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        const double excl = inc - s;
        pre[0] = excl + t0; pre[1] = excl + t0 + t1;
    }
    DP M1[2], D1[2], I1[2], Mt[2], Dt[2], It[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j = 2 * lane + r;
        M1[r] = {kBig, NINF}; D1[r] = {kBig, NINF};
        I1[r] = {(unsigned)(j + 1), pre[r]};                      // (j, -1)
        Mt[r] = {kBig, NINF}; Dt[r] = {kBig, NINF};
    }
    It[1] = {(unsigned)(2 * lane + 1), pre[0]};                   // (j-1, -1) of the lane's second row = its first row
    {
        const double up1 = __shfl_up(pre[1], 1);
        It[0] = {lane == 0 ? kBig : (unsigned)(2 * lane), lane == 0 ? NINF : up1};  // row 0: the start row, handled below
    }
    const int last_row = win.len_y - 1;
    const int lr = last_row & 1;
    const bool owner_lane = lane == (last_row >> 1);
    DP best = {kBig, NINF};
    const int nsteps = len_x + win.len_y - 1;
    AlleleStream<1> xs(a, win);
    for (int d = 0; d < nsteps; ++d) {
        xs.advance(w, d);
        DP Mu[2], Du[2], Iu[2];
        Mu[0] = dp_above(w, M1[1]); Du[0] = dp_above(w, D1[1]); Iu[0] = dp_above(w, I1[1]);
        Mu[1] = M1[0]; Du[1] = D1[0]; Iu[1] = I1[0];
        DP Mn[2], Dn[2], In[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int j = 2 * lane + r;
            const int i = d - j;
            const bool incol = (unsigned)i < (unsigned)len_x;
            const int xb = r == 0 ? xs.b0 : xs.b1;
            const bool is_match = xb == yb[r];
            const unsigned mm = is_match ? 0u : 1u;
            const double emit = is_match ? l_match[r] : l_mis[r];
            // match / substitution from (j-1, i-1)
            DP m = dp_best(dp_best(dp_step(Mt[r], mm, a.no_gap + emit), dp_step(Dt[r], mm, a.close_y + emit)), dp_step(It[r], mm, a.close_x + emit));
            // deletion (allele base alone, prob_emit_x = 1) from (j, i-1)
            DP dl = dp_best(dp_best(dp_step(M1[r], 1u, a.gap_y), dp_step(D1[r], 1u, a.reopen_y)), dp_step(I1[r], 1u, a.close_x + a.gap_y));
            // insertion (read base alone) from (j-1, i)
            DP in = dp_best(dp_best(dp_step(Mu[r], 1u, a.gap_x + l_ins[r]), dp_step(Iu[r], 1u, a.reopen_x + l_ins[r])), dp_step(Du[r], 1u, a.close_y + a.gap_x + l_ins[r]));
            if (j == 0) {  // the start row above row 0: first operation, no transition term (prev None, mod.rs:598-647)
                const DP sm = {mm, emit}, si = {1u, a.gap_x + l_ins[r]};
                m = dp_best(m, sm);
                in = dp_best(in, si);
            }
            const DP dead = {kBig, NINF};
            Mn[r] = incol ? m : dead; Dn[r] = incol ? dl : dead;
            In[r] = incol ? in : I1[r];  // before its first column a row keeps the insertion chain of column -1
            if (!incol && i >= len_x) In[r] = dead;
        }
        {
            const int i = d - last_row;
            const bool hit = owner_lane && (unsigned)i < (unsigned)len_x;
            const DP e = dp_best(Mn[lr], In[lr]);  // an optimal semiglobal alignment does not end in a deletion
            if (hit) best = dp_best(best, e);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) { Mt[r] = Mu[r]; Dt[r] = Du[r]; It[r] = Iu[r]; M1[r] = Mn[r]; D1[r] = Dn[r]; I1[r] = In[r]; }
    }
    if (owner_lane) a.ln_prob[pair] = best.d >= kBig ? NINF : best.p;
}

}  // namespace vlr

// ---- launchers -------------------------------------------------------------------------------------------------------------
static void set_pairs(vlr::PairArgs& a, const vlr_realign_batch_desc* b) {
    a.n_pairs = b->n_pairs; a.x_offset = b->x_offset; a.x_bases = b->x_bases; a.y_offset = b->y_offset; a.y_bases = b->y_bases;
}
// arguments of the summing kernels.  GapParamCache of the pair HMM: P(no gap) = 1 - (P(gap x) + P(gap y)); leaving a gap state:
// 1 - P(extend)
static void set_linear(vlr::RealignArgs& a, const vlr_realign_batch_desc* b, double* ln_prob) {
    set_pairs(a, b);
    a.y_quals = b->y_quals; a.max_edit_dist = b->max_edit_dist; a.ln_prob = ln_prob;
    const double gx = exp(b->gap[0]), gy = exp(b->gap[1]), gxe = exp(b->gap[2]), gye = exp(b->gap[3]);
    a.pgx = gx; a.pgy = gy; a.pgxe = gxe; a.pgye = gye;
    a.pn = fmax(0.0, 1.0 - (gx + gy)); a.pnx = 1.0 - gxe; a.pny = 1.0 - gye;  // (fmax: a legal sum of one may round to just above it)
}

extern "C" int vlr_launch_pathhmm_kernel(const vlr_realign_batch_desc* b, double* ln_prob, void* stream) {
    using namespace vlr;
    if (b->n_pairs <= 0) return 0;
    PathArgs a;
    set_pairs(a, b);
    a.y_quals = b->y_quals; a.ln_prob = ln_prob;
    // PathHMMRealigner::new (realignment/mod.rs:560-584)
    const double gx = exp(b->gap[0]), gy = exp(b->gap[1]), gxe = exp(b->gap[2]), gye = exp(b->gap[3]);
    a.gap_x = b->gap[0]; a.gap_y = b->gap[1];
    a.no_gap = log(fmax(0.0, 1.0 - (gx + gy)));
    a.close_x = log(1.0 - gxe); a.close_y = log(1.0 - gye);
    a.reopen_x = log(gxe + (1.0 - gxe) * gx); a.reopen_y = log(gye + (1.0 - gye) * gy);
    hipLaunchKernelGGL(vlr_pathhmm_kernel, dim3((unsigned)b->n_pairs), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// hop[16] = ln {hop_x[A,C,G,T] (prob_seq_homopolymer), hop_y[..] (prob_ref_homopolymer), hop_x_extend[..], hop_y_extend[..]}
extern "C" int vlr_launch_homopoly_kernel(const vlr_realign_batch_desc* b, const double* hop, double* ln_prob, void* stream) {
    using namespace vlr;
    if (b->n_pairs <= 0) return 0;
    HomopolyArgs h;
    set_linear(h.r, b, ln_prob);
    for (int k = 0; k < 4; ++k) { h.hx[k] = exp(hop[k]); h.hy[k] = exp(hop[4 + k]); h.hxe[k] = exp(hop[8 + k]); h.hye[k] = exp(hop[12 + k]); }
    hipLaunchKernelGGL(vlr_homopoly_kernel, dim3((unsigned)b->n_pairs), dim3(64), 0, (hipStream_t)stream, h);
    return (int)hipGetLastError();
}

// which pair-HMM kernel the last vlr_launch_realign_kernel of this process launched: 1 = vlr_realign_kernel, 2 = vlr_realign_kernel2,
// 0 = none yet (for the test that compares the two)
static int realign_pairs_per_wave = 0;
extern "C" int vlr_launch_realign_pairs_per_wave(void) { return realign_pairs_per_wave; }

extern "C" int vlr_launch_realign_kernel(const vlr_realign_batch_desc* b, double* ln_prob, void* stream) {
    using namespace vlr;
    if (b->n_pairs <= 0) return 0;
    RealignArgs a;
    set_linear(a, b, ln_prob);
    static const bool single = getenv("VLR_REALIGN_SINGLE") != nullptr;  // tuning / comparison knob
    realign_pairs_per_wave = single ? 1 : 2;
    if (single) hipLaunchKernelGGL(vlr_realign_kernel, dim3((unsigned)b->n_pairs), dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(vlr_realign_kernel2, dim3((unsigned)((b->n_pairs + 1) / 2)), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int vlr_launch_edit_kernel(const vlr_realign_batch_desc* b, int32_t* dist, int32_t* end, int32_t* n_hits, void* stream) {
    using namespace vlr;
    if (b->n_pairs <= 0) return 0;
    EditArgs a;
    set_pairs(a, b);
    a.dist = dist; a.end = end; a.n_hits = n_hits;
    hipLaunchKernelGGL(vlr_edit_kernel, dim3((unsigned)b->n_pairs), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
