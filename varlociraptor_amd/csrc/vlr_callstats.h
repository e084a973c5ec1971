// vlr_callstats.h — what csrc/vlr_callstats.hip offers the engine's other translation units (not part of the public ABI).
#ifndef VLR_CALLSTATS_H
#define VLR_CALLSTATS_H
#include <stdint.h>

extern "C" {
// vlr_range_group_lse (include/vlr.h) with the host-to-device copies made in pieces of `piece` entries (<= 0: one piece); the
// file-level command uploads this way.  The result does not depend on `piece`.
int vlr_launch_range_group_lse(int device, int64_t n, const double* vaf, const double* ln_prob, const int32_t* group, int n_ranges, const double* lo,
                               const double* hi, int n_groups, int64_t piece, double* out);
}
#endif
