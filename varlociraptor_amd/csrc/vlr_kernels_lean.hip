// vlr_kernels_lean.hip — the lean build of the call kernel (see VLR_LEAN in vlr_kernels.hip): the same source with the AFD log and
// replay, the l2fc operands, the general tree walk with its single-chain runner and the mapping of plans above two samples compiled
// out, for plans and launches in which the host has proved all of them unreachable (vlr_host.cpp: the lean_ok block of vlr_plan_create, vlr_batch_run).
// Everything lives in namespace vlr_lean; the exported symbols are vlr_launch_call_kernel_lean and vlr_launch_call_lds_bytes_lean.
#define VLR_LEAN_BUILD 1
#define vlr vlr_lean
#include "vlr_kernels.hip"
