// Host-side declarations of vn_balance.hip: the statistics of up to four gradient vectors (norms, mean and largest entry, Gram
// matrix) and the sum of a term's gradient over the batches of an epoch (maths and order contract: that file's header).  Kept out
// of vn_internal.h, which every kernel's source hash covers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define VN_BAL_MAX_K 4                       // VN_TERM_N of include/varnet_hip.h
#define VN_BAL_MAX_BLOCKS 1024               // rows of stage-1 partials at most
#define VN_BAL_ROW (3 * VN_BAL_MAX_K + VN_BAL_MAX_K * (VN_BAL_MAX_K - 1) / 2)   // doubles per row: 12 statistics + 6 dot products
#define VN_BAL_OUT (3 * VN_BAL_MAX_K + VN_BAL_MAX_K * VN_BAL_MAX_K)             // doubles of the result slot: stats [K][3] | gram [K][K]

// Stage-1 grid of a vector length: a function of n alone (never of the card), so the bits of the sums do not depend on the device.
int vn_balance_grid(int64_t n);

// stats [K][3] = {sum x^2, sum |x|, max |x|} and the symmetric gram [K][K] of T [K][n] (fp32, device) into out (device, the first
// 3 K + K K doubles of a slot of VN_BAL_OUT); part: VN_BAL_MAX_BLOCKS * VN_BAL_ROW doubles of device scratch.  Two launches, no
// atomics.  hipErrorInvalidValue for K outside 1..VN_BAL_MAX_K, n < 1 or a null pointer: nothing is launched.
hipError_t vn_balance_stats_launch(const float* T, int K, int64_t n, double* part, double* out, hipStream_t s);

// T[p] = g[p] (first) or fl32(T[p] + g[p]) over n entries, and val = (first ? 0 : val) + x with x the float at vf or, when vf is
// null, the double at vd (both null: val is left alone).  hipErrorInvalidValue for n < 1 or a null T or g.
hipError_t vn_balance_accum_launch(float* T, const float* g, int64_t n, int first, double* val, const float* vf, const double* vd,
                                   hipStream_t s);
