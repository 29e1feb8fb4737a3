// Device-resident L-BFGS (vn_lbfgs_step): the optimizer arithmetic above vn_grad, vn_lbfgs.hip.  Kept out of vn_internal.h,
// which every kernel's source hash covers.
//
// The two-loop recursion runs in its Gram ("vector-free") form.  Basis B = [s slots | y slots | g_k]: the ring has
// VN_LBFGS_SLOTS = m + 1 physical slots per family (m live pairs at most; the spare one receives the pair of an accepted step
// BEFORE the curvature test s.y > 1e-10 |s||y| has decided whether it evicts the oldest), so VN_LBFGS_NB = 2 (m + 1) + 1 basis
// vectors and a VN_LBFGS_NB x VN_LBFGS_NB fp64 matrix G = B^T B.  Per iteration only the rows of the vectors that are new (the
// pair written by the last commit, and g_k) are recomputed.  Four kernels, a constant number of launches whatever m and P:
//   1. vn_lbfgs_gram_launch     multi-block: fp64 partials of <new vector, every live vector> and of |g_k|_1, fixed order
//   2. vn_lbfgs_twoloop_launch  one wave: folds the partials in block order into G, decides the pending pair, runs the two-loop
//                               on the coefficients, leaves delta (d = B delta), g.d, t0
//   3. vn_lbfgs_trial_launch    multi-block: d = B delta (first trial; kept for the halved ones), theta = fl32(theta_k + t d)
//   4. vn_lbfgs_commit_launch   multi-block: s, y into the spare slot; theta_k, g_k and the loss scalars replaced
// Ring position and length live on the device (VnLbfgsMeta): no kernel argument depends on a decision taken on the device.
#pragma once
#include <hip/hip_runtime.h>

#define VN_LBFGS_M 10                          /* = VN_LBFGS_HISTORY (include/varnet_hip.h) */
#define VN_LBFGS_SLOTS (VN_LBFGS_M + 1)
#define VN_LBFGS_NB (2 * VN_LBFGS_SLOTS + 1)   /* 23 basis vectors; the last one is g_k */
#define VN_LBFGS_NACC (3 * VN_LBFGS_NB + 1)    /* per-block partials: 3 new rows + |g|_1 */
#define VN_LBFGS_MAXBLK 256                    /* workgroups of the Gram kernel (a constant: results do not depend on the GPU) */

struct VnLbfgsMeta {
  int head;      // slot the next commit writes (the spare one)
  int count;     // live pairs: slots head-count .. head-1 (mod VN_LBFGS_SLOTS)
  int pending;   // a pair sits in slot `head`, its curvature test not taken yet
  int pad;
};

// What the one-wave kernel leaves for the host (in host memory the device writes to; read after a synchronise)
struct VnLbfgsOut {
  double gd;        // g_k . d
  double t0;        // first step length: min(1, 1/|g_k|_1) without pairs, else 1
  double g1;        // |g_k|_1
  double pairs;     // pairs the direction was formed from (0 after a drop)
  double dropped;   // 1: g_k . d >= 0 with pairs, ring dropped, d = -g_k
  double kept;      // 1: the pending pair passed the curvature test
};

struct VnLbfgsBufs {
  float* ring;        // [2 * VN_LBFGS_SLOTS, P]: s slots, then y slots
  float* theta_k;     // [P]
  float* g_k;         // [P + 4]: gradient | loss, BC, IC, var at theta_k
  float* d;           // [P]
  double* part;       // [VN_LBFGS_MAXBLK, VN_LBFGS_NACC]
  double* G;          // [VN_LBFGS_NB, VN_LBFGS_NB]
  double* coef;       // [VN_LBFGS_NB + 1]: delta | t0
  VnLbfgsMeta* meta;
  VnLbfgsOut* out;    // host memory mapped into the device
};

int vn_lbfgs_gram_blocks(long P);
// reset != 0: the ring is dropped before this iteration (only g_k is live)
hipError_t vn_lbfgs_gram_launch(const VnLbfgsBufs& b, long P, int reset, hipStream_t s);
hipError_t vn_lbfgs_twoloop_launch(const VnLbfgsBufs& b, long P, int reset, hipStream_t s);
// theta = fl32(theta_k + t0 * scale * d); form_d != 0: d = B delta first
hipError_t vn_lbfgs_trial_launch(const VnLbfgsBufs& b, float* theta, long P, double scale, int form_d, hipStream_t s);
// first != 0: theta_k <- theta, g_k <- grad (P + 4 floats), no pair (the evaluation that starts a run)
hipError_t vn_lbfgs_commit_launch(const VnLbfgsBufs& b, const float* theta, const float* grad, long P, int first, hipStream_t s);
