// Host-side declarations of vn_weights.hip: per-test-function loss weights omega_k (vn_set_tf_weights) and the causal
// time-slab mode that recomputes them from every step's own loss field (vn_set_causal).  Maths, stage order and the
// determinism contract: that file's header.  Kept out of vn_internal.h, which every kernel's source hash covers.
#pragma once
#include "vn_internal.h"

constexpr int VN_WEIGHTS_MAX_SLABS = 4096;   // n_slabs of vn_set_causal: the apply kernel keeps omega_s of every slab in LDS (32 KiB)
constexpr int VN_WEIGHTS_MAX_CHUNKS = 16;    // workgroups that share one slab's sum

// What a batch registered.  Static: omega.  Causal: S > 0 and the engine-owned copies slab / sptr / sidx.  Neither: nothing.
struct VnWeightsReg {
  const float* omega = nullptr;              // [n_k] caller-owned device floats, read on every step
  const int* slab = nullptr;                 // [n_k] slab id of every test function
  const int* sptr = nullptr;                 // [S + 1] CSR slab -> test functions ...
  const int* sidx = nullptr;                 // [n_k]   ... in increasing k: the slab sums have a fixed order
  int S = 0;
  int chunks = 1;                            // workgroups per slab of the sum kernel, fixed at registration (<= VN_WEIGHTS_MAX_CHUNKS)
  double eps = 0.0;
};
inline bool vn_weights_on(const VnWeightsReg& w) { return w.omega != nullptr || w.S > 0; }

// Engine-owned work buffers of the causal mode
struct VnWeightsWork {
  double* lsum = nullptr;                    // [S * chunks] partial slab sums
  double* oslab = nullptr;                   // [S] omega_s as last computed (vn_causal_weights reads it back)
};

// *err_dev += number of ids outside [0, S); err_dev must hold 0 on entry
hipError_t vn_weights_check_launch(const int* slab, long n_k, int S, int* err_dev, hipStream_t s);

// The weights stage after a seed kernel that wrote lossVec [n_k] (unweighted, and left so):
//   causal   L_s = mean of lossVec over slab s, C_s = sum_{s' < s} L_s', omega_s = exp(-eps C_s), omega_k = omega_{slab[k]}
//            (one launch for the slab sums, the rest inside the apply launch); omega_k is also stored to omega_out [n_k]
//   static   omega_k = omega[k]
//   apply    stf[k] *= omega_k where stf is given (the de-duplicated step's test-function seeds), and
//            part[b * stride] = sum of omega_k lossVec[k] over the tfb test functions of loss-partial block b (fixed tree),
//            in place of the unweighted sum the seed kernel left there; the BC / IC slots of the block stay.
// tfb: test functions per loss partial of the seed kernel that ran (256 row-wise, VN_DEDUP_TFB de-duplicated).
hipError_t vn_weights_apply_f32(const VnWeightsReg& w, const VnWeightsWork& wk, const float* lossVec, long n_k, int tfb,
                                float* omega_out, float* stf, float* part, hipStream_t s);
// fp64 objective (vn_obj64.hip): loss partials [blocks][4] of 256 test functions; omega_out [n_k] is always written (static
// weights widened exactly)
hipError_t vn_weights_apply_f64(const VnWeightsReg& w, const VnWeightsWork& wk, const double* lossVec, long n_k,
                                double* omega_out, double* part, hipStream_t s);

// Row-wise routes, after every term's seed kernel: ubar[r] *= omega[r / q], udbar[r] *= omega[r / q]  (exact: every per-row
// seed is linear in its test function's seed).  fp32: four rows per thread with 16-byte accesses when q % 4 == 0 and every
// pointer is 16-byte aligned, else one row per thread.
hipError_t vn_weights_rows_f32(const float* omega, long n_k, int q, float* ubar, float* udbar, hipStream_t s);
hipError_t vn_weights_rows_f64(const double* omega, long n_k, int q, double* ubar, double* udbar, hipStream_t s);
