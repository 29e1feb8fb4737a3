// Host-side declarations of vn_adapt.hip: self-adaptive per-test-function weights (vn_set_tf_adapt).  A state lambda_k lives on
// the device and moves at every gradient step from that step's own loss field; the weights in use are a function of the
// COMMITTED state only.  Maths, stage order and the determinism contract: that file's header.  Kept out of vn_internal.h, which
// every kernel's source hash covers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int VN_ADAPT_SPAN = 1024;          // test functions per block and pass: 256 threads x 4
constexpr int VN_ADAPT_MAX_BLOCKS = 256;     // a block's prologue folds at most one partial per thread
constexpr int VN_ADAPT_SCAL = 8;             // doubles of a state's scalars: min, max, mean omega | share | Z | tau | 2 spare
enum { VN_ADAPT_NONE = 0, VN_ADAPT_RBA = 1, VN_ADAPT_SA = 2 };

// Grid of the three kernels: a function of n_k alone (never of the card), so the bits do not depend on the device
inline int vn_adapt_grid(long n_k) {
  const long b = (n_k + VN_ADAPT_SPAN - 1) / VN_ADAPT_SPAN;
  return (int)(b < 1 ? 1 : b > VN_ADAPT_MAX_BLOCKS ? VN_ADAPT_MAX_BLOCKS : b);
}
inline long vn_adapt_stride(long n_k) { return (n_k + 3) / 4 * 4; }   // every [n_k] piece of a state starts on the 16-byte grid

// One half of the double buffer.  lambda, omega [n_k]; m1, m2 [n_k] (sa, else nullptr); scal [VN_ADAPT_SCAL]
struct VnAdaptState {
  float* lambda = nullptr;
  float* m1 = nullptr;
  float* m2 = nullptr;
  float* omega = nullptr;
  double* scal = nullptr;
};

struct VnAdaptArgs {
  int rule = VN_ADAPT_NONE;                  // VN_ADAPT_NONE: lambda' = lambda, slots and tau kept (omega, Z, statistics rebuilt)
  int power = 2, normalize = 1;
  float gamma = 0.f, eta = 0.f, cap = 0.f;   // rba: gamma, eta;  sa: cap
  double lr = 0.0, beta1 = 0.0, beta2 = 0.0, eps = 0.0;   // sa
  long n_k = 0;
  const float* lossVec = nullptr;            // [n_k] unweighted l_k of this step, 16-byte aligned; unused by VN_ADAPT_NONE
  VnAdaptState cur, next;                    // committed (read) and pending (written); next == cur is allowed for VN_ADAPT_NONE
  double* part = nullptr;                    // [VN_ADAPT_MAX_BLOCKS * 6]: (max l, sum l) per block, then (sum m, sum m^2, min m, max m)
};

// lambda' , slots', tau' from lossVec and the committed state; omega', Z' and the statistics of the pending state.
// Three launches (two for VN_ADAPT_NONE), no floating-point atomics, every fold in a fixed order.
hipError_t vn_adapt_update_launch(const VnAdaptArgs& a, hipStream_t s);

// dst[k] = src[k] over n entries of any alignment; *err_dev += entries that are not finite or are negative (0 on entry)
hipError_t vn_adapt_check_copy_launch(const float* src, long n, float* dst, int* err_dev, hipStream_t s);
// dst[k] = v
hipError_t vn_adapt_fill_launch(float* dst, long n, float v, hipStream_t s);
