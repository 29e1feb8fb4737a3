// Self-adaptive per-test-function weights (vn_set_tf_adapt): a state lambda_k >= 0 per test function, on the device, moved at every
// gradient step from that step's own unweighted loss field l_k = lossVec[k].
//     weights in use   omega_k = m(lambda_k) / Z,  m(x) = x^p (p = 1, 2),  Z = mean_j m(lambda_j) (normalize) or 1
//                      -- a function of the COMMITTED state only, constant for the gradient, so a static registration of the
//                      committed omega buffer (VnWeightsReg::omega, vn_weights.hip) carries them through every route.
//     rba              r_k = sqrt(l_k), r_max = max_j r_j:   lambda'_k = gamma lambda_k + eta r_k / r_max
//     sa               lbar = mean_j l_j (fp64, fixed order), g_k = m'(lambda_k) l_k / lbar, Adam ASCENT on lambda:
//                      m1 = b1 m1 + (1 - b1) g, m2 = b2 m2 + (1 - b2) g^2, lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), t = tau + 1,
//                      lambda'_k = clamp(lambda_k + lr_t m1 / (sqrt(m2) + eps), 0, cap)
//     r_max (rba) or lbar (sa) zero or not finite: lambda' = lambda, slots and tau kept -- an all-zero loss field or a diverged step
//     does not move the state.
// The update writes the PENDING half of a double buffer (lambda', slots', omega', Z', tau', statistics); the host commits it by
// swapping the halves at the optimizer step.  omega therefore lags the loss field by one step, for both rules.
//
// Stage order (weights_stage of vn_api.hip is the only caller of the update), after the seed kernel has written lossVec:
//   vn_adapt_reduce_kernel     part[b] = (max l, sum l in fp64) of block b's test functions
//   vn_adapt_update_kernel     every block folds those partials in its prologue (the same code, so the same bits, in every block),
//                              then lambda', slots', and part[b] = (sum m, sum m^2, min m, max m) of m(lambda') in fp64
//   vn_adapt_norm_kernel       every block folds those into Z', omega'_k = fl32(m(lambda'_k) / Z'); block 0 writes the statistics
//                              min, max, mean omega and the effective sample share (sum omega)^2 / (n_k sum omega^2)
// All three are n_k-sized, on a grid fixed by n_k alone (vn_adapt_grid), four test functions per thread with 16-byte accesses
// (every buffer is the engine's own and starts on the 16-byte grid, the loss field of a gradient evaluation included) and
// scalar accesses in the last, partial group.  Every sum is a fixed shuffle / wave tree over fixed per-thread strides; no floating-point atomics:
// two runs give the same bits on any card (vn_state_rollback + replay and train()'s lossLag blocks rely on that).
// Square roots and divisions are the correctly rounded __fsqrt_rn / __fdiv_rn.
#include <cmath>

#include "vn_adapt.h"
#include "vn_rows4.h"

namespace {

constexpr int kPartR = 2, kPartU = 4;                       // doubles per block of the reduce / update partials
constexpr int kPartUOff = VN_ADAPT_MAX_BLOCKS * kPartR;     // where the update partials start in VnAdaptArgs::part

struct Sum { __device__ static double f(double a, double b) { return a + b; } };
struct Max { __device__ static double f(double a, double b) { return a > b ? a : b; } };
struct Min { __device__ static double f(double a, double b) { return a < b ? a : b; } };

// One double per thread over the 256-thread block, fixed order: shuffle tree per wave, the four waves left to right.
// NaN: Sum carries it; Max / Min callers encode a bad entry as +inf / -inf themselves.
template <class Op>
__device__ __forceinline__ double block_fold(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v = Op::f(v, __shfl_down(v, o, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return Op::f(Op::f(Op::f(red[0], red[1]), red[2]), red[3]);
}

// Entries k .. k + 3 of p (zero beyond n), p on the 16-byte grid: one 16-byte access for a whole group, scalars in the last,
// partial one
__device__ __forceinline__ f32x4t ld4(const float* p, long k, long n) {
  if (k + 4 <= n) return load4(p, k >> 2);
  f32x4t v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (k + j < n) v[j] = p[k + j];
  return v;
}
__device__ __forceinline__ void st4(float* p, long k, long n, f32x4t v) {
  if (k + 4 <= n) { store4(p, k >> 2, v); return; }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (k + j < n) p[k + j] = v[j];
}

__device__ __forceinline__ float mfun(float lam, int power) { return power == 2 ? lam * lam : lam; }

__global__ __launch_bounds__(256) void vn_adapt_reduce_kernel(const float* __restrict__ lossVec, long n_k, double* part) {
  __shared__ double red[4];
  double mx = 0.0, sum = 0.0;
  for (long k = 4 * ((long)blockIdx.x * 256 + threadIdx.x); k < n_k; k += (long)gridDim.x * VN_ADAPT_SPAN) {
    const f32x4t l = ld4(lossVec, k, n_k);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double v = (double)l[j];
      mx = v == v ? Max::f(mx, v) : (double)INFINITY;         // a NaN entry: the field is not finite
      sum += v;
    }
  }
  const double bm = block_fold<Max>(mx, red), bs = block_fold<Sum>(sum, red);
  if (threadIdx.x == 0) { part[blockIdx.x * kPartR] = bm; part[blockIdx.x * kPartR + 1] = bs; }
}

__global__ __launch_bounds__(256) void vn_adapt_update_kernel(VnAdaptArgs a) {
  __shared__ double red[4];
  __shared__ float s_lr;
  const int tid = threadIdx.x, nb = gridDim.x;
  const long n = a.n_k;
  bool move = false;
  float rmax = 1.f, lbar = 1.f, lr_t = 0.f;
  const double tau = a.cur.scal[5];
  if (a.rule != VN_ADAPT_NONE) {
    const double lmax = block_fold<Max>(tid < nb ? a.part[tid * kPartR] : 0.0, red);
    const double lsum = block_fold<Sum>(tid < nb ? a.part[tid * kPartR + 1] : 0.0, red);
    if (a.rule == VN_ADAPT_RBA) {
      move = lmax > 0.0 && lmax < (double)INFINITY;
      rmax = __fsqrt_rn((float)lmax);
    } else {
      const double mean = lsum / (double)n;
      lbar = (float)mean;
      move = mean > 0.0 && mean < (double)INFINITY && lbar > 0.f && lbar < INFINITY;
      if (tid == 0) {                                          // the bias-corrected rate, once per block
        const double t = tau + 1.0;
        s_lr = (float)(a.lr * sqrt(1.0 - pow(a.beta2, t)) / (1.0 - pow(a.beta1, t)));
      }
      __syncthreads();
      lr_t = s_lr;
    }
  }
  const float b1 = (float)a.beta1, b2 = (float)a.beta2, eps = (float)a.eps;
  const float c1 = (float)(1.0 - a.beta1), c2 = (float)(1.0 - a.beta2);   // formed in double: fl32(1) - fl32(0.999) is 3e-5 off
  double sm = 0.0, sm2 = 0.0, mn = (double)INFINITY, mx = -(double)INFINITY;
  for (long k = 4 * ((long)blockIdx.x * 256 + tid); k < n; k += (long)nb * VN_ADAPT_SPAN) {
    f32x4t lam = ld4(a.cur.lambda, k, n);
    if (move && a.rule == VN_ADAPT_RBA) {
      const f32x4t l = ld4(a.lossVec, k, n);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float r = __fsqrt_rn(l[j] > 0.f ? l[j] : 0.f);
        lam[j] = a.gamma * lam[j] + a.eta * __fdiv_rn(r, rmax);
      }
    } else if (a.rule == VN_ADAPT_SA) {
      f32x4t m1 = ld4(a.cur.m1, k, n), m2 = ld4(a.cur.m2, k, n);
      if (move) {
        const f32x4t l = ld4(a.lossVec, k, n);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float g = (a.power == 2 ? 2.f * lam[j] : 1.f) * __fdiv_rn(l[j], lbar);
          m1[j] = b1 * m1[j] + c1 * g;
          m2[j] = b2 * m2[j] + c2 * (g * g);
          const float x = lam[j] + lr_t * __fdiv_rn(m1[j], __fsqrt_rn(m2[j]) + eps);
          lam[j] = x > 0.f ? (x < a.cap ? x : a.cap) : 0.f;     // clamp to [0, cap]
        }
      }
      if (a.next.m1 != a.cur.m1) { st4(a.next.m1, k, n, m1); st4(a.next.m2, k, n, m2); }
    }
    if (a.next.lambda != a.cur.lambda || move) st4(a.next.lambda, k, n, lam);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (k + j < n) {
        const double m = (double)mfun(lam[j], a.power);
        sm += m; sm2 += m * m;
        mn = Min::f(mn, m); mx = Max::f(mx, m);
      }
  }
  const double bs = block_fold<Sum>(sm, red), bs2 = block_fold<Sum>(sm2, red);
  const double bmn = block_fold<Min>(mn, red), bmx = block_fold<Max>(mx, red);
  if (tid == 0) {
    double* p = a.part + kPartUOff + blockIdx.x * kPartU;
    p[0] = bs; p[1] = bs2; p[2] = bmn; p[3] = bmx;
    if (blockIdx.x == 0) a.next.scal[5] = move ? tau + 1.0 : tau;
  }
}

__global__ __launch_bounds__(256) void vn_adapt_norm_kernel(VnAdaptArgs a) {
  __shared__ double red[4];
  const int tid = threadIdx.x, nb = gridDim.x;
  const long n = a.n_k;
  const double* p = a.part + kPartUOff + tid * kPartU;
  const bool in = tid < nb;
  const double s1 = block_fold<Sum>(in ? p[0] : 0.0, red), s2 = block_fold<Sum>(in ? p[1] : 0.0, red);
  const double mn = block_fold<Min>(in ? p[2] : (double)INFINITY, red), mx = block_fold<Max>(in ? p[3] : -(double)INFINITY, red);
  double Z = a.normalize ? s1 / (double)n : 1.0;
  if (!(Z > 0.0 && Z < (double)INFINITY)) Z = 1.0;              // every lambda zero: omega = 0, not 0 / 0
  for (long k = 4 * ((long)blockIdx.x * 256 + tid); k < n; k += (long)nb * VN_ADAPT_SPAN) {
    const f32x4t lam = ld4(a.next.lambda, k, n);
    f32x4t om;
#pragma unroll
    for (int j = 0; j < 4; ++j) om[j] = (float)((double)mfun(lam[j], a.power) / Z);
    st4(a.next.omega, k, n, om);
  }
  if (blockIdx.x == 0 && tid == 0) {
    double* o = a.next.scal;
    o[0] = mn / Z; o[1] = mx / Z; o[2] = s1 / ((double)n * Z);
    o[3] = s2 > 0.0 ? s1 * s1 / ((double)n * s2) : 0.0;
    o[4] = Z;
  }
}

__global__ __launch_bounds__(256) void vn_adapt_check_copy_kernel(const float* __restrict__ src, long n, float* dst, int* err) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const float v = src[k];
  if (!(v >= 0.f && v < INFINITY)) atomicAdd(err, 1);
  dst[k] = v;
}

__global__ __launch_bounds__(256) void vn_adapt_fill_kernel(float* dst, long n, float v) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k < n) dst[k] = v;
}

}  // namespace

hipError_t vn_adapt_update_launch(const VnAdaptArgs& a, hipStream_t s) {
  if (a.n_k < 1 || !a.part || !a.cur.lambda || !a.cur.scal || !a.next.lambda || !a.next.omega || !a.next.scal) return hipErrorInvalidValue;
  if (a.rule != VN_ADAPT_NONE && a.rule != VN_ADAPT_RBA && a.rule != VN_ADAPT_SA) return hipErrorInvalidValue;
  if (a.rule != VN_ADAPT_NONE && (!a.lossVec || a.next.lambda == a.cur.lambda)) return hipErrorInvalidValue;
  if (a.rule == VN_ADAPT_SA && (!a.cur.m1 || !a.cur.m2 || !a.next.m1 || !a.next.m2)) return hipErrorInvalidValue;
  // the engine's own pieces sit on the 16-byte grid (vn_adapt_stride), and so does the loss field: every gradient evaluation
  // writes it to the engine's own [n_k] buffer (vn_grad takes no caller's array)
  for (const void* p : {(const void*)a.lossVec, (const void*)a.cur.lambda, (const void*)a.cur.m1, (const void*)a.cur.m2, (const void*)a.next.lambda,
                        (const void*)a.next.m1, (const void*)a.next.m2, (const void*)a.next.omega})
    if (!aligned16(p)) return hipErrorInvalidValue;
  const int grid = vn_adapt_grid(a.n_k);
  if (a.rule != VN_ADAPT_NONE) {
    hipLaunchKernelGGL(vn_adapt_reduce_kernel, dim3(grid), dim3(256), 0, s, a.lossVec, a.n_k, a.part);
    if (hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(vn_adapt_update_kernel, dim3(grid), dim3(256), 0, s, a);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(vn_adapt_norm_kernel, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_adapt_check_copy_launch(const float* src, long n, float* dst, int* err_dev, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_adapt_check_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, n, dst, err_dev);
  return hipGetLastError();
}

hipError_t vn_adapt_fill_launch(float* dst, long n, float v, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_adapt_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, n, v);
  return hipGetLastError();
}
