// Per-test-function loss weights and the causal time-slab mode
//     var = sum_k omega_k l_k,   l_k = detJ_k R_k^2 (lossVec[k], which stays unweighted everywhere),
//     loss = w0 BC + w1 IC + w2 var,   omega held CONSTANT for the gradient.
//   static  (vn_set_tf_weights)  omega_k given by the caller.
//   causal  (vn_set_causal)      every test function has a slab id s_k in [0, S); with L_s the mean of l_k over the batch's test
//                                functions of slab s (an empty slab: 0) and C_s = sum_{s' < s} L_s',
//                                omega_k = exp(-eps C_{s_k}): 1 on slab 0, small where the earlier slabs have not converged
//                                (Wang, Sankaran, Perdikaris 2022).  Recomputed at every step from that step's own loss field.
// The seed of a test function becomes 2 w2 omega_k detJ_k R_k, and every per-row seed derived from it -- time term, reaction, flux
// and D(u) value seeds, the D(u) rescale -- is linear in it.  So nothing here touches the seed kernels: the weights are applied in
// kernels of their own, after them.
//
// Stage order (weights_stage of vn_api.hip is the only caller):
//   seed kernel (vn_seed_kernel / vn_dedup_seed_kernel / vn_obj64_seed_kernel, writing lossVec)
//   the terms' seed kernels (row-wise routes: vn_terms.hip)
//   [causal] vn_slab_sum_kernel      lsum[s, c] = chunk c's share of sum_{k in slab s} lossVec[k]
//   vn_weights_apply_kernel          [causal: L_s, C_s, omega_s in LDS, omega_k = omega_{s_k};] stf[k] *= omega_k (de-duplicated
//                                    step: before vn_dedup_gather_kernel); loss partial of the block = sum omega_k lossVec[k]
//   vn_weights_rows_kernel           row-wise routes: ubar[r] *= omega_{r/q}, udbar[r] *= omega_{r/q}
// Everything is n_k-sized but the last kernel, latency-bound (n_k reaches 1e5, S is tens) and accumulates the slab statistics
// in fp64 in a FIXED order: within a slab a fixed stride per thread over the CSR (increasing k) and a fixed shuffle / wave tree,
// the chunks of a slab in chunk order, the prefix over S as contiguous per-thread segments joined sequentially.  No
// floating-point atomics: two calls give the same bits (vn_state_rollback + replay and train()'s lossLag blocks rely on that).
#include <cstdint>

#include "vn_internal.h"
#include "vn_rows4.h"
#include "vn_weights.h"

namespace {

template <class T>
__device__ __forceinline__ T block_sum_w(T v, T* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void vn_weights_check_kernel(const int* slab, long n_k, int S, int* err) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_k) return;
  if (slab[k] < 0 || slab[k] >= S) atomicAdd(err, 1);
}

// grid (chunks, S): chunk c of slab s walks the slab's CSR entries c*256 + tid, + chunks*256, ... -- four loads in flight
template <class T>
__global__ __launch_bounds__(256) void vn_slab_sum_kernel(const T* __restrict__ lossVec, const int* __restrict__ sptr,
                                                          const int* __restrict__ sidx, double* __restrict__ lsum) {
  __shared__ double red[4];
  const int s = blockIdx.y, c = blockIdx.x, C = gridDim.x;
  const long e0 = sptr[s], e1 = sptr[s + 1];
  const long step = (long)C * 256;
  double acc = 0.0;
  for (long e = e0 + (long)c * 256 + threadIdx.x; e < e1; e += 4 * step) {
    int k[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = (e + j * step < e1) ? sidx[e + j * step] : -1;
    T v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = k[j] >= 0 ? lossVec[k[j]] : (T)0;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += (double)v[j];
  }
  const double t = block_sum_w(acc, red);
  if (threadIdx.x == 0) lsum[(long)s * C + c] = t;
}

struct ApplyArgs {
  VnWeightsReg w;
  const double* lsum; double* oslab;
  long n_k; int tfb, stride;
};

// One block = the tfb test functions of one loss partial, k = blockIdx.x * tfb + tid for tid < tfb (tfb <= 256).
// Causal: every block first rebuilds omega_s of all slabs in LDS from the S * chunks partial sums (S is tens: cheaper than a
// launch of its own; the same code in every block, so every block holds the same bits).
template <class T>
__global__ __launch_bounds__(256) void vn_weights_apply_kernel(ApplyArgs a, const T* __restrict__ lossVec, T* omega_out, T* stf,
                                                               T* part) {
  __shared__ double som[VN_WEIGHTS_MAX_SLABS];
  __shared__ double seg[256];
  __shared__ T red[4];
  const int tid = threadIdx.x, S = a.w.S;
  if (S > 0) {
    const int C = a.w.chunks;
    for (int s = tid; s < S; s += 256) {
      double L = 0.0;
      for (int c = 0; c < C; ++c) L += a.lsum[(long)s * C + c];
      const int cnt = a.w.sptr[s + 1] - a.w.sptr[s];
      som[s] = cnt > 0 ? L / (double)cnt : 0.0;                // L_s; an empty slab: 0
    }
    __syncthreads();
    // exclusive prefix C_s: thread t owns slabs [t * per, (t + 1) * per), thread 0 joins the segment totals in order
    const int per = (S + 255) / 256;
    const int s0 = tid * per, s1 = (s0 + per < S) ? s0 + per : S;
    double loc = 0.0;
    for (int s = s0; s < s1; ++s) loc += som[s];
    seg[tid] = loc;
    __syncthreads();
    if (tid == 0) {
      double run = 0.0;
      for (int t = 0; t < 256; ++t) { const double v = seg[t]; seg[t] = run; run += v; }
    }
    __syncthreads();
    double run = seg[tid];
    for (int s = s0; s < s1; ++s) {
      const double L = som[s];
      som[s] = exp(-a.w.eps * run);                            // omega_s, exp in double
      run += L;
    }
    __syncthreads();
    if (blockIdx.x == 0)
      for (int s = tid; s < S; s += 256) a.oslab[s] = som[s];
  }
  const long k = (long)blockIdx.x * a.tfb + tid;
  T wl = (T)0;
  if (tid < a.tfb && k < a.n_k) {
    const T om = S > 0 ? (T)som[a.w.slab[k]] : (T)a.w.omega[k];  // (slab ids validated against S by vn_set_causal)
    if (omega_out) omega_out[k] = om;
    if (stf) stf[k] *= om;
    wl = om * lossVec[k];
  }
  const T t = block_sum_w(wl, red);
  if (tid == 0) part[(long)blockIdx.x * a.stride] = t;
}

template <class T>
__global__ __launch_bounds__(256) void vn_weights_rows_kernel(const T* __restrict__ omega, long nT, int q, T* ubar, T* udbar) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= nT) return;
  const T om = omega[r / q];
  ubar[r] *= om;
  udbar[r] *= om;
}

// q % 4 == 0 (the four rows of a thread belong to one test function), 16-byte aligned pointers
__global__ __launch_bounds__(256) void vn_weights_rows4_kernel(const float* __restrict__ omega, long nT, int q, float* ubar,
                                                               float* udbar) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nT / 4) return;
  const float om = omega[(i * 4) / q];
  f32x4t a = load4(ubar, i), b = load4(udbar, i);
#pragma unroll
  for (int c = 0; c < 4; ++c) { a[c] *= om; b[c] *= om; }
  store4(ubar, i, a);
  store4(udbar, i, b);
}

template <class T>
hipError_t apply(const VnWeightsReg& w, const VnWeightsWork& wk, const T* lossVec, long n_k, int tfb, int stride, T* omega_out,
                 T* stf, T* part, hipStream_t s) {
  if (n_k <= 0 || !vn_weights_on(w)) return hipSuccess;
  if (tfb < 1 || tfb > 256 || w.S > VN_WEIGHTS_MAX_SLABS || w.chunks < 1 || w.chunks > VN_WEIGHTS_MAX_CHUNKS)
    return hipErrorInvalidValue;
  if (w.S > 0) {
    hipLaunchKernelGGL(vn_slab_sum_kernel<T>, dim3(w.chunks, w.S), dim3(256), 0, s, lossVec, w.sptr, w.sidx, wk.lsum);
    if (hipError_t e = hipGetLastError()) return e;
  }
  ApplyArgs a{};
  a.w = w; a.lsum = wk.lsum; a.oslab = wk.oslab; a.n_k = n_k; a.tfb = tfb; a.stride = stride;
  hipLaunchKernelGGL(vn_weights_apply_kernel<T>, dim3((unsigned)((n_k + tfb - 1) / tfb)), dim3(256), 0, s, a, lossVec, omega_out,
                     stf, part);
  return hipGetLastError();
}

}  // namespace

hipError_t vn_weights_check_launch(const int* slab, long n_k, int S, int* err_dev, hipStream_t s) {
  if (n_k <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_weights_check_kernel, dim3((unsigned)((n_k + 255) / 256)), dim3(256), 0, s, slab, n_k, S, err_dev);
  return hipGetLastError();
}

hipError_t vn_weights_apply_f32(const VnWeightsReg& w, const VnWeightsWork& wk, const float* lossVec, long n_k, int tfb,
                                float* omega_out, float* stf, float* part, hipStream_t s) {
  return apply<float>(w, wk, lossVec, n_k, tfb, 3, omega_out, stf, part, s);
}

hipError_t vn_weights_apply_f64(const VnWeightsReg& w, const VnWeightsWork& wk, const double* lossVec, long n_k,
                                double* omega_out, double* part, hipStream_t s) {
  return apply<double>(w, wk, lossVec, n_k, 256, 4, omega_out, nullptr, part, s);
}

hipError_t vn_weights_rows_f32(const float* omega, long n_k, int q, float* ubar, float* udbar, hipStream_t s) {
  const long nT = n_k * q;
  if (nT <= 0) return hipSuccess;
  const bool four = rows4_ok(q, {omega, ubar, udbar});
  const long n = four ? nT / 4 : nT;
  if (four) hipLaunchKernelGGL(vn_weights_rows4_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, omega, nT, q, ubar, udbar);
  else hipLaunchKernelGGL(vn_weights_rows_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, omega, nT, q, ubar, udbar);
  return hipGetLastError();
}

hipError_t vn_weights_rows_f64(const double* omega, long n_k, int q, double* ubar, double* udbar, hipStream_t s) {
  const long nT = n_k * q;
  if (nT <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_weights_rows_kernel<double>, dim3((unsigned)((nT + 255) / 256)), dim3(256), 0, s, omega, nT, q, ubar, udbar);
  return hipGetLastError();
}
