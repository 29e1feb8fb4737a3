// Polynomial reaction term in the de-duplicated step: c_t = div(kappa grad c) - v.grad c + s + rate(x,t) p(c),
// p(c) = c1 c + c2 c^2 + c3 c^3.  The term depends on the network VALUE only, which the point pass computes once per unique
// point, so it enters the de-duplicated assembly through two small HBM-bound kernels around the existing ones (vn_dedup.hip
// is not edited):
//   vn_react_source_kernel  one row per thread: s_eff[r] = source[r] + rate[r] p(u_j), j = uid[r] -- handed to
//                           vn_dedup_seed_kernel as its `source`, which subtracts s_eff N_p from the row integrand as it does
//                           for a plain source term (TFModel.py:657);
//   vn_react_gather_kernel  one unique point per thread: the value seed of the term, d loss / d u_j -= p'(u_j) sum_r N_p W_p
//                           rate[r] stf[k_r] over the rows of the point in CSR order (fixed order: bitwise repeatable), added to
//                           what vn_dedup_gather_kernel stored.
#include "vn_internal.h"
#include "vn_react.h"

namespace {

__global__ __launch_bounds__(256) void vn_react_source_kernel(VnReactArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  const long j = a.uid[r];                                     // (validated against U by vn_set_dedup)
  const float src = a.source ? a.source[r] : 0.f;
  const float rho = a.rate ? a.rate[r] : 1.f;
  const float u = a.upack[j * 4];
  const float pu = u * (a.c1 + u * (a.c2 + u * a.c3));
  a.s_eff[r] = src + (a.rate ? rho * pu : pu);
}

// A point has 2^feDim rows on a uniform grid (<= 8): four entries in flight per thread -- all row indices, then all dependent
// loads, then the additions in CSR order.
__global__ __launch_bounds__(256) void vn_react_gather_kernel(VnReactArgs a) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.U) return;
  const int q = a.q;
  const bool qpow2 = (q & (q - 1)) == 0;
  const int qshift = __ffs(q) - 1;
  const int e0 = a.rowptr[j], e1 = a.rowptr[j + 1];
  const float u = a.upack[j * 4];
  const float su = a.seed_u[j];
  float acc = 0.f;
  for (int e = e0; e < e1; e += 4) {
    int r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = (e + c < e1) ? a.rowidx[e + c] : -1;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      // row -> (test function, quadrature point): a shift when integ_num is a power of two, else one unsigned division
      const unsigned ru = r[c] >= 0 ? (unsigned)r[c] : 0u;
      const unsigned k = qpow2 ? ru >> qshift : ru / (unsigned)q;
      const unsigned p = ru - k * (unsigned)q;
      float t = a.feN[p] * a.stf[k];
      if (a.feW) t *= a.feW[p];
      if (a.rate) t *= a.rate[ru];
      v[c] = r[c] >= 0 ? t : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (r[c] >= 0) acc += v[c];
  }
  const float dp = a.c1 + u * (2.f * a.c2 + 3.f * a.c3 * u);
  a.seed_u[j] = su - dp * acc;
}

}  // namespace

hipError_t vn_react_source_launch(const VnReactArgs& a, hipStream_t s) {
  if (a.nT <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_react_source_kernel, dim3((unsigned)((a.nT + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_react_gather_launch(const VnReactArgs& a, hipStream_t s) {
  if (a.U <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_react_gather_kernel, dim3((unsigned)((a.U + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}
