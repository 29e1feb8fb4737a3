// Polynomial flux term (vn_set_nlflux): c_t = div(kappa grad c) - v.grad c - div(w(x,t) F(c)) + s + rate p(c),
// F(c) = f1 c + f2 c^2 + f3 c^3 (Burgers: w = 1, F = c^2 / 2).  In the weak form the flux integrates by parts onto the test
// function, so only the network VALUE enters: with phi_r = sum_d w_d(x_r, t_r) dN_r/dx_d the row integrand gains -F(u_r) phi_r
// and the value seed of a row gains -phi_r F'(u_r) times the row's tangent seed.  All kernels here are HBM-bound and small:
//
// row-wise routes (vn_seed_kernel and vn_internal.h are not edited):
//   vn_nlflux_fold_kernel    ud[r] -= F(u_r) phi_r, in place, BEFORE vn_seed_kernel: the seed kernel starts the row integrand from
//                            ud[r] = sum_d u_{x_d} gcoef_d, and every later term is added to it;
//   vn_nlflux_seed_kernel    ubar[r] -= phi_r F'(u_r) udbar[r], AFTER vn_seed_kernel (udbar[r] already carries W_p).
//   Both: one row per thread, or four rows per thread with 16-byte accesses when nT and the pointers allow.
//
// de-duplicated step (vn_dedup.hip is not edited; modelled on vn_react.hip):
//   vn_nlflux_source_kernel  one row per thread: s_eff[r] = base[r] + F(u_j) phi_r / N_p, j = uid[r] -- handed to
//                            vn_dedup_seed_kernel as its `source`, which subtracts s_eff N_p from the row integrand;
//   vn_nlflux_gather_kernel  one unique point per thread: d loss / d u_j -= F'(u_j) sum_r W_p phi_r stf[k_r] over the rows of the
//                            point in CSR order (fixed order: bitwise repeatable), added to what vn_dedup_gather_kernel stored.
#include <cstdint>

#include "vn_internal.h"
#include "vn_nlflux.h"

namespace {

typedef float f32x4n __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float flux_F(float u, float f1, float f2, float f3) { return u * (f1 + u * (f2 + u * f3)); }
__device__ __forceinline__ float flux_dF(float u, float f1, float f2, float f3) { return f1 + u * (2.f * f2 + 3.f * f3 * u); }

__global__ __launch_bounds__(256) void vn_nlflux_fold_kernel(VnNlfluxRowArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  a.ud[r] -= flux_F(a.u[r], a.f1, a.f2, a.f3) * a.phi[r];
}

__global__ __launch_bounds__(256) void vn_nlflux_fold4_kernel(VnNlfluxRowArgs a) {      // nT % 4 == 0, 16-byte aligned pointers
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nT / 4) return;
  const f32x4n u = reinterpret_cast<const f32x4n*>(a.u)[i];
  const f32x4n ph = reinterpret_cast<const f32x4n*>(a.phi)[i];
  f32x4n ud = reinterpret_cast<const f32x4n*>(a.ud)[i];
#pragma unroll
  for (int c = 0; c < 4; ++c) ud[c] -= flux_F(u[c], a.f1, a.f2, a.f3) * ph[c];
  reinterpret_cast<f32x4n*>(a.ud)[i] = ud;
}

__global__ __launch_bounds__(256) void vn_nlflux_seed_kernel(VnNlfluxRowArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  a.ubar[r] -= a.phi[r] * flux_dF(a.u[r], a.f1, a.f2, a.f3) * a.udbar[r];
}

__global__ __launch_bounds__(256) void vn_nlflux_seed4_kernel(VnNlfluxRowArgs a) {      // nT % 4 == 0, 16-byte aligned pointers
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nT / 4) return;
  const f32x4n u = reinterpret_cast<const f32x4n*>(a.u)[i];
  const f32x4n ph = reinterpret_cast<const f32x4n*>(a.phi)[i];
  const f32x4n sd = reinterpret_cast<const f32x4n*>(a.udbar)[i];
  f32x4n ub = reinterpret_cast<const f32x4n*>(a.ubar)[i];
#pragma unroll
  for (int c = 0; c < 4; ++c) ub[c] -= ph[c] * flux_dF(u[c], a.f1, a.f2, a.f3) * sd[c];
  reinterpret_cast<f32x4n*>(a.ubar)[i] = ub;
}

__global__ __launch_bounds__(256) void vn_nlflux_source_kernel(VnNlfluxDedupArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  const long j = a.uid[r];                                     // (validated against U by vn_set_dedup)
  const int p = (int)(r % a.q);
  const float base = a.base ? a.base[r] : 0.f;
  const float u = a.upack[j * 4];
  // vn_dedup_seed_kernel multiplies its source by N_p (non-zero: checked on the host against the table of vn_set_fe_table)
  a.s_eff[r] = base + flux_F(u, a.f1, a.f2, a.f3) * a.phi[r] / a.feN[p];
}

// A point has 2^feDim rows on a uniform grid (<= 8): four entries in flight per thread -- all row indices, then all dependent
// loads, then the additions in CSR order.
__global__ __launch_bounds__(256) void vn_nlflux_gather_kernel(VnNlfluxDedupArgs a) {
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
      float t = a.phi[ru] * a.stf[k];
      if (a.feW) t *= a.feW[p];
      v[c] = r[c] >= 0 ? t : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (r[c] >= 0) acc += v[c];
  }
  a.seed_u[j] = su - flux_dF(u, a.f1, a.f2, a.f3) * acc;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t vn_nlflux_fold_launch(const VnNlfluxRowArgs& a, hipStream_t s) {
  if (a.nT <= 0) return hipSuccess;
  if (a.nT % 4 == 0 && aligned16(a.u) && aligned16(a.phi) && aligned16(a.ud))
    hipLaunchKernelGGL(vn_nlflux_fold4_kernel, dim3((unsigned)((a.nT / 4 + 255) / 256)), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(vn_nlflux_fold_kernel, dim3((unsigned)((a.nT + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_nlflux_seed_launch(const VnNlfluxRowArgs& a, hipStream_t s) {
  if (a.nT <= 0) return hipSuccess;
  if (a.nT % 4 == 0 && aligned16(a.u) && aligned16(a.phi) && aligned16(a.udbar) && aligned16(a.ubar))
    hipLaunchKernelGGL(vn_nlflux_seed4_kernel, dim3((unsigned)((a.nT / 4 + 255) / 256)), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(vn_nlflux_seed_kernel, dim3((unsigned)((a.nT + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_nlflux_source_launch(const VnNlfluxDedupArgs& a, hipStream_t s) {
  if (a.nT <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_nlflux_source_kernel, dim3((unsigned)((a.nT + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_nlflux_gather_launch(const VnNlfluxDedupArgs& a, hipStream_t s) {
  if (a.U <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_nlflux_gather_kernel, dim3((unsigned)((a.U + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}
