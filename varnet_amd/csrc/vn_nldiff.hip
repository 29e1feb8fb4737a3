// Solution-dependent diffusivity (vn_set_nldiff): c_t = div(kappa(x,t) D(c) grad c) - v.grad c - div(w F(c)) + s + rate p(c),
// D(c) = d0 + d1 c + d2 c^2 (porous medium: D = c^m; temperature-dependent conductivity).  The engine carries ONE tangent per row,
// along gcoef; D(u) must scale the diffusion part only, so on a batch with the term gcoef = kappa dN/dx and the advection moves to
// the value side: int v.grad u N = -int u psi, psi_r = sum_d v_d dN_r/dx_d + N_r div v.  With A_r = sum_d u_{x_d} gcoef_d the row
// integrand starts from  D(u_r) A_r - u_r psi_r  instead of A_r, and with s_r the row's tangent seed
//     value seed  += (D'(u_r) A_r - psi_r) s_r,      tangent seed = D(u_r) s_r.
// Nothing divides by D(u): D(0) = 0 (porous medium) is a regular point.  All kernels here are HBM-bound and small:
//
// row-wise routes (vn_seed_kernel, vn_nlflux.hip, vn_react.hip and vn_internal.h are not edited):
//   vn_nldiff_fold_kernel    A[r] = ud[r]; ud[r] = D(u_r) A[r] - u_r psi_r, BEFORE everything else that edits ud: the seed kernel
//                            starts the row integrand from ud[r], and every later term is added to it;
//   vn_nldiff_seed_kernel    ubar[r] += (D'(u_r) A[r] - psi_r) udbar[r]; udbar[r] *= D(u_r), AFTER everything else that reads udbar
//                            (the flux term's seed kernel must see the unscaled tangent seed).
//   Both: one row per thread, or four rows per thread with 16-byte accesses when nT and the pointers allow.
//
// de-duplicated step (vn_dedup.hip is not edited):
//   vn_nldiff_source_kernel  one row per thread: s_eff[r] = base[r] + ((1 - D(u_j)) (grad u_j . gcoef_r) + u_j psi_r) / N_p,
//                            j = uid[r] -- vn_dedup_seed_kernel subtracts s_eff N_p from A_r, which leaves D(u_j) A_r - u_j psi_r;
//   vn_nldiff_point_kernel   one unique point per thread, after the gathers: seed_g[j,:] = sum_r W_p gcoef_r stf[k_r] is what the
//                            rows' tangent seeds add up to, so d loss / d u_j += D'(u_j) (grad u_j . seed_g[j,:]) and seed_g[j,:] *=
//                            D(u_j) need no gather; only -sum_r W_p psi_r stf[k_r] walks the rows of the point, in CSR order
//                            (fixed order: bitwise repeatable), four entries in flight.
#include <cstdint>

#include "vn_internal.h"
#include "vn_nldiff.h"

namespace {

typedef float f32x4e __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float diff_D(float u, float d0, float d1, float d2) { return d0 + u * (d1 + u * d2); }
__device__ __forceinline__ float diff_dD(float u, float d1, float d2) { return d1 + 2.f * d2 * u; }

__global__ __launch_bounds__(256) void vn_nldiff_fold_kernel(VnNldiffRowArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  const float u = a.u[r], A = a.ud[r];
  a.A[r] = A;
  float t = diff_D(u, a.d0, a.d1, a.d2) * A;
  if (a.psi) t -= u * a.psi[r];
  a.ud[r] = t;
}

__global__ __launch_bounds__(256) void vn_nldiff_fold4_kernel(VnNldiffRowArgs a) {      // nT % 4 == 0, 16-byte aligned pointers
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nT / 4) return;
  const f32x4e u = reinterpret_cast<const f32x4e*>(a.u)[i];
  const f32x4e A = reinterpret_cast<const f32x4e*>(a.ud)[i];
  f32x4e ps = {0.f, 0.f, 0.f, 0.f};
  if (a.psi) ps = reinterpret_cast<const f32x4e*>(a.psi)[i];
  f32x4e t;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    t[c] = diff_D(u[c], a.d0, a.d1, a.d2) * A[c];
    if (a.psi) t[c] -= u[c] * ps[c];
  }
  reinterpret_cast<f32x4e*>(a.A)[i] = A;
  reinterpret_cast<f32x4e*>(a.ud)[i] = t;
}

__global__ __launch_bounds__(256) void vn_nldiff_seed_kernel(VnNldiffRowArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  const float u = a.u[r], sd = a.udbar[r];
  float g = diff_dD(u, a.d1, a.d2) * a.A[r];
  if (a.psi) g -= a.psi[r];
  a.ubar[r] += g * sd;
  a.udbar[r] = diff_D(u, a.d0, a.d1, a.d2) * sd;
}

__global__ __launch_bounds__(256) void vn_nldiff_seed4_kernel(VnNldiffRowArgs a) {      // nT % 4 == 0, 16-byte aligned pointers
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nT / 4) return;
  const f32x4e u = reinterpret_cast<const f32x4e*>(a.u)[i];
  const f32x4e A = reinterpret_cast<const f32x4e*>(a.A)[i];
  f32x4e sd = reinterpret_cast<const f32x4e*>(a.udbar)[i];
  f32x4e ub = reinterpret_cast<const f32x4e*>(a.ubar)[i];
  f32x4e ps = {0.f, 0.f, 0.f, 0.f};
  if (a.psi) ps = reinterpret_cast<const f32x4e*>(a.psi)[i];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float g = diff_dD(u[c], a.d1, a.d2) * A[c];
    if (a.psi) g -= ps[c];
    ub[c] += g * sd[c];
    sd[c] = diff_D(u[c], a.d0, a.d1, a.d2) * sd[c];
  }
  reinterpret_cast<f32x4e*>(a.ubar)[i] = ub;
  reinterpret_cast<f32x4e*>(a.udbar)[i] = sd;
}

__global__ __launch_bounds__(256) void vn_nldiff_source_kernel(VnNldiffDedupArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  const long j = a.uid[r];                                     // (validated against U by vn_set_dedup)
  const int p = (int)(r % a.q);
  const long gr = a.gper ? p : r;                              // periodic gcoef: the table = the rows of test function 0
  const float base = a.base ? a.base[r] : 0.f;
  const f32x4e pd = *reinterpret_cast<const f32x4e*>(a.upack + j * 4);
  float A = 0.f;
  for (int d = 0; d < a.dim; ++d) A += pd[1 + d] * a.gcoef[gr * a.dim + d];
  float t = (1.f - diff_D(pd[0], a.d0, a.d1, a.d2)) * A;
  if (a.psi) t += pd[0] * a.psi[r];
  // vn_dedup_seed_kernel multiplies its source by N_p (non-zero: checked on the host against the table of vn_set_fe_table)
  a.s_eff[r] = base + t / a.feN[p];
}

// A point has 2^feDim rows on a uniform grid (<= 8): four entries in flight per thread -- all row indices, then all dependent
// loads, then the additions in CSR order.
__global__ __launch_bounds__(256) void vn_nldiff_point_kernel(VnNldiffDedupArgs a) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.U) return;
  const int q = a.q, dim = a.dim;
  const f32x4e pd = *reinterpret_cast<const f32x4e*>(a.upack + j * 4);
  float acc = 0.f;
  if (a.psi) {
    const bool qpow2 = (q & (q - 1)) == 0;
    const int qshift = __ffs(q) - 1;
    const int e0 = a.rowptr[j], e1 = a.rowptr[j + 1];
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
        float t = a.psi[ru] * a.stf[k];
        if (a.feW) t *= a.feW[p];
        v[c] = r[c] >= 0 ? t : 0.f;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (r[c] >= 0) acc += v[c];
    }
  }
  const float D = diff_D(pd[0], a.d0, a.d1, a.d2);
  float gs = 0.f;
  for (int d = 0; d < dim; ++d) {
    const float sg = a.seed_g[j * dim + d];
    gs += pd[1 + d] * sg;
    a.seed_g[j * dim + d] = D * sg;
  }
  a.seed_u[j] = a.seed_u[j] + diff_dD(pd[0], a.d1, a.d2) * gs - acc;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t vn_nldiff_fold_launch(const VnNldiffRowArgs& a, hipStream_t s) {
  if (a.nT <= 0) return hipSuccess;
  if (a.nT % 4 == 0 && aligned16(a.u) && aligned16(a.psi) && aligned16(a.ud) && aligned16(a.A))
    hipLaunchKernelGGL(vn_nldiff_fold4_kernel, dim3((unsigned)((a.nT / 4 + 255) / 256)), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(vn_nldiff_fold_kernel, dim3((unsigned)((a.nT + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_nldiff_seed_launch(const VnNldiffRowArgs& a, hipStream_t s) {
  if (a.nT <= 0) return hipSuccess;
  if (a.nT % 4 == 0 && aligned16(a.u) && aligned16(a.psi) && aligned16(a.A) && aligned16(a.udbar) && aligned16(a.ubar))
    hipLaunchKernelGGL(vn_nldiff_seed4_kernel, dim3((unsigned)((a.nT / 4 + 255) / 256)), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(vn_nldiff_seed_kernel, dim3((unsigned)((a.nT + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_nldiff_source_launch(const VnNldiffDedupArgs& a, hipStream_t s) {
  if (a.nT <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_nldiff_source_kernel, dim3((unsigned)((a.nT + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_nldiff_point_launch(const VnNldiffDedupArgs& a, hipStream_t s) {
  if (a.U <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_nldiff_point_kernel, dim3((unsigned)((a.U + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}
