// The three polynomial terms of the PDE
//     c_t = div(kappa D(c) grad c) - v.grad c - div(w F(c)) + s + rate p(c)
//   reaction     rate(x,t) p(c),    p(c) = c1 c + c2 c^2 + c3 c^3                        (vn_set_reaction)
//   flux         -div(w(x,t) F(c)), F(c) = f1 c + f2 c^2 + f3 c^3 (Burgers: w = 1, F = c^2 / 2)   (vn_set_nlflux)
//   diffusivity  D(c) = d0 + d1 c + d2 c^2 (porous medium: D = c^m)                      (vn_set_nldiff)
// outside the kernels that carry them inline (the row-wise reaction: vn_seed_kernel; all three in fp64: vn_obj64_seed_kernel).
// All kernels here are HBM-bound and small.  With u_r the network value of row r, A_r = sum_d u_{x_d} gcoef_d its one tangent
// and s_r its tangent seed:
//   reaction  depends on the VALUE only: the row integrand gains -rate_r p(u_r) N_p like a source term (TFModel.py:657).
//   flux      integrates by parts onto the test function, so again only the value enters: with phi_r = sum_d w_d dN_r/dx_d the
//             row integrand gains -F(u_r) phi_r and the value seed -phi_r F'(u_r) s_r.
//   D(u)      must scale the diffusion part only, so on a batch with the term gcoef = kappa dN/dx and the advection moves to the
//             value side: int v.grad u N = -int u psi, psi_r = sum_d v_d dN_r/dx_d + N_r div v.  The row integrand starts from
//             D(u_r) A_r - u_r psi_r instead of A_r;  value seed += (D'(u_r) A_r - psi_r) s_r,  tangent seed = D(u_r) s_r.
//             Nothing divides by D(u): D(0) = 0 (porous medium) is a regular point.
//
// Ordering contract (the four stage helpers of vn_api.hip are the only callers):
//   row-wise routes, around vn_seed_kernel, which starts the row integrand from ud[r] and adds every later term to it:
//     vn_nldiff_fold_kernel   A[r] = ud[r]; ud[r] = D(u_r) A[r] - u_r psi_r      first: before anything else edits ud
//     vn_nlflux_fold_kernel   ud[r] -= F(u_r) phi_r
//     vn_seed_kernel          (carries the reaction)
//     vn_nlflux_seed_kernel   ubar[r] -= phi_r F'(u_r) udbar[r]                  (udbar[r] already carries W_p)
//     vn_nldiff_seed_kernel   ubar[r] += (D'(u_r) A[r] - psi_r) udbar[r]; udbar[r] *= D(u_r)
//                                                                                last: the flux seed reads the unscaled udbar
//     One row per thread, or four rows per thread (fold4 / seed4) with 16-byte accesses when nT and the pointers allow.
//   de-duplicated step, around vn_dedup_seed_kernel / vn_dedup_gather_kernel; every term is evaluated once per unique point j:
//     vn_react_source_kernel, vn_nlflux_source_kernel, vn_nldiff_source_kernel, in this order, one row per thread, each adding
//       its share to what the previous one left in s_eff (vn_terms.h) -- handed to vn_dedup_seed_kernel as its `source`, which
//       subtracts s_eff N_p from the row integrand;
//     vn_dedup_seed_kernel, vn_dedup_gather_kernel;
//     vn_react_gather_kernel, vn_nlflux_gather_kernel   one unique point per thread: the term's value seed, a sum over the rows
//       of the point in CSR order (fixed order: bitwise repeatable), added to what vn_dedup_gather_kernel stored;
//     vn_nldiff_point_kernel  last: seed_g[j,:] = sum_r W_p gcoef_r stf[k_r] is what the rows' tangent seeds add up to, so
//       d loss / d u_j += D'(u_j) (grad u_j . seed_g[j,:]) needs the unscaled seed_g and no gather, then seed_g[j,:] *= D(u_j);
//       only -sum_r W_p psi_r stf[k_r] walks the rows of the point.
//
// Inverse mode (vn_set_coef_learn): every kernel takes its three coefficients from the argument `cp` when it is given -- the engine's
// device vector, which the optimizer step updates -- and from the by-value `c` otherwise; the gather and point kernels store their
// per-point sum (accR_j, accF_j, gs_j) to `acc_out` when it is given, for the coefficient reduction of vn_learnt.hip.  With both null
// code path and arithmetic are unchanged.
#include "vn_internal.h"
#include "vn_rows4.h"
#include "vn_terms.h"

namespace {

// c[0] + c[1] u + c[2] u^2 is D(u); u times it is p(u) and F(u)
__device__ __forceinline__ float quad(float u, const float* c) { return c[0] + u * (c[1] + u * c[2]); }
__device__ __forceinline__ float dquad(float u, const float* c) { return c[1] + 2.f * c[2] * u; }
__device__ __forceinline__ float cubic(float u, const float* c) { return u * quad(u, c); }
__device__ __forceinline__ float dcubic(float u, const float* c) { return c[0] + u * (2.f * c[1] + 3.f * c[2] * u); }

// The three coefficients of a term: the engine's device vector while the coefficients are learnt (vn_set_coef_learn: cp), else
// the by-value ones.  Either way three floats in registers before the first use: the arithmetic after it is the same.
struct Coef3 { float c[3]; };
template <class Args>
__device__ __forceinline__ Coef3 coef3(const Args& a) {
  Coef3 k;
  if (a.cp) { k.c[0] = a.cp[0]; k.c[1] = a.cp[1]; k.c[2] = a.cp[2]; }
  else { k.c[0] = a.c[0]; k.c[1] = a.c[1]; k.c[2] = a.c[2]; }
  return k;
}

// ---- row-wise routes ----
__global__ __launch_bounds__(256) void vn_nlflux_fold_kernel(VnTermRowArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  const Coef3 k = coef3(a);
  a.ud[r] -= cubic(a.u[r], k.c) * a.stream[r];
}

__global__ __launch_bounds__(256) void vn_nlflux_fold4_kernel(VnTermRowArgs a) {      // nT % 4 == 0, 16-byte aligned pointers
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nT / 4) return;
  const Coef3 k = coef3(a);
  const f32x4t u = load4(a.u, i), ph = load4(a.stream, i);
  f32x4t ud = load4(a.ud, i);
#pragma unroll
  for (int c = 0; c < 4; ++c) ud[c] -= cubic(u[c], k.c) * ph[c];
  store4(a.ud, i, ud);
}

__global__ __launch_bounds__(256) void vn_nlflux_seed_kernel(VnTermRowArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  const Coef3 k = coef3(a);
  a.ubar[r] -= a.stream[r] * dcubic(a.u[r], k.c) * a.udbar[r];
}

__global__ __launch_bounds__(256) void vn_nlflux_seed4_kernel(VnTermRowArgs a) {      // nT % 4 == 0, 16-byte aligned pointers
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nT / 4) return;
  const Coef3 k = coef3(a);
  const f32x4t u = load4(a.u, i), ph = load4(a.stream, i), sd = load4(a.udbar, i);
  f32x4t ub = load4(a.ubar, i);
#pragma unroll
  for (int c = 0; c < 4; ++c) ub[c] -= ph[c] * dcubic(u[c], k.c) * sd[c];
  store4(a.ubar, i, ub);
}

__global__ __launch_bounds__(256) void vn_nldiff_fold_kernel(VnTermRowArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  const Coef3 k = coef3(a);
  const float u = a.u[r], A = a.ud[r];
  a.A[r] = A;
  float t = quad(u, k.c) * A;
  if (a.stream) t -= u * a.stream[r];
  a.ud[r] = t;
}

__global__ __launch_bounds__(256) void vn_nldiff_fold4_kernel(VnTermRowArgs a) {      // nT % 4 == 0, 16-byte aligned pointers
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nT / 4) return;
  const Coef3 k = coef3(a);
  const f32x4t u = load4(a.u, i), A = load4(a.ud, i);
  f32x4t ps = {0.f, 0.f, 0.f, 0.f};
  if (a.stream) ps = load4(a.stream, i);
  f32x4t t;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    t[c] = quad(u[c], k.c) * A[c];
    if (a.stream) t[c] -= u[c] * ps[c];
  }
  store4(a.A, i, A);
  store4(a.ud, i, t);
}

__global__ __launch_bounds__(256) void vn_nldiff_seed_kernel(VnTermRowArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  const Coef3 k = coef3(a);
  const float u = a.u[r], sd = a.udbar[r];
  float g = dquad(u, k.c) * a.A[r];
  if (a.stream) g -= a.stream[r];
  a.ubar[r] += g * sd;
  a.udbar[r] = quad(u, k.c) * sd;
}

__global__ __launch_bounds__(256) void vn_nldiff_seed4_kernel(VnTermRowArgs a) {      // nT % 4 == 0, 16-byte aligned pointers
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nT / 4) return;
  const Coef3 k = coef3(a);
  const f32x4t u = load4(a.u, i), A = load4(a.A, i);
  f32x4t sd = load4(a.udbar, i), ub = load4(a.ubar, i);
  f32x4t ps = {0.f, 0.f, 0.f, 0.f};
  if (a.stream) ps = load4(a.stream, i);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float g = dquad(u[c], k.c) * A[c];
    if (a.stream) g -= ps[c];
    ub[c] += g * sd[c];
    sd[c] = quad(u[c], k.c) * sd[c];
  }
  store4(a.ubar, i, ub);
  store4(a.udbar, i, sd);
}

// ---- de-duplicated step ----
__global__ __launch_bounds__(256) void vn_react_source_kernel(VnTermDedupArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  const Coef3 k = coef3(a);
  const long j = a.uid[r];                                     // (validated against U by vn_set_dedup)
  const float base = a.base ? a.base[r] : 0.f;
  const float rho = a.stream ? a.stream[r] : 1.f;
  const float pu = cubic(a.upack[j * 4], k.c);
  a.s_eff[r] = base + (a.stream ? rho * pu : pu);
}

__global__ __launch_bounds__(256) void vn_nlflux_source_kernel(VnTermDedupArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  const Coef3 k = coef3(a);
  const long j = a.uid[r];                                     // (validated against U by vn_set_dedup)
  const int p = (int)(r % a.q);
  const float base = a.base ? a.base[r] : 0.f;
  const float u = a.upack[j * 4];
  // vn_dedup_seed_kernel multiplies its source by N_p (non-zero: checked on the host against the table of vn_set_fe_table)
  a.s_eff[r] = base + cubic(u, k.c) * a.stream[r] / a.feN[p];
}

__global__ __launch_bounds__(256) void vn_nldiff_source_kernel(VnTermDedupArgs a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.nT) return;
  const Coef3 k = coef3(a);
  const long j = a.uid[r];                                     // (validated against U by vn_set_dedup)
  const int p = (int)(r % a.q);
  const long gr = a.gper ? p : r;                              // periodic gcoef: the table = the rows of test function 0
  const float base = a.base ? a.base[r] : 0.f;
  const f32x4t pd = *reinterpret_cast<const f32x4t*>(a.upack + j * 4);
  float A = 0.f;
  for (int d = 0; d < a.dim; ++d) A += pd[1 + d] * a.gcoef[gr * a.dim + d];
  float t = (1.f - quad(pd[0], k.c)) * A;
  if (a.stream) t += pd[0] * a.stream[r];
  // N_p non-zero, as for the flux term
  a.s_eff[r] = base + t / a.feN[p];
}

// sum over the rows r of unique point j, in CSR order, of term(r, k, p): k = r / q the row's test function, p = r % q its
// quadrature point.  A point has up to 2^feDim rows on a uniform grid (8 in 2D+t, 16 in 3D+t) and any number on a caller-built
// map (one thread then walks them all): four entries in flight per thread and pass -- all row indices, then all dependent loads,
// then the additions in CSR order.
template <class Term>
__device__ __forceinline__ float csr_walk(const VnTermDedupArgs& a, long j, Term term) {
  const int q = a.q;
  const bool qpow2 = (q & (q - 1)) == 0;
  const int qshift = __ffs(q) - 1;
  const int e0 = a.rowptr[j], e1 = a.rowptr[j + 1];
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
      const float t = term(ru, k, p);
      v[c] = r[c] >= 0 ? t : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (r[c] >= 0) acc += v[c];
  }
  return acc;
}

// W_p stream[r] stf[k]: the row term of the flux gather (stream = phi) and of the D(u) point kernel (stream = psi)
__device__ __forceinline__ float stream_term(const VnTermDedupArgs& a, unsigned ru, unsigned k, unsigned p) {
  float t = a.stream[ru] * a.stf[k];
  if (a.feW) t *= a.feW[p];
  return t;
}

__global__ __launch_bounds__(256) void vn_react_gather_kernel(VnTermDedupArgs a) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.U) return;
  const Coef3 k = coef3(a);
  const float u = a.upack[j * 4];
  const float su = a.seed_u[j];
  const float acc = csr_walk(a, j, [&a](unsigned ru, unsigned k, unsigned p) {
    float t = a.feN[p] * a.stf[k];
    if (a.feW) t *= a.feW[p];
    if (a.stream) t *= a.stream[ru];
    return t;
  });
  if (a.acc_out) a.acc_out[j] = acc;                          // vn_coefgrad_points_kernel reads it (vn_set_coef_learn)
  a.seed_u[j] = su - dcubic(u, k.c) * acc;
}

__global__ __launch_bounds__(256) void vn_nlflux_gather_kernel(VnTermDedupArgs a) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.U) return;
  const Coef3 k = coef3(a);
  const float u = a.upack[j * 4];
  const float su = a.seed_u[j];
  const float acc = csr_walk(a, j, [&a](unsigned ru, unsigned k, unsigned p) { return stream_term(a, ru, k, p); });
  if (a.acc_out) a.acc_out[j] = acc;                          // vn_coefgrad_points_kernel reads it (vn_set_coef_learn)
  a.seed_u[j] = su - dcubic(u, k.c) * acc;
}

__global__ __launch_bounds__(256) void vn_nldiff_point_kernel(VnTermDedupArgs a) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.U) return;
  const Coef3 k = coef3(a);
  const int dim = a.dim;
  const f32x4t pd = *reinterpret_cast<const f32x4t*>(a.upack + j * 4);
  float acc = 0.f;
  if (a.stream) acc = csr_walk(a, j, [&a](unsigned ru, unsigned k, unsigned p) { return stream_term(a, ru, k, p); });
  const float D = quad(pd[0], k.c);
  float gs = 0.f;
  for (int d = 0; d < dim; ++d) {
    const float sg = a.seed_g[j * dim + d];
    gs += pd[1 + d] * sg;
    a.seed_g[j * dim + d] = D * sg;
  }
  if (a.acc_out) a.acc_out[j] = gs;                           // ... the dot product with the unscaled seed_g
  a.seed_u[j] = a.seed_u[j] + dquad(pd[0], k.c) * gs - acc;
}

// ---- launches ----
// The 4-row kernel by the rule of vn_rows4.h, else the 1-row kernel
hipError_t launch_rows(void (*k4)(VnTermRowArgs), void (*k1)(VnTermRowArgs), const VnTermRowArgs& a,
                       std::initializer_list<const void*> ptrs, hipStream_t s) {
  if (a.nT <= 0) return hipSuccess;
  const bool four = rows4_ok(a.nT, ptrs);
  const long n = four ? a.nT / 4 : a.nT;
  hipLaunchKernelGGL(four ? k4 : k1, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// One thread per row (n = nT) or per unique point (n = U)
hipError_t launch_each(void (*k)(VnTermDedupArgs), long n, const VnTermDedupArgs& a, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t vn_nlflux_fold_launch(const VnTermRowArgs& a, hipStream_t s) {
  return launch_rows(vn_nlflux_fold4_kernel, vn_nlflux_fold_kernel, a, {a.u, a.stream, a.ud}, s);
}
hipError_t vn_nlflux_seed_launch(const VnTermRowArgs& a, hipStream_t s) {
  return launch_rows(vn_nlflux_seed4_kernel, vn_nlflux_seed_kernel, a, {a.u, a.stream, a.udbar, a.ubar}, s);
}
hipError_t vn_nldiff_fold_launch(const VnTermRowArgs& a, hipStream_t s) {
  return launch_rows(vn_nldiff_fold4_kernel, vn_nldiff_fold_kernel, a, {a.u, a.stream, a.ud, a.A}, s);
}
hipError_t vn_nldiff_seed_launch(const VnTermRowArgs& a, hipStream_t s) {
  return launch_rows(vn_nldiff_seed4_kernel, vn_nldiff_seed_kernel, a, {a.u, a.stream, a.A, a.udbar, a.ubar}, s);
}

hipError_t vn_react_source_launch(const VnTermDedupArgs& a, hipStream_t s) { return launch_each(vn_react_source_kernel, a.nT, a, s); }
hipError_t vn_nlflux_source_launch(const VnTermDedupArgs& a, hipStream_t s) { return launch_each(vn_nlflux_source_kernel, a.nT, a, s); }
hipError_t vn_nldiff_source_launch(const VnTermDedupArgs& a, hipStream_t s) { return launch_each(vn_nldiff_source_kernel, a.nT, a, s); }
hipError_t vn_react_gather_launch(const VnTermDedupArgs& a, hipStream_t s) { return launch_each(vn_react_gather_kernel, a.U, a, s); }
hipError_t vn_nlflux_gather_launch(const VnTermDedupArgs& a, hipStream_t s) { return launch_each(vn_nlflux_gather_kernel, a.U, a, s); }
hipError_t vn_nldiff_point_launch(const VnTermDedupArgs& a, hipStream_t s) { return launch_each(vn_nldiff_point_kernel, a.U, a, s); }
