// Hard-constraint ansatz: the solution is u(x,t) = A(x,t) + B(x,t) n(x,t) with n the network output, A carrying the Dirichlet
// and initial data and B vanishing where they must hold (vn_set_ansatz, vn_set_ansatz_points, vn_set_ansatz_rows).  The map is
// affine in n, so it is an elementwise stage around kernels that exist: the engine carries n_r and one tangent
// nd_r = grad_x n . G_r per row (G: gcoef, a normal, a pair direction, an observation direction), and with the per-row streams
// A_r, B_r, a_r = grad_x A . G_r, b_r = grad_x B . G_r
//   fold      u_r  = A_r + B_r n_r                       ud_r = a_r + b_r n_r + B_r nd_r
//   adjoint   nbar_r = B_r ubar_r + b_r udbar_r          ndbar_r = B_r udbar_r
// Everything between the two sees u, ud and their seeds as it does without an ansatz.  Nothing is saved between them: the
// adjoint needs B and b only.  At the unique points of a de-duplication map the same map acts on the record (u, grad u):
//   fold      u_j = A_j + B_j n_j                        grad u_j = grad A_j + n_j grad B_j + B_j grad n_j
//   adjoint   su_j = B_j su_j + grad B_j . sg_j          sg_j = B_j sg_j            (su reads the sg of before)
// after which the reverse launch with direction sg, tangent seed 1 and value seed su yields the whole gradient:
// dL = su B dn + sg . (grad B dn + B d grad n).
//
// Order contract (the stage helpers of vn_api.hip are the only callers):
//   fold     right after the forward that produced (n, nd), before anything reads them (the terms' fold kernels, the seed kernels);
//   adjoint  last before the reverse pass, after everything that reads or edits seeds with respect to the true u (the terms'
//            seed kernels, the loss weights, the edge sets' seed kernels).
// The results are spelt as fmaf so that the bits do not depend on contraction flags.  Row kernels: four rows per thread with
// 16-byte accesses by the rule of vn_rows4.h, else one row per thread; 256-thread blocks, no LDS; all HBM-bound.
#include "vn_ansatz.h"
#include "vn_rows4.h"

namespace {

__device__ __forceinline__ float fold_u(float A, float B, float n) { return fmaf(B, n, A); }
__device__ __forceinline__ float fold_ud(float a, float b, float B, float n, float nd) { return fmaf(B, nd, fmaf(b, n, a)); }
__device__ __forceinline__ float adj_u(float B, float b, float ubar, float udbar) { return fmaf(b, udbar, B * ubar); }

__device__ __forceinline__ f32x4t load4z(const float* p, long i) {       // a stream that may be nullptr (zero)
  const f32x4t z = {0.f, 0.f, 0.f, 0.f};
  return p ? load4(p, i) : z;
}

__global__ __launch_bounds__(256) void vn_ansatz_fold_kernel(VnAnsatzRowArgs r) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= r.n) return;
  const float n = r.v[i], B = r.B[i];
  r.v[i] = fold_u(r.A ? r.A[i] : 0.f, B, n);
  if (r.vd) r.vd[i] = fold_ud(r.a ? r.a[i] : 0.f, r.b ? r.b[i] : 0.f, B, n, r.vd[i]);
}

__global__ __launch_bounds__(256) void vn_ansatz_fold4_kernel(VnAnsatzRowArgs r) {      // n % 4 == 0, 16-byte aligned pointers
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= r.n / 4) return;
  const f32x4t n = load4(r.v, i), B = load4(r.B, i);
  const f32x4t A = load4z(r.A, i);
  f32x4t u;
#pragma unroll
  for (int c = 0; c < 4; ++c) u[c] = fold_u(A[c], B[c], n[c]);
  store4(r.v, i, u);
  if (r.vd) {
    const f32x4t nd = load4(r.vd, i);
    const f32x4t a = load4z(r.a, i), b = load4z(r.b, i);
    f32x4t ud;
#pragma unroll
    for (int c = 0; c < 4; ++c) ud[c] = fold_ud(a[c], b[c], B[c], n[c], nd[c]);
    store4(r.vd, i, ud);
  }
}

__global__ __launch_bounds__(256) void vn_ansatz_adjoint_kernel(VnAnsatzRowArgs r) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= r.n) return;
  const float B = r.B[i], ub = r.v[i];
  if (!r.vd) { r.v[i] = B * ub; return; }
  const float sd = r.vd[i];
  r.v[i] = adj_u(B, r.b ? r.b[i] : 0.f, ub, sd);
  r.vd[i] = B * sd;
}

__global__ __launch_bounds__(256) void vn_ansatz_adjoint4_kernel(VnAnsatzRowArgs r) {   // n % 4 == 0, 16-byte aligned pointers
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= r.n / 4) return;
  const f32x4t B = load4(r.B, i);
  f32x4t ub = load4(r.v, i);
  if (!r.vd) {
#pragma unroll
    for (int c = 0; c < 4; ++c) ub[c] = B[c] * ub[c];
    store4(r.v, i, ub);
    return;
  }
  f32x4t sd = load4(r.vd, i);
  const f32x4t b = load4z(r.b, i);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    ub[c] = adj_u(B[c], b[c], ub[c], sd[c]);
    sd[c] = B[c] * sd[c];
  }
  store4(r.v, i, ub);
  store4(r.vd, i, sd);
}

// ---- the unique points of a de-duplication map: one point per thread ----
__global__ __launch_bounds__(256) void vn_ansatz_points_fold_kernel(VnAnsatzPointArgs p) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= p.U) return;
  f32x4t pk = load4(p.pack, j);
  const float n = pk[0], B = p.B[j];
  pk[0] = fold_u(p.A ? p.A[j] : 0.f, B, n);
  for (int d = 0; d < p.dim; ++d) {
    const float gA = p.gA ? p.gA[j * p.dim + d] : 0.f, gB = p.gB ? p.gB[j * p.dim + d] : 0.f;
    pk[1 + d] = fold_ud(gA, gB, B, n, pk[1 + d]);
  }
  store4(p.pack, j, pk);
}

__global__ __launch_bounds__(256) void vn_ansatz_points_adjoint_kernel(VnAnsatzPointArgs p) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= p.U) return;
  const float B = p.B[j];
  float su = B * p.seed_u[j];
  for (int d = 0; d < p.dim; ++d) {
    const float sg = p.seed_g[j * p.dim + d];
    if (p.gB) su = fmaf(p.gB[j * p.dim + d], sg, su);
    p.seed_g[j * p.dim + d] = B * sg;
  }
  p.seed_u[j] = su;
}

__global__ __launch_bounds__(256) void vn_ansatz_check_kernel(const float* p, long n, int* err) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n && !isfinite(p[i])) atomicAdd(err, 1);
}

inline dim3 blocks_of(long n) { return dim3((unsigned)((n + 255) / 256)); }

// The 4-row kernel by the rule of vn_rows4.h, else the 1-row kernel
hipError_t launch_rows(void (*k4)(VnAnsatzRowArgs), void (*k1)(VnAnsatzRowArgs), const VnAnsatzRowArgs& r,
                       std::initializer_list<const void*> ptrs, hipStream_t s) {
  if (r.n <= 0) return hipSuccess;
  const bool four = rows4_ok(r.n, ptrs);
  hipLaunchKernelGGL(four ? k4 : k1, blocks_of(four ? r.n / 4 : r.n), dim3(256), 0, s, r);
  return hipGetLastError();
}

}  // namespace

hipError_t vn_ansatz_fold_launch(const VnAnsatzRowArgs& r, hipStream_t s) {
  return launch_rows(vn_ansatz_fold4_kernel, vn_ansatz_fold_kernel, r, {r.A, r.B, r.a, r.b, r.v, r.vd}, s);
}
hipError_t vn_ansatz_adjoint_launch(const VnAnsatzRowArgs& r, hipStream_t s) {
  return launch_rows(vn_ansatz_adjoint4_kernel, vn_ansatz_adjoint_kernel, r, {r.B, r.b, r.v, r.vd}, s);
}

hipError_t vn_ansatz_points_fold_launch(const VnAnsatzPointArgs& p, hipStream_t s) {
  if (p.U <= 0) return hipSuccess;
  if (p.dim < 1 || p.dim > 3) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vn_ansatz_points_fold_kernel, blocks_of(p.U), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t vn_ansatz_points_adjoint_launch(const VnAnsatzPointArgs& p, hipStream_t s) {
  if (p.U <= 0) return hipSuccess;
  if (p.dim < 1 || p.dim > 3) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vn_ansatz_points_adjoint_kernel, blocks_of(p.U), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t vn_ansatz_check_launch(const float* p, long n, int* err_dev, hipStream_t s) {
  if (!p || n <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_ansatz_check_kernel, blocks_of(n), dim3(256), 0, s, p, n, err_dev);
  return hipGetLastError();
}
