// Inverse mode (vn_set_coef_learn): the gradient of the loss with respect to the nine polynomial coefficients of vn_terms.hip
// and their optimizer step.  Coefficient index: 0..2 = (c1, c2, c3) reaction, 3..5 = (f1, f2, f3) flux, 6..8 = (d0, d1, d2) D(u).
// With s_r the tangent seed of row r as vn_seed_kernel writes it (2 w2 detJ R_k W_p, BEFORE vn_nldiff_seed_kernel rescales it by
// D(u)) and u_r, A_r, N_p, rate_r, phi_r as in vn_terms.hip's header, only the variational term contains the coefficients:
//   row-wise            d loss / d c_m = - sum_r s_r N_p rate_r u_r^m      m = 1, 2, 3   (rate_r = 1 when the stream is null)
//                       d loss / d f_m = - sum_r s_r phi_r u_r^m           m = 1, 2, 3
//                       d loss / d d_m = + sum_r s_r A_r u_r^m             m = 0, 1, 2
//   de-duplicated step  d loss / d c_m = - sum_j u_j^m accR_j,  d loss / d f_m = - sum_j u_j^m accF_j,  d loss / d d_m = + sum_j u_j^m gs_j
//                       with accR_j, accF_j the CSR sums of vn_react_gather_kernel / vn_nlflux_gather_kernel and gs_j the dot product
//                       grad u_j . seed_g[j,:] of vn_nldiff_point_kernel (unscaled seed_g), which those kernels store: no second walk.
// Both reductions are grid-stride loops over a capped grid, so every partial covers a fixed set of rows; fp32 accumulators per
// thread, for the masked entries only; per block the order of block_sum (vn_blocksum.h); one [blocks, 9] partial array, folded
// in fp64 in index order by the single block of vn_coef_apply_kernel.  No atomics, plain vector stores: two evaluations give the
// same bits.  HBM-bound: at most five 4-byte streams per row (u, s, rate, phi, A).
#include <cstdint>
#include <initializer_list>

#include "vn_blocksum.h"
#include "vn_coef.h"

namespace {

typedef float f32x4t __attribute__((ext_vector_type(4)));
constexpr int TB = 256;

__device__ __forceinline__ f32x4t load4(const float* p, long i) { return reinterpret_cast<const f32x4t*>(p)[i]; }

// acc[3 g + m] += w x^(m + first) for the masked entries of group g
__device__ __forceinline__ void add_powers(float* acc, unsigned mask, int g, float w, float x, bool from_one) {
  float p = from_one ? w * x : w;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    if (mask >> (3 * g + m) & 1u) acc[3 * g + m] += p;
    p *= x;
  }
}

__device__ __forceinline__ void add_row(const VnCoefRowsArgs& a, float* acc, long r, float u, float s, float rate, float phi, float A) {
  if (a.react && (a.mask & 0x7u)) {
    const float N = a.Nrow ? a.Nrow[r] : a.feN[r % a.q];
    add_powers(acc, a.mask, 0, a.rate ? s * N * rate : s * N, u, true);
  }
  if (a.phi && (a.mask & 0x38u)) add_powers(acc, a.mask, 1, s * phi, u, true);
  if (a.A && (a.mask & 0x1C0u)) add_powers(acc, a.mask, 2, s * A, u, false);
}

// signs: the reaction and the flux enter the row integrand with a minus
__device__ __forceinline__ void write_partials(float* acc, unsigned mask, float* part) {
  __shared__ float red[4];
#pragma unroll
  for (int i = 0; i < VN_COEF_N; ++i) {
    float t = 0.f;
    if (mask >> i & 1u) t = block_sum(acc[i], red);           // (mask is uniform: every thread takes the same branch)
    if (threadIdx.x == 0) part[(long)blockIdx.x * VN_COEF_N + i] = i < 6 ? -t : t;
  }
}

__global__ __launch_bounds__(TB) void vn_coefgrad_rows_kernel(VnCoefRowsArgs a) {
  float acc[VN_COEF_N] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool wr = a.react && a.rate && (a.mask & 0x7u), wf = a.phi && (a.mask & 0x38u), wd = a.A && (a.mask & 0x1C0u);
  for (long r = (long)blockIdx.x * TB + threadIdx.x; r < a.nT; r += (long)gridDim.x * TB)
    add_row(a, acc, r, a.u[r], a.udbar[r], wr ? a.rate[r] : 1.f, wf ? a.phi[r] : 0.f, wd ? a.A[r] : 0.f);
  write_partials(acc, a.mask, a.part);
}

__global__ __launch_bounds__(TB) void vn_coefgrad_rows4_kernel(VnCoefRowsArgs a) {     // nT % 4 == 0, 16-byte aligned pointers
  float acc[VN_COEF_N] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool wr = a.react && a.rate && (a.mask & 0x7u), wf = a.phi && (a.mask & 0x38u), wd = a.A && (a.mask & 0x1C0u);
  const f32x4t zero = {0.f, 0.f, 0.f, 0.f}, one = {1.f, 1.f, 1.f, 1.f};
  for (long i = (long)blockIdx.x * TB + threadIdx.x; i < a.nT / 4; i += (long)gridDim.x * TB) {
    const f32x4t u = load4(a.u, i), s = load4(a.udbar, i);
    const f32x4t rt = wr ? load4(a.rate, i) : one, ph = wf ? load4(a.phi, i) : zero, A = wd ? load4(a.A, i) : zero;
#pragma unroll
    for (int c = 0; c < 4; ++c) add_row(a, acc, 4 * i + c, u[c], s[c], rt[c], ph[c], A[c]);
  }
  write_partials(acc, a.mask, a.part);
}

__global__ __launch_bounds__(TB) void vn_coefgrad_points_kernel(VnCoefPointsArgs a) {
  float acc[VN_COEF_N] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long j = (long)blockIdx.x * TB + threadIdx.x; j < a.U; j += (long)gridDim.x * TB) {
    const float u = a.upack[j * 4];
    if (a.accR && (a.mask & 0x7u)) add_powers(acc, a.mask, 0, a.accR[j], u, true);
    if (a.accF && (a.mask & 0x38u)) add_powers(acc, a.mask, 1, a.accF[j], u, true);
    if (a.gs && (a.mask & 0x1C0u)) add_powers(acc, a.mask, 2, a.gs[j], u, false);
  }
  write_partials(acc, a.mask, a.part);
}

// 16 groups of 16 lanes: lane i < 9 of group g adds the partials of the blocks [g chunk, (g + 1) chunk) in index order, then
// thread i adds the sixteen group sums in group order
__global__ __launch_bounds__(TB) void vn_coef_apply_kernel(VnCoefApplyArgs a) {
  __shared__ double sub[16][16];
  const int i = threadIdx.x & 15, g = threadIdx.x >> 4;
  if (a.blocks > 0) {
    const int chunk = (a.blocks + 15) / 16;
    const int b1 = (g + 1) * chunk < a.blocks ? (g + 1) * chunk : a.blocks;
    double t = 0.0;
    if (i < VN_COEF_N)
      for (int b = g * chunk; b < b1; ++b) t += (double)a.part[(long)b * VN_COEF_N + i];
    sub[g][i] = t;
  }
  __syncthreads();
  if (threadIdx.x >= VN_COEF_N) return;
  const bool on = a.mask >> i & 1u;
  double gr = a.grad[i];
  if (a.blocks > 0) {
    gr = 0.0;
    for (int k = 0; k < 16; ++k) gr += sub[k][i];
    if (!on) gr = 0.0;
    a.grad[i] = gr;
  }
  if (a.update && on) {                                        // same arithmetic as vn_adam_kernel, then the clamp
    const float gi = (float)gr;
    const float mi = a.b1 * a.m[i] + (1.f - a.b1) * gi;
    const float vi = a.b2 * a.v[i] + (1.f - a.b2) * gi * gi;
    a.m[i] = mi;
    a.v[i] = vi;
    const float c = a.coef[i] - a.lr_t * mi / (sqrtf(vi) + a.eps);
    a.coef[i] = fminf(fmaxf(c, a.lo[i]), a.hi[i]);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

int vn_coefgrad_blocks(long n) {
  const long b = (n + TB - 1) / TB;
  return (int)(b < 1 ? 1 : b < VN_COEF_MAXBLK ? b : VN_COEF_MAXBLK);
}

// The 4-row kernel when nT % 4 == 0 and every stream is 16-byte aligned (nullptr counts), else the 1-row kernel: the rule of
// launch_rows in vn_terms.hip
hipError_t vn_coefgrad_rows_launch(const VnCoefRowsArgs& a, int* blocks, hipStream_t s) {
  bool four = a.nT % 4 == 0;
  for (const void* p : {(const void*)a.u, (const void*)a.udbar, (const void*)a.rate, (const void*)a.phi, (const void*)a.A})
    four = four && aligned16(p);
  *blocks = vn_coefgrad_blocks(four ? a.nT / 4 : a.nT);
  hipLaunchKernelGGL(four ? vn_coefgrad_rows4_kernel : vn_coefgrad_rows_kernel, dim3((unsigned)*blocks), dim3(TB), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_coefgrad_points_launch(const VnCoefPointsArgs& a, int* blocks, hipStream_t s) {
  *blocks = vn_coefgrad_blocks(a.U);
  hipLaunchKernelGGL(vn_coefgrad_points_kernel, dim3((unsigned)*blocks), dim3(TB), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_coef_apply_launch(const VnCoefApplyArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(vn_coef_apply_kernel, dim3(1), dim3(TB), 0, s, a);
  return hipGetLastError();
}
