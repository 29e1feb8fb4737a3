// Field identification (vn_set_field_basis, vn_set_field_learn): the tangent direction of a batch is
//   gcoef_r = g0_r + sum_j b_j G_j[r, :]   over J <= 32 per-row basis streams of dim floats per row
// (G_j = chi_j dN/dx for a diffusivity stream, omega_j N for a velocity stream; the engine does not know which is which), and the
// amplitudes b_j are learnt next to the parameters.  The row integrand is linear in gcoef through A_r = grad u_r . gcoef_r
// (t_r = D(u_r) A_r - ..., D = 1 without vn_set_nldiff), so with s_r the tangent seed the reverse pass consumes (udbar[r] AFTER
// vn_nldiff_seed_kernel rescaled it by D(u_r) -- unlike vn_source.hip, which reads it before):
//   d loss / d b_j = + sum_r s_r (grad u_r . G_j[r, :])
// On the de-duplicated step s_r = stf[r / q] W_p D(u_j), j = uid[r], and grad u is that of point j.
// The mix gcoef = g0 + G^T b and the fold / Adam step / clamp are vn_source.hip's kernels (the mix over nT dim entries per
// stream); the reduction is here:
//   vn_fldgrad_rows_kernel<DIM>   the J sums.  Grid (row blocks <= 256, ceil(J / 8)): a workgroup carries eight streams in eight
//                                 accumulators per thread (compile-time indices: no scratch at any J), a grid-stride loop over a
//                                 capped grid so every partial covers a fixed set of rows, per block the order of block_sum
//                                 (vn_blocksum.h).  Per row: the seed, one 16-byte (u, grad u) record, DIM floats per stream.
// One [blocks, J] partial array.  No atomics, plain vector stores: two evaluations give the same bits.
#include <cstdint>

#include "vn_blocksum.h"
#include "vn_field.h"

namespace {

typedef float f32x4t __attribute__((ext_vector_type(4)));
constexpr int TB = 256;
constexpr int JG = VN_FLD_JG;

// the learnt streams of this workgroup's group of eight, as bits 0..7
__device__ __forceinline__ unsigned group_mask(const VnFldGradArgs& a, int j0) {
  const int left = a.J - j0;
  const unsigned in = left >= JG ? 0xFFu : (1u << left) - 1u;
  return (a.mask >> j0) & in;
}

template <int DIM>
__global__ __launch_bounds__(TB) void vn_fldgrad_rows_kernel(VnFldGradArgs a) {
  __shared__ float red[4];
  const int j0 = blockIdx.y * JG;
  const unsigned m = group_mask(a, j0);
  const long stride = a.nT * DIM;                                // floats between two streams
  float c0 = 1.f, c1 = 0.f, c2 = 0.f;
  if (a.nldiff) {
    if (a.cp) { c0 = a.cp[0]; c1 = a.cp[1]; c2 = a.cp[2]; }
    else { c0 = a.c[0]; c1 = a.c[1]; c2 = a.c[2]; }
  }
  float acc[JG] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m)
    for (long r = (long)blockIdx.x * TB + threadIdx.x; r < a.nT; r += (long)gridDim.x * TB) {
      const long j = a.uid ? (long)a.uid[r] : r;                 // (uid validated against U by vn_set_dedup)
      const f32x4t pd = *reinterpret_cast<const f32x4t*>(a.pack + j * 4);
      float s;
      if (a.udbar) {
        s = a.udbar[r];
      } else {
        s = a.stf[r / a.q];
        if (a.feW) s *= a.feW[r % a.q];
        if (a.nldiff) s *= c0 + pd[0] * (c1 + pd[0] * c2);       // D(u_j), the form of quad() in vn_terms.hip
      }
      float w[DIM];
#pragma unroll
      for (int d = 0; d < DIM; ++d) w[d] = s * pd[1 + d];
#pragma unroll
      for (int c = 0; c < JG; ++c)
        if (m >> c & 1u) {
          const float* g = a.G + (long)(j0 + c) * stride + r * DIM;
#pragma unroll
          for (int d = 0; d < DIM; ++d) acc[c] += w[d] * g[d];
        }
    }
#pragma unroll
  for (int c = 0; c < JG; ++c) {
    float t = 0.f;
    if (m >> c & 1u) t = block_sum(acc[c], red);                 // (m is uniform: every thread takes the same branch)
    if (threadIdx.x == 0 && j0 + c < a.J) a.part[(long)blockIdx.x * a.J + j0 + c] = t;
  }
}

}  // namespace

hipError_t vn_fldgrad_rows_launch(const VnFldGradArgs& a, int* blocks, hipStream_t s) {
  if (a.dim < 1 || a.dim > 3 || a.J < 1 || a.J > VN_FLD_JMAX) return hipErrorInvalidValue;
  const long b = (a.nT + TB - 1) / TB;
  *blocks = (int)(b < 1 ? 1 : b < VN_FLD_MAXBLK ? b : VN_FLD_MAXBLK);
  const dim3 grid((unsigned)*blocks, (unsigned)((a.J + JG - 1) / JG));
  switch (a.dim) {
    case 1: hipLaunchKernelGGL(vn_fldgrad_rows_kernel<1>, grid, dim3(TB), 0, s, a); break;
    case 2: hipLaunchKernelGGL(vn_fldgrad_rows_kernel<2>, grid, dim3(TB), 0, s, a); break;
    default: hipLaunchKernelGGL(vn_fldgrad_rows_kernel<3>, grid, dim3(TB), 0, s, a); break;
  }
  return hipGetLastError();
}
