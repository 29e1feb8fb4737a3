// Source identification (vn_set_source_basis, vn_set_source_learn): the source of a batch is s(r) = s0(r) + sum_j a_j phi_j(r) over
// J <= 64 per-row basis streams, and the amplitudes a_j are learnt next to the parameters.  The source enters the row integrand
// linearly (t_r -= s_r N_p), so with seed_r the tangent seed of row r as vn_seed_kernel writes it (2 w2 detJ R_k W_p, BEFORE
// vn_nldiff_seed_kernel rescales it by D(u)):
//   d loss / d a_j = - sum_r seed_r N_p phi_j[r]
// On the de-duplicated step seed_r = stf[r / q] W_p with stf the per-test-function seed of vn_dedup_seed_kernel.
// Two bandwidth-bound passes over the [J, nT] streams per step:
//   vn_source_mix_kernel     s_mix = s0 + Phi^T a, which every kernel of the step then reads in place of the batch's source;
//   vn_srcgrad_rows_kernel   the J sums.  Grid (row blocks <= 256, ceil(J / 8)): a workgroup carries eight streams in eight
//                            accumulators per thread (compile-time indices: no scratch at any J), a grid-stride loop over a capped
//                            grid so every partial covers a fixed set of rows, per block the order of block_sum (vn_blocksum.h).
//                            The seed stream is re-read once per group of eight: (J + 2 ceil(J / 8)) nT floats at most.
// One [blocks, J] partial array, folded in fp64 in index order by the single block of vn_source_apply_kernel, which also takes
// the Adam step and clamps.  No atomics, plain vector stores: two evaluations give the same bits.
#include <cstdint>
#include <initializer_list>

#include "vn_blocksum.h"
#include "vn_source.h"

namespace {

typedef float f32x4t __attribute__((ext_vector_type(4)));
constexpr int TB = 256;
constexpr int JG = VN_SRC_JG;

__device__ __forceinline__ f32x4t load4(const float* p, long i) { return reinterpret_cast<const f32x4t*>(p)[i]; }

__global__ __launch_bounds__(TB) void vn_source_mix_kernel(VnSrcMixArgs a) {
  const long r = (long)blockIdx.x * TB + threadIdx.x;
  if (r >= a.nT) return;
  float s = a.s0[r];
#pragma unroll 8
  for (int j = 0; j < a.J; ++j) s = fmaf(a.amp[j], a.phi[(long)j * a.nT + r], s);
  a.out[r] = s;
}

__global__ __launch_bounds__(TB) void vn_source_mix4_kernel(VnSrcMixArgs a) {        // nT % 4 == 0, 16-byte aligned pointers
  const long i = (long)blockIdx.x * TB + threadIdx.x, n4 = a.nT / 4;
  if (i >= n4) return;
  f32x4t s = load4(a.s0, i);
#pragma unroll 8
  for (int j = 0; j < a.J; ++j) {
    const float aj = a.amp[j];
    const f32x4t p = load4(a.phi + (long)j * a.nT, i);
    s[0] = fmaf(aj, p[0], s[0]); s[1] = fmaf(aj, p[1], s[1]); s[2] = fmaf(aj, p[2], s[2]); s[3] = fmaf(aj, p[3], s[3]);
  }
  reinterpret_cast<f32x4t*>(a.out)[i] = s;
}

// seed_r N_p of row r
__device__ __forceinline__ float row_weight(const VnSrcGradArgs& a, long r) {
  const int p = (int)(r % a.q);
  const float N = a.Nrow ? a.Nrow[r] : a.feN[p];
  const float s = a.udbar ? a.udbar[r] : (a.feW ? a.stf[r / a.q] * a.feW[p] : a.stf[r / a.q]);
  return s * N;
}

// the learnt streams of this workgroup's group of eight, as bits 0..7
__device__ __forceinline__ unsigned group_mask(const VnSrcGradArgs& a, int j0) {
  const int left = a.J - j0;
  const unsigned in = left >= JG ? 0xFFu : (1u << left) - 1u;
  return (unsigned)(a.mask >> j0) & in;
}

__device__ __forceinline__ void write_partials(const VnSrcGradArgs& a, const float* acc, unsigned m, int j0) {
  __shared__ float red[4];
#pragma unroll
  for (int c = 0; c < JG; ++c) {
    float t = 0.f;
    if (m >> c & 1u) t = block_sum(acc[c], red);                 // (m is uniform: every thread takes the same branch)
    if (threadIdx.x == 0 && j0 + c < a.J) a.part[(long)blockIdx.x * a.J + j0 + c] = -t;   // the source enters with a minus
  }
}

__global__ __launch_bounds__(TB) void vn_srcgrad_rows_kernel(VnSrcGradArgs a) {
  const int j0 = blockIdx.y * JG;
  const unsigned m = group_mask(a, j0);
  float acc[JG] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m)
    for (long r = (long)blockIdx.x * TB + threadIdx.x; r < a.nT; r += (long)gridDim.x * TB) {
      const float w = row_weight(a, r);
#pragma unroll
      for (int c = 0; c < JG; ++c)
        if (m >> c & 1u) acc[c] += w * a.phi[(long)(j0 + c) * a.nT + r];
    }
  write_partials(a, acc, m, j0);
}

__global__ __launch_bounds__(TB) void vn_srcgrad_rows4_kernel(VnSrcGradArgs a) {     // nT % 4 == 0, 16-byte aligned streams
  const int j0 = blockIdx.y * JG;
  const unsigned m = group_mask(a, j0);
  float acc[JG] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m)
    for (long i = (long)blockIdx.x * TB + threadIdx.x; i < a.nT / 4; i += (long)gridDim.x * TB) {
      f32x4t w;
      if (a.udbar && a.Nrow) {
        w = load4(a.udbar, i) * load4(a.Nrow, i);
      } else if (a.udbar) {
        const f32x4t s = load4(a.udbar, i);
        const int p = (int)((4 * i) % a.q);
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = s[c] * a.feN[(p + c) % a.q];
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = row_weight(a, 4 * i + c);
      }
#pragma unroll
      for (int c = 0; c < JG; ++c)
        if (m >> c & 1u) {
          const f32x4t p = load4(a.phi + (long)(j0 + c) * a.nT, i);
          acc[c] += w[0] * p[0]; acc[c] += w[1] * p[1]; acc[c] += w[2] * p[2]; acc[c] += w[3] * p[3];
        }
    }
  write_partials(a, acc, m, j0);
}

// four groups of 64 lanes: lane j < J of group g adds the partials of the blocks [g chunk, (g + 1) chunk) in index order, then
// thread j adds the four group sums in group order
__global__ __launch_bounds__(TB) void vn_source_apply_kernel(VnSrcApplyArgs a) {
  __shared__ double sub[4][VN_SRC_JMAX];
  const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
  if (a.blocks > 0) {
    const int chunk = (a.blocks + 3) / 4;
    const int b1 = (g + 1) * chunk < a.blocks ? (g + 1) * chunk : a.blocks;
    double t = 0.0;
    if (j < a.J)
      for (int b = g * chunk; b < b1; ++b) t += (double)a.part[(long)b * a.J + j];
    sub[g][j] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x >= a.J) return;
  const bool on = a.mask >> j & 1ull;
  double gr = a.grad[j];
  if (a.blocks > 0) {
    gr = 0.0;
    for (int k = 0; k < 4; ++k) gr += sub[k][j];
    if (!on) gr = 0.0;
    a.grad[j] = gr;
  }
  if (a.update && on) {                                        // same arithmetic as vn_adam_kernel, then the clamp
    const float gi = (float)gr;
    const float mi = a.b1 * a.m[j] + (1.f - a.b1) * gi;
    const float vi = a.b2 * a.v[j] + (1.f - a.b2) * gi * gi;
    a.m[j] = mi;
    a.v[j] = vi;
    const float c = a.amp[j] - a.lr_t * mi / (sqrtf(vi) + a.eps);
    a.amp[j] = fminf(fmaxf(c, a.lo[j]), a.hi[j]);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

// The 4-row kernels when nT % 4 == 0 and every stream is 16-byte aligned (nullptr counts; the streams of phi are nT floats
// apart, so its base decides for all of them), else the 1-row kernels: the rule of launch_rows in vn_terms.hip
hipError_t vn_source_mix_launch(const VnSrcMixArgs& a, hipStream_t s) {
  if (a.nT <= 0) return hipSuccess;
  bool four = a.nT % 4 == 0;
  for (const void* p : {(const void*)a.s0, (const void*)a.phi, (const void*)a.out}) four = four && aligned16(p);
  const long n = four ? a.nT / 4 : a.nT;
  hipLaunchKernelGGL(four ? vn_source_mix4_kernel : vn_source_mix_kernel, dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_srcgrad_rows_launch(const VnSrcGradArgs& a, int* blocks, hipStream_t s) {
  bool four = a.nT % 4 == 0 && a.nT > 0;
  for (const void* p : {(const void*)a.udbar, (const void*)a.Nrow, (const void*)a.phi}) four = four && aligned16(p);
  const long n = four ? a.nT / 4 : a.nT, b = (n + TB - 1) / TB;
  *blocks = (int)(b < 1 ? 1 : b < VN_SRC_MAXBLK ? b : VN_SRC_MAXBLK);
  const dim3 grid((unsigned)*blocks, (unsigned)((a.J + JG - 1) / JG));
  hipLaunchKernelGGL(four ? vn_srcgrad_rows4_kernel : vn_srcgrad_rows_kernel, grid, dim3(TB), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_source_apply_launch(const VnSrcApplyArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(vn_source_apply_kernel, dim3(1), dim3(TB), 0, s, a);
  return hipGetLastError();
}
