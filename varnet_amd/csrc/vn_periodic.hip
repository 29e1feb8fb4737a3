// Periodic boundary pairs (vn_set_periodic): P = mean_P[ biDimVal (r0^2 + gamma r1^2) ] over the pairs (i, i + nP) of the
// registered rows, r0 the jump of the value and r1 the jump of the derivative along the pair's common direction.  The rows take
// the route of the boundary-flux rows (vn_api.hip, periodic_pass): the generic forward kernel with the directions as tangents,
// this seed kernel, the generic reverse kernel into partials of their own, and one more operand of the step's reduction.
#include "vn_periodic.h"

namespace {

constexpr int PER_TB = 256;

// the order of vn_generic.hip's block_sum: a shuffle tree per wave, then the four wave sums left to right
__device__ __forceinline__ float per_block_sum(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// One thread per pair, one loss partial per block (folded by vn_reduce_kernel in a fixed order).
__global__ __launch_bounds__(PER_TB) void vn_periodic_seed_kernel(VnPeriodicSeedArgs a) {
  __shared__ float red[4];
  const long i = (long)blockIdx.x * PER_TB + threadIdx.x;
  float e2 = 0.f;
  if (i < a.nP) {
    const long j = i + a.nP;
    const float r0 = a.u[i] - a.u[j];
    const float r1 = a.ud ? a.ud[i] - a.ud[j] : 0.f;           // gamma == 0: no tangent stream was computed
    e2 = a.biDimVal * (r0 * r0 + a.gamma * r1 * r1);
    if (a.ubar) {
      const float s = 2.f * a.w0 * a.biDimVal / (float)a.nP;
      const float sv = s * r0, sd = s * a.gamma * r1;
      a.ubar[i] = sv; a.ubar[j] = -sv;
      if (a.udbar) { a.udbar[i] = sd; a.udbar[j] = -sd; }
    }
  }
  const float t = per_block_sum(e2, red);
  if (threadIdx.x == 0) a.part[blockIdx.x] = t;
}

}  // namespace

int vn_periodic_seed_blocks(long nP) { return (int)((nP + PER_TB - 1) / PER_TB); }

hipError_t vn_periodic_seed_launch(const VnPeriodicSeedArgs& a, hipStream_t s) {
  const int grid = vn_periodic_seed_blocks(a.nP);
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_periodic_seed_kernel, dim3(grid), dim3(PER_TB), 0, s, a);
  return hipGetLastError();
}
