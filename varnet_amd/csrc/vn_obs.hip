// Observations (vn_set_observations): O = (1/nO) sum_i wgt_i r_i^2, r_i = l_i(u) - value_i, with l_i a linear functional of the
// network over a segment of registered points, l_i = sum_j (q_j u(x_j) + g_j . grad_x u(x_j)).  The points take the route of the
// boundary-flux rows and the periodic pairs (vn_api.hip, obs_pass): the generic forward kernel with the directions g as tangents,
// this seed kernel, the generic reverse kernel into partials of their own, and one more operand of the step's reduction.
#include "vn_obs.h"

namespace {

constexpr int OBS_TB = 256;

// the order of vn_generic.hip's block_sum: a shuffle tree per wave, then the four wave sums left to right
__device__ __forceinline__ float obs_block_sum(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// One thread per observation: its segment in CSR order, four entries in flight and the additions in CSR order (csr_walk of
// vn_terms.hip), then the seeds of the segment's points.  One loss partial per block (folded by vn_reduce_kernel in a fixed order).
__global__ __launch_bounds__(OBS_TB) void vn_obs_seed_kernel(VnObsSeedArgs a) {
  __shared__ float red[4];
  const long i = (long)blockIdx.x * OBS_TB + threadIdx.x;
  float e2 = 0.f;
  if (i < a.nO) {
    const long e0 = a.rowptr ? (long)a.rowptr[i] : i, e1 = a.rowptr ? (long)a.rowptr[i + 1] : i + 1;
    float acc = 0.f;
    for (long e = e0; e < e1; e += 4) {
      float v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool in = e + c < e1;
        const long j = in ? e + c : e0;
        float t = a.q ? a.q[j] * a.u[j] : a.u[j];
        if (a.ud) t += a.ud[j];
        v[c] = in ? t : 0.f;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (e + c < e1) acc += v[c];
    }
    const float w = a.wgt ? a.wgt[i] : 1.f;
    const float r = acc - a.value[i];
    e2 = w * r * r;
    if (a.ubar) {
      const float s = 2.f * a.lambda * w * r / (float)a.nO;
      for (long j = e0; j < e1; ++j) {
        a.ubar[j] = a.q ? s * a.q[j] : s;
        if (a.udbar) a.udbar[j] = s;                        // the direction already carries its coefficient
      }
    }
  }
  const float t = obs_block_sum(e2, red);
  if (threadIdx.x == 0) a.part[blockIdx.x] = t;
}

// Registration check: thread k looks at observation k (k < nO), point k (k < n) and direction entry k (k < n dim).  rowptr is
// read at k and k + 1 <= nO only; a strictly increasing rowptr from 0 to n keeps every later index inside [0, n).
__global__ __launch_bounds__(256) void vn_obs_check_kernel(const float* q, const float* dir, const int* rowptr, const float* value,
                                                           const float* wgt, long n, long nO, long nd, int* err) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  int bad = 0;
  if (k < nO) {
    if (!isfinite(value[k])) ++bad;
    if (wgt && !(isfinite(wgt[k]) && wgt[k] >= 0.f)) ++bad;
    if (rowptr) {
      if (!(rowptr[k] < rowptr[k + 1])) ++bad;
      if (k == 0 && rowptr[0] != 0) ++bad;
      if (k == nO - 1 && (long)rowptr[nO] != n) ++bad;
    }
  }
  if (q && k < n && !isfinite(q[k])) ++bad;
  if (dir && k < nd && !isfinite(dir[k])) ++bad;
  if (bad) atomicAdd(err, bad);
}

}  // namespace

int vn_obs_seed_blocks(long nO) { return (int)((nO + OBS_TB - 1) / OBS_TB); }

hipError_t vn_obs_seed_launch(const VnObsSeedArgs& a, hipStream_t s) {
  const int grid = vn_obs_seed_blocks(a.nO);
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_obs_seed_kernel, dim3(grid), dim3(OBS_TB), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_obs_check_launch(const float* q, const float* dir, const int* rowptr, const float* value, const float* wgt, long n,
                               long nO, int dim, int* err_dev, hipStream_t s) {
  const long nd = n * dim;
  long most = nO > n ? nO : n;
  if (dir && nd > most) most = nd;
  if (most <= 0) return hipSuccess;
  hipLaunchKernelGGL(vn_obs_check_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, s, q, dir, rowptr, value, wgt, n, nO,
                     nd, err_dev);
  return hipGetLastError();
}
