// The seed kernels of the edge row sets (vn_edge.h): each turns the values u and directional derivatives ud of its rows into
// loss partials and the seeds of the generic reverse kernel.  One thread per row, pair or observation, one loss partial per
// block (block_sum; folded by vn_reduce_kernel in a fixed order).  Three kernels because the arithmetic differs:
//   boundary-flux rows   F = mean_F[ biDimVal r^2 ],  r = n . grad_x u + c u - l
//   periodic pairs       P = mean_P[ biDimVal (r0^2 + gamma r1^2) ] over the pairs (i, i + nP), r0 the jump of the value and r1
//                        the jump of the derivative along the pair's common direction
//   observations         O = (1/nO) sum_i wgt_i r_i^2,  r_i = l_i(u) - value_i, with l_i a linear functional of the network over a
//                        segment of registered points, l_i = sum_j (q_j u(x_j) + g_j . grad_x u(x_j))
#include "vn_blocksum.h"
#include "vn_edge.h"

namespace {

constexpr int EDGE_TB = 256;

__global__ __launch_bounds__(EDGE_TB) void vn_flux_seed_kernel(VnFluxSeedArgs a) {
  __shared__ float red[4];
  const long k = (long)blockIdx.x * EDGE_TB + threadIdx.x;
  float e2 = 0.f;
  if (k < a.nF) {
    const float c = a.coef[k];
    const float r = a.ud[k] + c * a.u[k] - a.label[k];
    e2 = a.biDimVal * r * r;
    if (a.ubar) {
      const float s = 2.f * a.w0 * a.biDimVal / (float)a.nF;
      a.udbar[k] = s * r;
      a.ubar[k] = s * c * r;
    }
  }
  const float t = block_sum(e2, red);
  if (threadIdx.x == 0) a.part[blockIdx.x] = t;
}

__global__ __launch_bounds__(EDGE_TB) void vn_periodic_seed_kernel(VnPeriodicSeedArgs a) {
  __shared__ float red[4];
  const long i = (long)blockIdx.x * EDGE_TB + threadIdx.x;
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
  const float t = block_sum(e2, red);
  if (threadIdx.x == 0) a.part[blockIdx.x] = t;
}

// An observation's segment in CSR order, four entries in flight and the additions in CSR order (csr_walk of vn_terms.hip), then
// the seeds of the segment's points.
__global__ __launch_bounds__(EDGE_TB) void vn_obs_seed_kernel(VnObsSeedArgs a) {
  __shared__ float red[4];
  const long i = (long)blockIdx.x * EDGE_TB + threadIdx.x;
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
  const float t = block_sum(e2, red);
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

// one thread per row, pair or observation; nothing to launch for an empty set
template <class Args>
hipError_t seed_launch(void (*kernel)(Args), const Args& a, long count, hipStream_t s) {
  const int grid = vn_edge_seed_blocks(count);
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(EDGE_TB), 0, s, a);
  return hipGetLastError();
}

}  // namespace

int vn_edge_seed_blocks(long count) { return (int)((count + EDGE_TB - 1) / EDGE_TB); }

hipError_t vn_flux_seed_launch(const VnFluxSeedArgs& a, hipStream_t s) { return seed_launch(vn_flux_seed_kernel, a, a.nF, s); }
hipError_t vn_periodic_seed_launch(const VnPeriodicSeedArgs& a, hipStream_t s) { return seed_launch(vn_periodic_seed_kernel, a, a.nP, s); }
hipError_t vn_obs_seed_launch(const VnObsSeedArgs& a, hipStream_t s) { return seed_launch(vn_obs_seed_kernel, a, a.nO, s); }

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
