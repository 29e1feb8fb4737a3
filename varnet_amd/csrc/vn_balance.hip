// Adaptive loss balancing, device side: what a balancing rule needs of the per-term gradients G_k = d L_k / d theta, reduced on
// the device so that a probe ends in one read-back of 32 doubles.
//
// Statistics of K <= 4 fp32 vectors T [K][n], all in fp64:
//   sumsq_k = sum_p T_k[p]^2,   sumabs_k = sum_p |T_k[p]|,   maxabs_k = max_p |T_k[p]|,   gram_ab = sum_p T_a[p] T_b[p]
// Every product is (double) a * (double) b, exact (two 24-bit significands), so the only roundings are the fp64 adds.
//   stage 1   vn_balance_grid(n) blocks of 256 threads -- a function of n alone, so the bits do not depend on the card --, a
//             grid-stride loop four entries deep: the 4 K loads of an iteration are issued before anything waits (the rule at the top
//             of vn_reduce_kernel: at P ~ 1e4 this is a latency chain between two training steps, not a bandwidth problem).
//             Per thread fp64 accumulators in entry order, then one fixed shuffle tree per wave, then the four wave sums left to
//             right (the fp64 form of block_sum, vn_blocksum.h; max in place of + for maxabs).  One row of partials per block.
//   stage 2   one wave: lane v folds value v of the rows in block order, sixteen loads in flight, and the lanes write the slot:
//             stats [K][3] then gram [K][K], whose diagonal IS sumsq (computed once) and whose halves are one value.
// No atomics anywhere: two launches on the same bits give the same bits.  A NaN entry makes its sums NaN; maxabs ignores it (fmax).
//
// Accumulate: T[p] = g[p] for the first batch of an epoch, T[p] = fl32(T[p] + g[p]) after it, in the order given; thread 0 sums the
// term's unweighted loss scalar next to it in fp64.
#include "vn_balance.h"

namespace {

constexpr int BAL_THREADS = 256;
constexpr int BAL_DEPTH = 4;                 // entries per thread and iteration
constexpr int BAL_PER_BLOCK = 4096;          // entries a block takes before the grid grows (until VN_BAL_MAX_BLOCKS)

// row layout of the partials and of stage 2's LDS: sumsq [K] | sumabs [K] | maxabs [K] | dot products (a < b, a-major) [K (K-1) / 2]
template <int K>
__global__ __launch_bounds__(BAL_THREADS) void vn_balance_stats_kernel(const float* __restrict__ T, long n, double* __restrict__ part) {
  constexpr int ND = K * (K - 1) / 2, NV = 3 * K + ND;
  __shared__ double red[4][NV];
  double acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.0;
  const long stride = (long)gridDim.x * BAL_THREADS;
  for (long i0 = (long)blockIdx.x * BAL_THREADS + threadIdx.x; i0 < n; i0 += BAL_DEPTH * stride) {
    float x[BAL_DEPTH][K];
#pragma unroll
    for (int j = 0; j < BAL_DEPTH; ++j) {
      const long i = i0 + j * stride;
#pragma unroll
      for (int k = 0; k < K; ++k) x[j][k] = i < n ? T[(long)k * n + i] : 0.f;      // (a zero adds nothing to any of the sums)
    }
#pragma unroll
    for (int j = 0; j < BAL_DEPTH; ++j) {
      double d[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        d[k] = (double)x[j][k];
        acc[k] += d[k] * d[k];
        acc[K + k] += fabs(d[k]);
        acc[2 * K + k] = fmax(acc[2 * K + k], fabs(d[k]));
      }
      int v = 3 * K;
#pragma unroll
      for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = a + 1; b < K; ++b) acc[v++] += d[a] * d[b];
    }
  }
  // the fp64 form of block_sum: a fixed shuffle tree per wave, then the four wave values left to right
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const bool is_max = v >= 2 * K && v < 3 * K;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double t = __shfl_down(acc[v], o, 64);
      acc[v] = is_max ? fmax(acc[v], t) : acc[v] + t;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) red[wave][v] = acc[v];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int v = threadIdx.x;
    const bool is_max = v >= 2 * K && v < 3 * K;
    const double r = is_max ? fmax(fmax(fmax(red[0][v], red[1][v]), red[2][v]), red[3][v]) : red[0][v] + red[1][v] + red[2][v] + red[3][v];
    part[(long)blockIdx.x * VN_BAL_ROW + v] = r;
  }
}

template <int K>
__global__ __launch_bounds__(64) void vn_balance_fold_kernel(const double* __restrict__ part, int rows, double* __restrict__ out) {
  constexpr int ND = K * (K - 1) / 2, NV = 3 * K + ND;
  __shared__ double res[NV];
  const int v = threadIdx.x;
  if (v < NV) {
    const bool is_max = v >= 2 * K && v < 3 * K;
    double r = 0.0;
    for (int b0 = 0; b0 < rows; b0 += 16) {
      double t[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) t[j] = b0 + j < rows ? part[(long)(b0 + j) * VN_BAL_ROW + v] : 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (b0 + j < rows) r = is_max ? fmax(r, t[j]) : r + t[j];            // block order
    }
    res[v] = r;
  }
  __syncthreads();
  if (v < 3 * K) out[v] = res[(v % 3) * K + v / 3];                          // stats [k][c]
  if (v < K * K) {
    const int a = v / K < v % K ? v / K : v % K, b = v / K < v % K ? v % K : v / K;
    // (a, b), a < b, sits at 3 K + a K - a (a + 1) / 2 + (b - a - 1); the diagonal is sumsq itself
    out[3 * K + v] = a == b ? res[a] : res[3 * K + a * K - a * (a + 1) / 2 + (b - a - 1)];
  }
}

__global__ __launch_bounds__(BAL_THREADS) void vn_balance_accum_kernel(float* __restrict__ T, const float* __restrict__ g, long n, int first,
                                                                       double* __restrict__ val, const float* __restrict__ vf,
                                                                       const double* __restrict__ vd) {
  const long i0 = (long)blockIdx.x * (BAL_THREADS * BAL_DEPTH) + threadIdx.x;
  float gi[BAL_DEPTH], ti[BAL_DEPTH];
#pragma unroll
  for (int j = 0; j < BAL_DEPTH; ++j) {
    const long i = i0 + j * BAL_THREADS;
    gi[j] = i < n ? g[i] : 0.f;
    ti[j] = i < n && !first ? T[i] : 0.f;
  }
  const bool sum_val = blockIdx.x == 0 && threadIdx.x == 0 && val != nullptr && (vf != nullptr || vd != nullptr);
  double x = 0.0, v0 = 0.0;
  if (sum_val) {
    x = vf ? (double)vf[0] : vd[0];
    v0 = first ? 0.0 : val[0];
  }
#pragma unroll
  for (int j = 0; j < BAL_DEPTH; ++j) {
    const long i = i0 + j * BAL_THREADS;
    if (i < n) T[i] = first ? gi[j] : __fadd_rn(ti[j], gi[j]);
  }
  if (sum_val) val[0] = v0 + x;
}

template <int K>
void stats_launch(const float* T, long n, int grid, double* part, double* out, hipStream_t s) {
  hipLaunchKernelGGL(vn_balance_stats_kernel<K>, dim3(grid), dim3(BAL_THREADS), 0, s, T, n, part);
  hipLaunchKernelGGL(vn_balance_fold_kernel<K>, dim3(1), dim3(64), 0, s, part, grid, out);
}

}  // namespace

int vn_balance_grid(int64_t n) {
  const int64_t g = (n + BAL_PER_BLOCK - 1) / BAL_PER_BLOCK;
  return g < 1 ? 1 : g > VN_BAL_MAX_BLOCKS ? VN_BAL_MAX_BLOCKS : (int)g;
}

hipError_t vn_balance_stats_launch(const float* T, int K, int64_t n, double* part, double* out, hipStream_t s) {
  if (!T || !part || !out || K < 1 || K > VN_BAL_MAX_K || n < 1) return hipErrorInvalidValue;
  const int grid = vn_balance_grid(n);
  switch (K) {
    case 1: stats_launch<1>(T, (long)n, grid, part, out, s); break;
    case 2: stats_launch<2>(T, (long)n, grid, part, out, s); break;
    case 3: stats_launch<3>(T, (long)n, grid, part, out, s); break;
    default: stats_launch<4>(T, (long)n, grid, part, out, s); break;
  }
  return hipGetLastError();
}

hipError_t vn_balance_accum_launch(float* T, const float* g, int64_t n, int first, double* val, const float* vf, const double* vd,
                                   hipStream_t s) {
  if (!T || !g || n < 1) return hipErrorInvalidValue;
  const int64_t per = (int64_t)BAL_THREADS * BAL_DEPTH;
  hipLaunchKernelGGL(vn_balance_accum_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(BAL_THREADS), 0, s, T, g, (long)n, first, val,
                     vf, vd);
  return hipGetLastError();
}
