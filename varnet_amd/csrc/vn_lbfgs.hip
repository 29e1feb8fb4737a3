// Kernels of the device-resident L-BFGS optimizer (vn_lbfgs_step): see vn_lbfgs.h for the scheme.  Vector loads and stores
// only; every inner product is accumulated in fp64 in an order fixed by (P, the constants of vn_lbfgs.h) alone, so an
// iteration is bitwise repeatable from run to run and from GPU to GPU.
#include "vn_lbfgs.h"

namespace {

constexpr int M = VN_LBFGS_M, SLOTS = VN_LBFGS_SLOTS, NB = VN_LBFGS_NB, NACC = VN_LBFGS_NACC;
constexpr int GBLOCK = 256;       // threads of the Gram kernel's workgroups
constexpr int EBLOCK = 256;       // threads of the elementwise kernels' workgroups
constexpr int EMAXBLK = 1024;

__device__ inline const float* basis_vec(const VnLbfgsBufs& b, long P, int j) {
  return j < 2 * SLOTS ? b.ring + (long)j * P : b.g_k;
}

constexpr int NRED = 72;          // NACC padded to 8 * 9 for the wave reduction below

// Sums each of a lane's NRED values over the 64 lanes of its wave in a fixed order.  Three halving exchanges -- the two lanes of
// a pair split the values between them, each keeps the half its lane bit selects and adds the partner's copy of it: 72 -> 36 -> 18
// -> 9 values per lane -- then a butterfly inside the 8-lane groups: 90 lane exchanges where a butterfly per value takes 432 (the
// exchanges go through the LDS crossbar, which the four waves of a workgroup share: 18 -> 5 us for P = 81).
// On return a[0..8] of lane l hold the totals of the values e + 9 (l>>3 & 1) + 18 (l>>4 & 1) + 36 (l>>5 & 1), e = 0..8.
__device__ inline void wave_sum_many(double (&a)[NRED], int lane) {
  const bool b32 = lane & 32, b16 = lane & 16, b8 = lane & 8;
#pragma unroll
  for (int e = 0; e < 36; ++e) a[e] = (b32 ? a[e + 36] : a[e]) + __shfl_xor(b32 ? a[e] : a[e + 36], 32, 64);
#pragma unroll
  for (int e = 0; e < 18; ++e) a[e] = (b16 ? a[e + 18] : a[e]) + __shfl_xor(b16 ? a[e] : a[e + 18], 16, 64);
#pragma unroll
  for (int e = 0; e < 9; ++e) a[e] = (b8 ? a[e + 9] : a[e]) + __shfl_xor(b8 ? a[e] : a[e + 9], 8, 64);
#pragma unroll
  for (int o = 4; o > 0; o >>= 1)
#pragma unroll
    for (int e = 0; e < 9; ++e) a[e] += __shfl_xor(a[e], o, 64);
}

// Sum over the NB lanes that hold a coefficient, the same in every lane: through the LDS in index order (a butterfly of six
// dependent lane exchanges costs three times as much, and the two-loop is a chain of 21 such sums)
__device__ inline double coef_sum(double term, double* tmp, int lane) {
  __syncthreads();
  if (lane < NB) tmp[lane] = term;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < NB; ++j) s += tmp[j];
  return s;
}

// slot of the i-th newest live pair
__device__ inline int slot_of(int head, int i) { return (head - 1 - i + 2 * SLOTS) % SLOTS; }

// 1. Rows of G = B^T B of the vectors that are new since the last iteration: the pending pair (s, y in slot `head`) and g_k,
// against every live vector; plus |g_k|_1.  Workgroup k owns the k-th contiguous chunk of [0, P); its threads stride through the
// chunk, then fold through a fixed butterfly and a fixed order over the waves.  Partials: part[k][NACC].
__global__ __launch_bounds__(GBLOCK) void vn_lbfgs_gram_kernel(VnLbfgsBufs b, long P, int reset) {
  __shared__ double red[GBLOCK / 64][NACC];
  const int head = b.meta->head;
  const int count = reset ? 0 : b.meta->count;
  const int pending = reset ? 0 : b.meta->pending;
  unsigned live = 1u << (NB - 1);
  for (int i = 0; i < count; ++i) {
    const int s = slot_of(head, i);
    live |= (1u << s) | (1u << (SLOTS + s));
  }
  if (pending) live |= (1u << head) | (1u << (SLOTS + head));
  const float* n0 = b.ring + (long)head * P;
  const float* n1 = b.ring + (long)(SLOTS + head) * P;

  const long per = (P + gridDim.x - 1) / gridDim.x;
  const long lo = (long)blockIdx.x * per;
  const long hi = lo + per < P ? lo + per : P;
  double acc[NRED];
#pragma unroll
  for (int e = 0; e < NRED; ++e) acc[e] = 0.0;
  for (long i = lo + threadIdx.x; i < hi; i += GBLOCK) {
    double v[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      // every load is issued (a dead slot reads g_k instead and is zeroed by a select): loads behind 23 uniform branches would
      // each wait for the one before
      const bool on = (live >> j) & 1u;
      const float x = (on ? basis_vec(b, P, j) : b.g_k)[i];
      v[j] = on ? (double)x : 0.0;
    }
    const double a2 = v[NB - 1];
    acc[NACC - 1] += fabs(a2);
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[2 * NB + j] = fma(a2, v[j], acc[2 * NB + j]);
    if (pending) {
      const double a0 = (double)n0[i], a1 = (double)n1[i];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        acc[j] = fma(a0, v[j], acc[j]);
        acc[NB + j] = fma(a1, v[j], acc[NB + j]);
      }
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  wave_sum_many(acc, lane);
  if ((lane & 7) == 0) {
    const int base = 9 * ((lane >> 3) & 1) + 18 * ((lane >> 4) & 1) + 36 * ((lane >> 5) & 1);
#pragma unroll
    for (int e = 0; e < 9; ++e)
      if (base + e < NACC) red[wave][base + e] = acc[e];
  }
  __syncthreads();
  if (threadIdx.x < NACC) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < GBLOCK / 64; ++w) s += red[w][threadIdx.x];
    b.part[(long)blockIdx.x * NACC + threadIdx.x] = s;
  }
}

// 2. One wave: partials folded in block order into G, curvature test of the pending pair, the two-loop recursion on the
// NB coefficients (lane j holds coefficient j; an inner product with a basis vector is a row of G times the coefficients, summed
// through a fixed butterfly), delta, g.d, t0.
__global__ __launch_bounds__(64) void vn_lbfgs_twoloop_kernel(VnLbfgsBufs b, int nblk, int reset) {
  __shared__ double G[NB * NB];
  __shared__ double fold[NACC];
  __shared__ double tmp[NB];
  const int lane = threadIdx.x;
  int head = b.meta->head;
  int count = reset ? 0 : b.meta->count;
  const int pending = reset ? 0 : b.meta->pending;

  for (int e = lane; e < NACC; e += 64) {
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += b.part[(long)k * NACC + e];
    fold[e] = s;
  }
  for (int e = lane; e < NB * NB; e += 64) G[e] = b.G[e];
  __syncthreads();
  for (int e = lane; e < 3 * NB; e += 64) {
    const int a = e / NB, j = e % NB;
    if (a < 2 && !pending) continue;
    const int r = a == 0 ? head : a == 1 ? SLOTS + head : NB - 1;
    // (an entry between two new vectors is written from both rows: the same products in the same order, the same bits)
    G[r * NB + j] = fold[e];
    G[j * NB + r] = fold[e];
  }
  __syncthreads();

  double kept = 0.0;
  if (pending) {
    const double sy = G[head * NB + SLOTS + head], ss = G[head * NB + head], yy = G[(SLOTS + head) * NB + SLOTS + head];
    if (sy > 1e-10 * sqrt(ss) * sqrt(yy)) {
      kept = 1.0;
      count = count + 1 < M ? count + 1 : M;
      head = (head + 1) % SLOTS;
    }
  }

  const int gi = NB - 1;
  double q = lane == gi ? 1.0 : 0.0;
  double alpha[M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    alpha[i] = 0.0;
    if (i < count) {
      const int si = slot_of(head, i), yi = SLOTS + si;
      const double rho = 1.0 / G[si * NB + yi];
      const double a = rho * coef_sum((lane < NB && q != 0.0) ? q * G[si * NB + lane] : 0.0, tmp, lane);
      alpha[i] = a;
      if (lane == yi) q -= a;
    }
  }
  double gamma = 1.0;
  if (count > 0) {
    const int s0 = slot_of(head, 0), y0 = SLOTS + s0;
    gamma = G[s0 * NB + y0] / G[y0 * NB + y0];
  }
  double r = gamma * q;
#pragma unroll
  for (int i = M - 1; i >= 0; --i) {
    if (i < count) {
      const int si = slot_of(head, i), yi = SLOTS + si;
      const double rho = 1.0 / G[si * NB + yi];
      const double beta = rho * coef_sum((lane < NB && r != 0.0) ? r * G[yi * NB + lane] : 0.0, tmp, lane);
      if (lane == si) r += alpha[i] - beta;
    }
  }
  double delta = -r;
  double gd = coef_sum((lane < NB && delta != 0.0) ? delta * G[gi * NB + lane] : 0.0, tmp, lane);
  double dropped = 0.0;
  int pairs = count;
  if (!(gd < 0.0)) {             // not a descent direction (or not a number): drop the ring, steepest descent
    if (count > 0) dropped = 1.0;
    count = 0;
    pairs = 0;
    delta = lane == gi ? -1.0 : 0.0;
    gd = -G[gi * NB + gi];
  }
  const double g1 = fold[NACC - 1];
  double t0 = 1.0;
  if (pairs == 0) {
    const double inv = 1.0 / g1;
    t0 = inv < 1.0 ? inv : 1.0;
  }
  if (lane < NB) b.coef[lane] = delta;
  for (int e = lane; e < NB * NB; e += 64) b.G[e] = G[e];
  if (lane == 0) {
    b.coef[NB] = t0;
    b.meta->head = head;
    b.meta->count = count;
    b.meta->pending = 0;
    b.out->gd = gd;
    b.out->t0 = t0;
    b.out->g1 = g1;
    b.out->pairs = (double)pairs;
    b.out->dropped = dropped;
    b.out->kept = kept;
  }
}

// 3. d = B delta (fp64 sum over the basis in index order, rounded once) and the trial point fl32(theta_k + t d)
__global__ __launch_bounds__(EBLOCK) void vn_lbfgs_trial_kernel(VnLbfgsBufs b, float* __restrict__ theta, long P, double scale,
                                                                 int form_d) {
  __shared__ double c[NB + 1];
  if (threadIdx.x < NB + 1) c[threadIdx.x] = b.coef[threadIdx.x];
  __syncthreads();
  const double t = c[NB] * scale;
  const long stride = (long)gridDim.x * EBLOCK;
  for (long i = (long)blockIdx.x * EBLOCK + threadIdx.x; i < P; i += stride) {
    float di;
    if (form_d) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < NB; ++j) {       // (as in the Gram kernel: all loads issued, vectors with a zero coefficient selected away)
        const bool on = c[j] != 0.0;
        const float x = (on ? basis_vec(b, P, j) : b.g_k)[i];
        acc = fma(c[j], on ? (double)x : 0.0, acc);
      }
      di = (float)acc;
      b.d[i] = di;
    } else {
      di = b.d[i];
    }
    theta[i] = (float)((double)b.theta_k[i] + t * (double)di);
  }
}

// 4. Accepted trial: s = fl32(theta - theta_k), y = fl32(g - g_k) into the spare slot (pending until the next iteration's
// curvature test); theta_k, g_k and the four loss scalars replaced.  first: no pair.
__global__ __launch_bounds__(EBLOCK) void vn_lbfgs_commit_kernel(VnLbfgsBufs b, const float* __restrict__ theta,
                                                                  const float* __restrict__ grad, long P, int first) {
  const int head = b.meta->head;
  float* s = b.ring + (long)head * P;
  float* y = b.ring + (long)(SLOTS + head) * P;
  const long stride = (long)gridDim.x * EBLOCK;
  const long i0 = (long)blockIdx.x * EBLOCK + threadIdx.x;
  for (long i = i0; i < P; i += stride) {
    const float th = theta[i], g = grad[i];
    if (!first) {
      s[i] = th - b.theta_k[i];
      y[i] = g - b.g_k[i];
    }
    b.theta_k[i] = th;
    b.g_k[i] = g;
  }
  if (i0 < 4) b.g_k[P + i0] = grad[P + i0];
  if (i0 == 4) b.meta->pending = first ? 0 : 1;
}

int eblocks(long P) {
  const long n = (P + EBLOCK - 1) / EBLOCK;
  return (int)(n < 1 ? 1 : n < EMAXBLK ? n : EMAXBLK);
}

}  // namespace

int vn_lbfgs_gram_blocks(long P) {
  const long n = (P + 1023) / 1024;
  return (int)(n < 1 ? 1 : n < VN_LBFGS_MAXBLK ? n : VN_LBFGS_MAXBLK);
}

hipError_t vn_lbfgs_gram_launch(const VnLbfgsBufs& b, long P, int reset, hipStream_t s) {
  hipLaunchKernelGGL(vn_lbfgs_gram_kernel, dim3(vn_lbfgs_gram_blocks(P)), dim3(GBLOCK), 0, s, b, P, reset);
  return hipGetLastError();
}

hipError_t vn_lbfgs_twoloop_launch(const VnLbfgsBufs& b, long P, int reset, hipStream_t s) {
  hipLaunchKernelGGL(vn_lbfgs_twoloop_kernel, dim3(1), dim3(64), 0, s, b, vn_lbfgs_gram_blocks(P), reset);
  return hipGetLastError();
}

hipError_t vn_lbfgs_trial_launch(const VnLbfgsBufs& b, float* theta, long P, double scale, int form_d, hipStream_t s) {
  hipLaunchKernelGGL(vn_lbfgs_trial_kernel, dim3(eblocks(P)), dim3(EBLOCK), 0, s, b, theta, P, scale, form_d);
  return hipGetLastError();
}

hipError_t vn_lbfgs_commit_launch(const VnLbfgsBufs& b, const float* theta, const float* grad, long P, int first,
                                  hipStream_t s) {
  hipLaunchKernelGGL(vn_lbfgs_commit_kernel, dim3(eblocks(P)), dim3(EBLOCK), 0, s, b, theta, grad, P, first);
  return hipGetLastError();
}
