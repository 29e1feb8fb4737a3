// Learnt weight scales: the network the compute kernels evaluate is theta_eff = f(s_group) * V, a raw vector V and one scale per
// group of entries; the optimizer steps (V, s) through the chain rule.  An entry in no group is the ordinary parameter (f = 1).
//   rwf    f(s) = exp(s);  one group per output neuron of EVERY layer;  a group = column j of W_l (weights only)
//   slope  f(s) = n s;     hidden layers only;  a group = column j of W_l and b_l[j], or (tied) all of W_l and b_l
// With g = d loss / d theta_eff in the gradient buffer:
//   g_V[p] = fl32( f(s_old) g[p] )                      (f formed in double from the scale of BEFORE the step: one rounding)
//   g_s    = fl32( f'(s_old) sum_{p in group} V[p] g[p] )    (products widened exactly, summed in fp64 in a fixed order)
//   Adam on V with g_V and on s with g_s: the arithmetic of vn_adam_kernel, the rate of s its own
//   theta_eff[p] = fl32(f(s_new)) * V_new[p]            (f rounded ONCE to fp32, one fp32 multiply)
// Kernel shape: one workgroup of four waves per layer, every dependency of the step being layer-local.  Lane j owns column j
// (loads along a row of W_l are coalesced), wave w takes the rows i = w, w + 4, ...; the waves' fp64 sub-sums are added in wave
// order through LDS, the bias product last, and a tied layer folds its 64 column sums with one fixed shuffle tree.  No atomics:
// two launches on the same inputs give the same bits.  The threads that own a scale step it, publish fl32(f(s_new)) through LDS,
// and after the barrier every thread steps its entries of V and writes theta_eff.
// This kernel sits between two training steps that may be 40 us long, so (the rule of vn_reduce_kernel) every global load is
// issued before anything waits.
#include "vn_reparam.h"
#include "../../include/varnet_hip.h"

namespace {

constexpr int RP_WAVES = 4;
constexpr int RP_ROWS = VN_RP_MAX_WIDTH / RP_WAVES;          // rows of W_l one wave takes at most

__device__ __forceinline__ double scale_f(int mode, double n, float s) { return mode == VN_REPARAM_RWF ? exp((double)s) : n * (double)s; }

template <bool STEP>
__global__ __launch_bounds__(64 * RP_WAVES) void vn_reparam_kernel(VnReparamArgs a) {
  __shared__ double sub[RP_WAVES][64];
  __shared__ float fnew[64];
  const int k = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fi = a.fi[k], fo = a.fo[k], wo = a.woff[k], bo = a.boff[k], so = a.soff[k];
  const bool col = lane < fo;
  const bool grouped = so >= 0, tied = grouped && a.tied != 0, bias_in = grouped && a.mode == VN_REPARAM_SLOPE;
  const int sidx = grouped ? so + (tied ? 0 : lane) : 0;
  const bool owner = grouped && w == 0 && (tied ? lane == 0 : col);
  const bool hasb = w == 0 && col;

  float Vw[RP_ROWS], gw[RP_ROWS], mw[RP_ROWS], vw[RP_ROWS];
#pragma unroll
  for (int r = 0; r < RP_ROWS; ++r) {
    const int i = w + RP_WAVES * r;
    const bool ok = col && i < fi;
    const int idx = wo + i * fo + lane;
    Vw[r] = ok ? a.V[idx] : 0.f;
    gw[r] = ok ? a.g[idx] : 0.f;
    if (STEP) { mw[r] = ok ? a.m[idx] : 0.f; vw[r] = ok ? a.v[idx] : 0.f; }
  }
  float Vb = 0.f, gb = 0.f, mb = 0.f, vb = 0.f;
  if (hasb) {
    Vb = a.V[bo + lane]; gb = a.g[bo + lane];
    if (STEP) { mb = a.m[bo + lane]; vb = a.v[bo + lane]; }
  }
  float s_old = 0.f, mso = 0.f, vso = 0.f;
  if (grouped && (col || tied)) s_old = a.s[sidx];
  if (STEP && owner) { mso = a.ms[sidx]; vso = a.vs[sidx]; }
  float loss = 0.f, lacc = 0.f;
  const bool acc_loss = STEP && k == 0 && threadIdx.x == 0 && a.loss_acc != nullptr;
  if (acc_loss) { loss = a.g[a.P]; lacc = a.loss_acc[0]; }

  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < RP_ROWS; ++r) acc += (double)Vw[r] * (double)gw[r];      // (a product of two floats is exact in double)
  sub[w][lane] = acc;
  const double fd = grouped ? scale_f(a.mode, a.n, s_old) : 1.0;               // f of BEFORE the step
  __syncthreads();
  if (w == 0 && grouped) {
    double c = ((sub[0][lane] + sub[1][lane]) + sub[2][lane]) + sub[3][lane];
    if (bias_in) c += (double)Vb * (double)gb;
    if (tied) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    }
    if (owner) {
      const float gsi = (float)((a.mode == VN_REPARAM_RWF ? fd : a.n) * c);
      if (STEP) {
        const float mi = a.b1 * mso + (1.f - a.b1) * gsi;
        const float vi = a.b2 * vso + (1.f - a.b2) * gsi * gsi;
        const float sn = s_old - a.lr_s_t * mi / (sqrtf(vi) + a.eps);
        const float fn = (float)scale_f(a.mode, a.n, sn);
        a.ms[sidx] = mi;
        a.vs[sidx] = vi;
        a.s[sidx] = sn;
        a.f[sidx] = fn;
        fnew[lane] = fn;
      } else {
        a.gs[sidx] = gsi;
      }
    }
  }
  if (!STEP) {
#pragma unroll
    for (int r = 0; r < RP_ROWS; ++r) {
      const int i = w + RP_WAVES * r;
      if (col && i < fi) a.gV[wo + i * fo + lane] = grouped ? (float)(fd * (double)gw[r]) : gw[r];
    }
    if (hasb) a.gV[bo + lane] = bias_in ? (float)(fd * (double)gb) : gb;
    return;
  }
  __syncthreads();
  const float fn = grouped ? fnew[tied ? 0 : lane] : 1.f;      // (lanes beyond the layer's width read a slot nobody wrote and use it nowhere)
  if (acc_loss) a.loss_acc[0] = lacc + loss;                   // epoch loss = sum of pre-update losses, as vn_adam_kernel adds it
#pragma unroll
  for (int r = 0; r < RP_ROWS; ++r) {
    const int i = w + RP_WAVES * r;
    if (col && i < fi) {
      const int idx = wo + i * fo + lane;
      const float gi = grouped ? (float)(fd * (double)gw[r]) : gw[r];
      const float mi = a.b1 * mw[r] + (1.f - a.b1) * gi;       // vn_adam_kernel, operation for operation
      const float vi = a.b2 * vw[r] + (1.f - a.b2) * gi * gi;
      const float Vn = Vw[r] - a.lr_t * mi / (sqrtf(vi) + a.eps);
      a.m[idx] = mi;
      a.v[idx] = vi;
      a.V[idx] = Vn;
      a.theta[idx] = grouped ? __fmul_rn(fn, Vn) : Vn;         // one fp32 multiply, never contracted
    }
  }
  if (hasb) {
    const float gi = bias_in ? (float)(fd * (double)gb) : gb;
    const float mi = a.b1 * mb + (1.f - a.b1) * gi;
    const float vi = a.b2 * vb + (1.f - a.b2) * gi * gi;
    const float Vn = Vb - a.lr_t * mi / (sqrtf(vi) + a.eps);
    a.m[bo + lane] = mi;
    a.v[bo + lane] = vi;
    a.V[bo + lane] = Vn;
    a.theta[bo + lane] = bias_in ? __fmul_rn(fn, Vn) : Vn;
  }
}

// Elementwise over the P entries: REBUILD theta = f * V, else V = theta / f.  Every thread forms the f of its own entry's group
// (the same double expression everywhere: the same bits); the threads t < S also store it.
template <bool REBUILD>
__global__ __launch_bounds__(256) void vn_reparam_map_kernel(VnReparamArgs a, const int* __restrict__ group) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < a.S) a.f[p] = (float)scale_f(a.mode, a.n, a.s[p]);
  if (p >= a.P) return;
  const int gi = group[p];
  if (gi < 0) {
    if (REBUILD) a.theta[p] = a.V[p]; else a.V[p] = a.theta[p];
    return;
  }
  const float f = (float)scale_f(a.mode, a.n, a.s[gi]);
  if (REBUILD) a.theta[p] = __fmul_rn(f, a.V[p]);
  else a.V[p] = __fdiv_rn(a.theta[p], f);
}

bool args_ok(const VnReparamArgs& a) {
  if (a.nl < 1 || a.nl > VN_RP_MAX_LAYERS || a.P < 1 || a.S < 1) return false;
  for (int k = 0; k < a.nl; ++k) {
    if (a.fi[k] < 1 || a.fi[k] > VN_RP_MAX_WIDTH || a.fo[k] < 1 || a.fo[k] > VN_RP_MAX_WIDTH) return false;
    if (a.woff[k] < 0 || a.woff[k] + a.fi[k] * a.fo[k] > a.P || a.boff[k] < 0 || a.boff[k] + a.fo[k] > a.P) return false;
    if (a.soff[k] >= 0 && a.soff[k] + (a.tied ? 1 : a.fo[k]) > a.S) return false;
  }
  return true;
}

}  // namespace

hipError_t vn_reparam_step_launch(const VnReparamArgs& a, hipStream_t s) {
  if (!args_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vn_reparam_kernel<true>, dim3(a.nl), dim3(64 * RP_WAVES), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_reparam_grad_launch(const VnReparamArgs& a, hipStream_t s) {
  if (!args_ok(a) || !a.gV || !a.gs) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vn_reparam_kernel<false>, dim3(a.nl), dim3(64 * RP_WAVES), 0, s, a);
  return hipGetLastError();
}

static int map_grid(const VnReparamArgs& a) { return ((a.P > a.S ? a.P : a.S) + 255) / 256; }

hipError_t vn_reparam_factorise_launch(const VnReparamArgs& a, const int* group, hipStream_t s) {
  if (!args_ok(a) || !group) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vn_reparam_map_kernel<false>, dim3(map_grid(a)), dim3(256), 0, s, a, group);
  return hipGetLastError();
}

hipError_t vn_reparam_rebuild_launch(const VnReparamArgs& a, const int* group, hipStream_t s) {
  if (!args_ok(a) || !group) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vn_reparam_map_kernel<true>, dim3(map_grid(a)), dim3(256), 0, s, a, group);
  return hipGetLastError();
}
