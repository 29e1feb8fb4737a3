// Weights on the Dirichlet and initial rows (vn_set_bic_weights, vn_set_bic_adapt).  Per row i of vn_set_bic, e_i = u_i - label_i,
// the unweighted loss field l_i = e_i^2 and a weight omega_i >= 0 that is a constant of the gradient:
//     BC = biDimVal (1 / bDof) sum_{i < bDof} omega_i e_i^2,      IC likewise over rows [bDof, nB)
//     value seed of row i = vn_bic_value_seed(...) * omega_i      (vn_bicseed.h: the one place the unweighted seed is written)
// omega_i = m(lambda_i) / Z_s per part s (bc, ic), formed by the kernels of vn_adapt.hip from that part's committed state; a
// static registration is a state that never moves (m(x) = x).  While a part is adaptive, its state moves at every gradient step
// from the loss field this kernel wrote, by the rules and the commit protocol of vn_adapt.hip, one update per part.
//
// vn_bic_rows_kernel is the rows' seed kernel: one thread per row, 256 rows per block.  It writes l_i to the part's own buffer
// (each starts on the 16-byte grid, so the kernels of vn_adapt.hip read them with 16-byte accesses), the weighted seed, and per
// block the weighted partial sums (0, bc, ic), summed in fp64 over a fixed shuffle / wave tree -- no atomics, the same bits on
// every run -- and stored as the fp32 triple vn_reduce_kernel folds (it divides by bDof and nB - bDof).
//
// vn_bic_rows_f64_kernel carries the same weights into the fp64 objective (vn_obj64.hip), omega widened exactly: it runs on
// either side of that file's own seed kernel (vn_bicadapt.h says what each phase does), with the same block tree.
#include "vn_bicadapt.h"
#include "vn_bicseed.h"

namespace {

// One double per thread over the 256-thread block, fixed order: shuffle tree per wave, the four waves left to right
__device__ __forceinline__ double block_sum64(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(VN_BICROWS_TB) void vn_bic_rows_kernel(VnBicRowsArgs a) {
  __shared__ double red[4];
  const long k = (long)blockIdx.x * VN_BICROWS_TB + threadIdx.x;
  double bc = 0.0, ic = 0.0;
  if (k < a.nB) {
    const bool isbc = k < a.bDof;
    const int s = isbc ? 0 : 1;
    const long j = isbc ? k : k - a.bDof;          // the row's index in its part
    const float e = a.ub[k] - a.label[k];
    const float om = a.omega[s] ? a.omega[s][j] : 1.f;
    if (a.field[s]) a.field[s][j] = e * e;
    if (a.ubar_b) a.ubar_b[k] = vn_bic_value_seed(k, e, a.nB, a.bDof, a.biDimVal, a.w0, a.w1) * om;
    const double v = (double)a.biDimVal * (double)om * ((double)e * (double)e);
    if (isbc) bc = v; else ic = v;
  }
  const double sb = block_sum64(bc, red), si = block_sum64(ic, red);
  if (threadIdx.x == 0) {
    a.part[blockIdx.x * 3 + 0] = 0.f;
    a.part[blockIdx.x * 3 + 1] = (float)sb;
    a.part[blockIdx.x * 3 + 2] = (float)si;
  }
}

__global__ __launch_bounds__(VN_BICROWS_TB) void vn_bic_rows_f64_kernel(VnBicRows64Args a, int phase) {
  __shared__ double red[4];
  const long k = (long)blockIdx.x * VN_BICROWS_TB + threadIdx.x;
  const bool in = k < a.nB, isbc = k < a.bDof;
  const int s = isbc ? 0 : 1;
  const double om = in && a.omega[s] ? (double)a.omega[s][isbc ? k : k - a.bDof] : 1.0;
  if (phase == 0) {
    double bc = 0.0, ic = 0.0;
    if (in) {
      const double e = a.u[k] - (double)a.label[k];
      const double v = a.biDimVal * om * (e * e);
      if (isbc) bc = v; else ic = v;
    }
    const double sb = block_sum64(bc, red), si = block_sum64(ic, red);
    if (threadIdx.x == 0) { a.wpart[blockIdx.x * 2] = sb; a.wpart[blockIdx.x * 2 + 1] = si; }
    return;
  }
  if (in && a.seeds) a.u[k] *= om;
  if (threadIdx.x == 0) {
    a.lpart[blockIdx.x * 4 + 1] = a.wpart[blockIdx.x * 2];
    a.lpart[blockIdx.x * 4 + 2] = a.wpart[blockIdx.x * 2 + 1];
  }
}

}  // namespace

hipError_t vn_bic_rows_f64_launch(const VnBicRows64Args& a, int phase, hipStream_t s) {
  if (a.nB <= 0) return hipSuccess;
  if (!a.u || !a.label || !a.wpart || !a.lpart || a.bDof < 0 || a.bDof > a.nB) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vn_bic_rows_f64_kernel, dim3((unsigned)vn_bic_rows_blocks(a.nB)), dim3(VN_BICROWS_TB), 0, s, a, phase);
  return hipGetLastError();
}

hipError_t vn_bic_rows_launch(const VnBicRowsArgs& a, hipStream_t s) {
  if (a.nB <= 0) return hipSuccess;
  if (!a.ub || !a.label || !a.part || a.bDof < 0 || a.bDof > a.nB) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vn_bic_rows_kernel, dim3((unsigned)vn_bic_rows_blocks(a.nB)), dim3(VN_BICROWS_TB), 0, s, a);
  return hipGetLastError();
}
