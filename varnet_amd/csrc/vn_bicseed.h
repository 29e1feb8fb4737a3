// The value seed of a BC/IC row: d loss / d u_b[k] for the error e = u_b[k] - label[k] of row k, rows [0, bDof) boundary, rows
// [bDof, nB) initial (TFModel.py:643).  Written once: vn_seed_kernel (vn_generic.hip) stores it as ubar_b[k], and the reduction
// of the learnt boundary / initial amplitudes (vn_bicgrad_kernel, vn_learnt.hip) forms the same value from the same inputs.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float vn_bic_value_seed(long k, float e, long nB, long bDof, float biDimVal, float w0, float w1) {
  const long nI = nB - bDof;
  const float cb = 2.f * w0 * biDimVal / (float)bDof;
  const float ci = nI > 0 ? 2.f * w1 * biDimVal / (float)nI : 0.f;
  return (k < bDof ? cb : ci) * e;
}
