// Host-side declarations of vn_bicadapt.hip: weights on the Dirichlet and initial rows (vn_set_bic_weights, vn_set_bic_adapt).
// The rows of vn_set_bic fall into two parts, bc = [0, bDof) and ic = [bDof, nB); each part has its own weights omega_i and,
// when adaptive, its own state of vn_adapt.h.  Maths and the determinism contract: that file's header.  Kept out of
// vn_internal.h, which every kernel's source hash covers.
#pragma once
#include <hip/hip_runtime.h>

constexpr int VN_BICROWS_TB = 256;           // rows per block, and per loss partial
inline int vn_bic_rows_blocks(long nB) { return nB > 0 ? (int)((nB + VN_BICROWS_TB - 1) / VN_BICROWS_TB) : 0; }

struct VnBicRowsArgs {
  const float* ub = nullptr;                 // [nB] values of the rows
  const float* label = nullptr;              // [nB]
  long nB = 0, bDof = 0;
  float biDimVal = 0.f, w0 = 0.f, w1 = 0.f;
  const float* omega[2] = {nullptr, nullptr};   // committed weights of bc [bDof] and ic [nB - bDof]; nullptr: 1
  float* field[2] = {nullptr, nullptr};         // out: unweighted l_i = e_i^2 of each part (nullptr: not kept)
  float* ubar_b = nullptr;                   // [nB] out: vn_bic_value_seed(...) * omega_i (nullptr: loss only)
  float* part = nullptr;                     // [vn_bic_rows_blocks(nB), 3] out: (0, biDimVal sum omega e^2 over bc, ... over ic)
};

// The same weights in the fp64 objective (vn_obj64.hip), around its own seed kernel.  phase 0, before it: wpart[b] = the weighted
// (bc, ic) partial sums of block b from the forward values u [nB].  phase 1, after it: lpart[b * 4 + 1], [b * 4 + 2] = wpart[b]
// (the seed kernel's [*, 4] layout) and, with seeds, u[k] *= omega (the seed kernel left the unweighted seeds there).  omega is
// widened exactly.
struct VnBicRows64Args {
  double* u = nullptr;
  const float* label = nullptr;
  long nB = 0, bDof = 0;
  double biDimVal = 0.0;
  const float* omega[2] = {nullptr, nullptr};
  double* wpart = nullptr;                   // [vn_bic_rows_blocks(nB), 2]
  double* lpart = nullptr;                   // [>= vn_bic_rows_blocks(nB), 4]
  int seeds = 0;
};
hipError_t vn_bic_rows_f64_launch(const VnBicRows64Args& a, int phase, hipStream_t s);

// One launch over the rows: loss field, weighted seeds, weighted loss partials in the layout vn_reduce_launch folds
hipError_t vn_bic_rows_launch(const VnBicRowsArgs& a, hipStream_t s);
