// Host-side declarations of vn_react.hip: the polynomial reaction term rate * (c1 u + c2 u^2 + c3 u^3) in the de-duplicated
// step (kept out of vn_internal.h, which every kernel's source hash covers).  The row-wise routes carry the term inside
// vn_seed_kernel (vn_generic.hip), the fp64 objective inside vn_obj64_seed_kernel.
#pragma once
#include "vn_internal.h"

struct VnReactArgs {
  const float* upack;                        // [U, 4]: (u, grad u) at the unique points, u at offset 0 (vn_pgrad16's out_pack)
  const int* uid;                            // [nT] row -> unique point
  const int* rowptr; const int* rowidx;      // CSR unique point -> rows
  const float* source;                       // [nT] or nullptr
  const float* rate;                         // [nT] or nullptr (rate == 1)
  float c1, c2, c3;
  const float* feN; const float* feW;        // [q] tables (feW may be nullptr)
  const float* stf;                          // [n_k] seed of every test function (vn_dedup_seed_kernel's output)
  long nT, U; int q;
  float* s_eff;                              // [nT] out: source + rate p(u)
  float* seed_u;                             // [U] in/out: d loss / d u of the unique points
};
// s_eff[r] = source[r] + rate[r] p(u at the point of row r): the `source` of vn_dedup_seed_kernel for a batch with a reaction
hipError_t vn_react_source_launch(const VnReactArgs& a, hipStream_t s);
// seed_u[j] -= p'(u_j) sum over the rows r of point j, in CSR order, of N_p W_p rate[r] stf[r / q]   (after vn_dedup_gather_launch)
hipError_t vn_react_gather_launch(const VnReactArgs& a, hipStream_t s);
