// Host-side declarations of vn_nlflux.hip: the polynomial flux term -div(w F(c)), F(c) = f1 c + f2 c^2 + f3 c^3 (vn_set_nlflux),
// on the row-wise routes and in the de-duplicated step (kept out of vn_internal.h, which every kernel's source hash covers).
// The fp64 objective carries the term inside vn_obj64_seed_kernel.
#pragma once
#include "vn_internal.h"

// Row-wise routes (generic, layer by layer, two-pass): two elementwise kernels around vn_seed_kernel.
struct VnNlfluxRowArgs {
  const float* u;                            // [nT] network value per row
  const float* phi;                          // [nT] phi_r = sum_d w_d dN_r/dx_d
  float f1, f2, f3;
  long nT;
  float* ud;                                 // [nT] in/out: the row integrand's tangent part sum_d u_{x_d} gcoef_d
  const float* udbar;                        // [nT] tangent seed of every row (vn_seed_kernel's output)
  float* ubar;                               // [nT] in/out: value seed of every row
};
// ud[r] -= F(u_r) phi_r   (before vn_seed_launch)
hipError_t vn_nlflux_fold_launch(const VnNlfluxRowArgs& a, hipStream_t s);
// ubar[r] -= phi_r F'(u_r) udbar[r]   (after vn_seed_launch, when it produced seeds)
hipError_t vn_nlflux_seed_launch(const VnNlfluxRowArgs& a, hipStream_t s);

// De-duplicated step: two kernels around vn_dedup_seed_kernel / vn_dedup_gather_kernel, modelled on vn_react.hip.
struct VnNlfluxDedupArgs {
  const float* upack;                        // [U, 4]: (u, grad u) at the unique points, u at offset 0 (vn_pgrad16's out_pack)
  const int* uid;                            // [nT] row -> unique point
  const int* rowptr; const int* rowidx;      // CSR unique point -> rows
  const float* base;                         // [nT] or nullptr: the source of the batch, or source + rate p(u) (may be s_eff itself)
  const float* phi;                          // [nT]
  float f1, f2, f3;
  const float* feN; const float* feW;        // [q] tables (feW may be nullptr)
  const float* stf;                          // [n_k] seed of every test function (vn_dedup_seed_kernel's output)
  long nT, U; int q;
  float* s_eff;                              // [nT] out: base + F(u) phi / N_p
  float* seed_u;                             // [U] in/out: d loss / d u of the unique points
};
// s_eff[r] = base[r] + F(u at the point of row r) phi[r] / N_p: the `source` of vn_dedup_seed_kernel, which multiplies it by N_p.
// The caller has checked that no table entry N_p is zero.
hipError_t vn_nlflux_source_launch(const VnNlfluxDedupArgs& a, hipStream_t s);
// seed_u[j] -= F'(u_j) sum over the rows r of point j, in CSR order, of W_p phi[r] stf[r / q]   (after vn_dedup_gather_launch)
hipError_t vn_nlflux_gather_launch(const VnNlfluxDedupArgs& a, hipStream_t s);
