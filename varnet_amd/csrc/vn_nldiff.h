// Host-side declarations of vn_nldiff.hip: the solution-dependent diffusivity D(c) = d0 + d1 c + d2 c^2 of the quasilinear
// diffusion term div(kappa D(c) grad c) (vn_set_nldiff), on the row-wise routes and in the de-duplicated step (kept out of
// vn_internal.h, which every kernel's source hash covers).  The fp64 objective carries the term inside vn_obj64_seed_kernel.
// On a batch with the term gcoef = kappa dN/dx only: advection enters on the value side through psi.
#pragma once
#include "vn_internal.h"

// Row-wise routes (generic, layer by layer, two-pass): two elementwise kernels around vn_seed_kernel and the flux term's pair.
struct VnNldiffRowArgs {
  const float* u;                            // [nT] network value per row
  const float* psi;                          // [nT] psi_r = sum_d v_d dN_r/dx_d + N_r div v, or nullptr (no advection)
  float d0, d1, d2;
  long nT;
  float* ud;                                 // [nT] in/out: A_r = sum_d u_{x_d} gcoef_d  ->  D(u_r) A_r - u_r psi_r
  float* A;                                  // [nT] engine-owned: A_r saved by the fold kernel, read by the seed kernel
  float* udbar;                              // [nT] in/out: tangent seed of every row (vn_seed_kernel's output) -> D(u_r) x it
  float* ubar;                               // [nT] in/out: value seed of every row
};
// A[r] = ud[r];  ud[r] = D(u_r) A[r] - u_r psi_r   (before everything else that edits ud)
hipError_t vn_nldiff_fold_launch(const VnNldiffRowArgs& a, hipStream_t s);
// ubar[r] += (D'(u_r) A[r] - psi_r) udbar[r];  udbar[r] *= D(u_r)   (after everything else that reads udbar)
hipError_t vn_nldiff_seed_launch(const VnNldiffRowArgs& a, hipStream_t s);

// De-duplicated step: a source kernel before vn_dedup_seed_kernel and a per-point kernel after the gathers.
struct VnNldiffDedupArgs {
  const float* upack;                        // [U, 4]: (u, grad u) at the unique points (vn_pgrad16's out_pack)
  const int* uid;                            // [nT] row -> unique point
  const int* rowptr; const int* rowidx;      // CSR unique point -> rows
  const float* base;                         // [nT] or nullptr: the source of the batch, or what the reaction / flux term made of
                                             // it (may be s_eff itself)
  const float* gcoef;                        // [nT, dim] in row order; rows [0, q) serve as the table when gper
  const float* psi;                          // [nT] or nullptr
  float d0, d1, d2;
  const float* feN; const float* feW;        // [q] tables (feW may be nullptr)
  const float* stf;                          // [n_k] seed of every test function (vn_dedup_seed_kernel's output)
  long nT, U; int q, dim, gper;
  float* s_eff;                              // [nT] out: base + ((1 - D(u_j)) (grad u_j . gcoef_r) + u_j psi_r) / N_p
  float* seed_u; float* seed_g;              // [U], [U, dim] in/out: the gathered seeds of the unique points
};
// s_eff[r] = base[r] + ((1 - D(u_j)) (grad u_j . gcoef_r) + u_j psi_r) / N_p, j = uid[r]: vn_dedup_seed_kernel multiplies its
// `source` by N_p and subtracts it, which turns A_r into D(u_j) A_r - u_j psi_r.  The caller has checked that no N_p is zero.
hipError_t vn_nldiff_source_launch(const VnNldiffDedupArgs& a, hipStream_t s);
// seed_u[j] += D'(u_j) (grad u_j . seed_g[j,:]) - sum over the rows r of point j, in CSR order, of W_p psi[r] stf[r / q];
// seed_g[j,:] *= D(u_j)   (after vn_dedup_gather_launch and the other terms' gathers)
hipError_t vn_nldiff_point_launch(const VnNldiffDedupArgs& a, hipStream_t s);
