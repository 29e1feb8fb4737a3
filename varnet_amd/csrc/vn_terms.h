// Host-side declarations of vn_terms.hip: the three polynomial terms of the PDE (maths and ordering contract: that file's
// header) on the row-wise routes and in the de-duplicated step.  Kept out of vn_internal.h, which every kernel's source hash
// covers.  The row-wise reaction lives inside vn_seed_kernel (vn_generic.hip); the fp64 objective carries all three terms
// inside vn_obj64_seed_kernel.
#pragma once
#include "vn_internal.h"

// Row-wise routes (generic, layer by layer, two-pass): elementwise kernels around vn_seed_kernel.
struct VnTermRowArgs {
  const float* u;                            // [nT] network value per row
  const float* stream;                       // [nT] flux: phi_r = sum_d w_d dN_r/dx_d;  D(u): psi_r = sum_d v_d dN_r/dx_d + N_r div v,
                                             //      or nullptr (no advection)
  float c[3];                                // flux: (f1, f2, f3);  D(u): (d0, d1, d2)
  const float* cp;                           // [3] device, or nullptr: the same three while they are learnt (vn_set_coef_learn); c is then unused
  long nT;
  float* ud;                                 // [nT] in/out: the row integrand's tangent part A_r = sum_d u_{x_d} gcoef_d
  float* A;                                  // [nT] D(u) only, engine-owned: A_r saved by the fold kernel, read by the seed kernel
  float* udbar;                              // [nT] tangent seed of every row (vn_seed_kernel's output); in/out for D(u)
  float* ubar;                               // [nT] in/out: value seed of every row
};
// ud[r] -= F(u_r) phi_r   (before vn_seed_launch, after the D(u) fold)
hipError_t vn_nlflux_fold_launch(const VnTermRowArgs& a, hipStream_t s);
// ubar[r] -= phi_r F'(u_r) udbar[r]   (after vn_seed_launch, when it produced seeds)
hipError_t vn_nlflux_seed_launch(const VnTermRowArgs& a, hipStream_t s);
// A[r] = ud[r];  ud[r] = D(u_r) A[r] - u_r psi_r   (before everything else that edits ud)
hipError_t vn_nldiff_fold_launch(const VnTermRowArgs& a, hipStream_t s);
// ubar[r] += (D'(u_r) A[r] - psi_r) udbar[r];  udbar[r] *= D(u_r)   (after everything else that reads udbar)
hipError_t vn_nldiff_seed_launch(const VnTermRowArgs& a, hipStream_t s);

// De-duplicated step: a source kernel before vn_dedup_seed_kernel and a per-point kernel after vn_dedup_gather_kernel.
struct VnTermDedupArgs {
  const float* upack;                        // [U, 4]: (u, grad u) at the unique points, u at offset 0 (vn_pgrad16's out_pack)
  const int* uid;                            // [nT] row -> unique point
  const int* rowptr; const int* rowidx;      // CSR unique point -> rows
  const float* base;                         // [nT] or nullptr: the source of the batch, or what the terms before this one made of
                                             // it (may be s_eff itself)
  const float* stream;                       // [nT] reaction: rate, or nullptr (rate == 1);  flux: phi;  D(u): psi, or nullptr
  float c[3];                                // reaction: (c1, c2, c3);  flux: (f1, f2, f3);  D(u): (d0, d1, d2)
  const float* cp;                           // [3] device, or nullptr: the same three while they are learnt (vn_set_coef_learn); c is then unused
  float* acc_out;                            // [U] or nullptr: the gather kernels store their CSR sum (accR_j, accF_j), the point
                                             // kernel its dot product gs_j = grad u_j . seed_g[j,:] -- read by vn_learnt.hip
  const float* feN; const float* feW;        // [q] tables (feW may be nullptr)
  const float* stf;                          // [n_k] seed of every test function (vn_dedup_seed_kernel's output)
  long nT, U; int q;
  float* s_eff;                              // [nT] out: base + the term's share of the source
  float* seed_u;                             // [U] in/out: d loss / d u of the unique points
  // D(u) only (null / zero for the other two)
  const float* gcoef;                        // [nT, dim] in row order; rows [0, q) serve as the table when gper
  int dim, gper;
  float* seed_g;                             // [U, dim] in/out: the gathered tangent seeds of the unique points
};
// s_eff[r] = base[r] + the term's share at the point j = uid[r] of row r -- the `source` of vn_dedup_seed_kernel, which
// multiplies it by N_p and subtracts it from the row integrand:
//   reaction   rate[r] p(u_j)
//   flux       F(u_j) phi[r] / N_p
//   D(u)       ((1 - D(u_j)) (grad u_j . gcoef_r) + u_j psi[r]) / N_p, which turns A_r into D(u_j) A_r - u_j psi_r
// For the last two the caller has checked that no table entry N_p is zero.
hipError_t vn_react_source_launch(const VnTermDedupArgs& a, hipStream_t s);
hipError_t vn_nlflux_source_launch(const VnTermDedupArgs& a, hipStream_t s);
hipError_t vn_nldiff_source_launch(const VnTermDedupArgs& a, hipStream_t s);
// After vn_dedup_gather_launch, sums over the rows r of point j in CSR order:
//   reaction   seed_u[j] -= p'(u_j) sum_r N_p W_p rate[r] stf[r / q]
//   flux       seed_u[j] -= F'(u_j) sum_r W_p phi[r] stf[r / q]
//   D(u)       seed_u[j] += D'(u_j) (grad u_j . seed_g[j,:]) - sum_r W_p psi[r] stf[r / q];  seed_g[j,:] *= D(u_j)   (last)
hipError_t vn_react_gather_launch(const VnTermDedupArgs& a, hipStream_t s);
hipError_t vn_nlflux_gather_launch(const VnTermDedupArgs& a, hipStream_t s);
hipError_t vn_nldiff_point_launch(const VnTermDedupArgs& a, hipStream_t s);
