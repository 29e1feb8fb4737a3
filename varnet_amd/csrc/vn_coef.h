// Host-side declarations of vn_coef.hip: the gradient of the loss with respect to the nine polynomial coefficients of
// vn_terms.hip (index 0..2 reaction, 3..5 flux, 6..8 diffusivity) and their Adam update (vn_set_coef_learn).  Kept out of
// vn_internal.h, which every kernel's source hash covers.
#pragma once
#include "vn_internal.h"

constexpr int VN_COEF_N = 9;
constexpr int VN_COEF_MAXBLK = 256;           // cap of the reduction grids: every partial sums a fixed set of rows

// Row-wise routes, after vn_seed_launch and before the terms' seed kernels (udbar still unscaled by D(u)).
struct VnCoefRowsArgs {
  const float* u;                            // [nT] network value per row
  const float* udbar;                        // [nT] s_r: the tangent seed vn_seed_kernel wrote
  const float* rate;                         // [nT] or nullptr (rate == 1); read only with a masked reaction entry
  const float* Nrow; const float* feN;       // N_p of a row: Nrow[r] if given, else feN[r % q]
  const float* phi;                          // [nT] flux stream, or nullptr: the batch has no flux term
  const float* A;                            // [nT] A_r saved by vn_nldiff_fold_kernel, or nullptr: no D(u)
  long nT; int q;
  int react;                                 // the batch has a reaction term
  unsigned mask;                             // bit i: entry i is learnt
  float* part;                               // [blocks, 9] out
};
int vn_coefgrad_blocks(long n);              // blocks either reduction launches for n threads' worth of work (<= VN_COEF_MAXBLK)
hipError_t vn_coefgrad_rows_launch(const VnCoefRowsArgs& a, int* blocks, hipStream_t s);

// De-duplicated step, after the terms' gather kernels, which stored accR_j, accF_j, gs_j.
struct VnCoefPointsArgs {
  const float* upack;                        // [U, 4], u_j at offset 0
  const float* accR; const float* accF; const float* gs;   // [U] each, or nullptr: the batch has no such term
  long U;
  unsigned mask;
  float* part;                               // [blocks, 9] out
};
hipError_t vn_coefgrad_points_launch(const VnCoefPointsArgs& a, int* blocks, hipStream_t s);

// One block: grad[i] = sum over the partials in index order, in fp64 (blocks > 0; else grad as it stands), then with `update`
// the Adam step of the masked entries and the clamp.
struct VnCoefApplyArgs {
  const float* part; int blocks;
  double* grad;                              // [9]
  float* coef; float* m; float* v;           // [9] each
  unsigned mask;
  float lo[VN_COEF_N], hi[VN_COEF_N];
  int update;
  float lr_t, b1, b2, eps;
};
hipError_t vn_coef_apply_launch(const VnCoefApplyArgs& a, hipStream_t s);
