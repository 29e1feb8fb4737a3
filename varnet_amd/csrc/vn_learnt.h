// Host-side declarations of vn_learnt.hip: the vectors learnt next to the parameters -- the nine polynomial coefficients of
// vn_terms.hip (vn_set_coef_learn; index 0..2 reaction, 3..5 flux, 6..8 diffusivity), the source amplitudes (vn_set_source_learn)
// the field amplitudes (vn_set_field_learn), the boundary / initial amplitudes (vn_set_bic_learn) and the flux-row amplitudes
// (vn_set_fluxbc_learn) -- their mix, their gradient reductions and their Adam step.  Kept out of vn_internal.h, which every kernel's source hash covers.
#pragma once
#include "vn_internal.h"

constexpr int VN_COEF_N = 9;
constexpr int VN_SRC_JMAX = 64;              // == VN_SRC_MAX of the public header
constexpr int VN_FLD_JMAX = 32;              // == VN_FLD_MAX of the public header
constexpr int VN_BIC_JMAX = 64;              // == VN_BIC_MAX of the public header
constexpr int VN_FBC_JMAX = 64;              // == VN_FBC_MAX of the public header
constexpr int VN_LEARNT_JG = 8;              // streams one workgroup of an amplitude reduction carries
constexpr int VN_LEARNT_MAXBLK = 256;        // cap of every reduction grid along the rows: a partial sums a fixed set of rows

// out[r] = base[r] + sum_j amp[j] stream[j, r]: fp32, from base[r], j ascending, one fused multiply-add per stream.  The source of
// a batch (n = nT), its tangent direction gcoef (n = nT dim), the labels of a BC/IC row set (n = nB) and the flux datum and Robin
// coefficient of the flux rows (n = nF, one launch each) are all formed by it.
struct VnMixArgs {
  const float* base;                         // [n]
  const float* stream;                       // [J, n] stream-major
  const float* amp;                          // [J] device
  int J; long n;
  float* out;                                // [n]
};
hipError_t vn_learnt_mix_launch(const VnMixArgs& a, hipStream_t s);

// ---- coefficients.  Row-wise routes, after vn_seed_launch and before the terms' seed kernels (udbar still unscaled by D(u)).
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

// ---- source amplitudes.  part[b, j] = - sum_{r in block b's rows} s_r N_p(r) phi[j, r] for the masked j (0 for the others).
// Row-wise routes: s_r = udbar[r], after vn_seed_launch and before the terms' seed kernels (udbar still unscaled by D(u)).
// De-duplicated step: udbar == nullptr and s_r = stf[r / q] * feW[r % q] (feW nullptr: 1), after vn_dedup_seed_launch.
struct VnSrcGradArgs {
  const float* udbar;                        // [nT] or nullptr
  const float* stf; const float* feW;        // [n_k], [q] or nullptr
  const float* Nrow; const float* feN;       // N_p of a row: Nrow[r] if given, else feN[r % q]
  const float* phi;                          // [J, nT]
  int J; long nT; int q;
  unsigned long long mask;                   // bit j: amplitude j is learnt
  float* part;                               // [blocks, J] out
};
hipError_t vn_srcgrad_rows_launch(const VnSrcGradArgs& a, int* blocks, hipStream_t s);

// ---- field amplitudes.  part[b, j] = + sum_{r in block b's rows} s_r (grad u_r . G[j, r, :]) for the masked j (0 for the others).
// Row-wise routes: s_r = udbar[r] AFTER vn_nldiff_seed_launch rescaled it by D(u_r) (the row integrand is D(u) (grad u . gcoef));
//   (u, grad u) of row r is the record pack[r] of a point pass over the batch's own rows; uid == nullptr.
// De-duplicated step: udbar == nullptr, s_r = stf[r / q] * feW[r % q] (feW nullptr: 1) * D(u_j), j = uid[r], with (u, grad u) the
//   record pack[j] of the unique points; D(u) = c[0] + c[1] u + c[2] u^2 when nldiff (cp: the three on the device, else c).
struct VnFldGradArgs {
  const float* udbar;                        // [nT] or nullptr
  const float* stf; const float* feW;        // [n_k], [q] or nullptr
  const float* pack;                         // [nT, 4] (uid == nullptr) or [U, 4]: (u, du/dx_0, du/dx_1, du/dx_2)
  const int* uid;                            // [nT] row -> record, or nullptr: the row's own
  const float* G;                            // [J, nT, dim] stream-major
  int nldiff; float c[3]; const float* cp;   // D(u) of the de-duplicated step
  int J, dim; long nT; int q;
  unsigned mask;                             // bit j: amplitude j is learnt
  float* part;                               // [blocks, J] out
};
hipError_t vn_fldgrad_rows_launch(const VnFldGradArgs& a, int* blocks, hipStream_t s);

// ---- boundary / initial amplitudes.  part[b, j] = - sum_{k in block b's rows} ubar_b[k] B[j, k] for the masked j (0 for the
// others), over the rows k < (steady ? bDof : nB); ubar_b[k] = vn_bic_value_seed(k, ub[k] - label[k], ...) of vn_bicseed.h, the
// value vn_seed_kernel stores for the row.  After the forward of the BC/IC rows, on every route; reads no seed buffer.
struct VnBicGradArgs {
  const float* ub;                           // [rows] network value per BC/IC row
  const float* label;                        // [nB] the mixed label the step reads
  const float* B;                            // [J, nB] stream-major
  int J; long nB, bDof;                      // nB: rows of a stream (and the stride between two)
  int steady;                                // the problem has no initial rows: [bDof, nB) are never evaluated
  float biDimVal, w0, w1;
  unsigned long long mask;                   // bit j: amplitude j is learnt
  float* part;                               // [blocks, J] out
};
hipError_t vn_bicgrad_launch(const VnBicGradArgs& a, int* blocks, hipStream_t s);

// ---- flux-row amplitudes.  The flux rows' residual is r_k = ud_k + coef[k] u_k - label[k] with label = label0 + sum_{j < Jl} a_j
// S[j, :] and coef = coef0 + sum_{j >= Jl} a_j S[j, :].  part[b, j] = sum_{k in block b's rows} w_j[k] S[j, k] for the masked j (0 for
// the others) with the row weight w_j[k] = - udbar[k] for j < Jl (the flux datum) and + udbar[k] u[k] for j >= Jl (the Robin
// coefficient); udbar[k] = d loss / d r_k as vn_flux_seed_kernel stores it.  After the flux set's edge pass of a gradient
// evaluation, whose value and seed buffers it reads.
struct VnFbcGradArgs {
  const float* u;                            // [nF] network value per flux row
  const float* udbar;                        // [nF] the tangent seed of the row
  const float* S;                            // [J, nF] stream-major: Jl streams of the flux datum, then J - Jl of the coefficient
  int J, Jl; long nF;
  unsigned long long mask;                   // bit j: amplitude j is learnt
  float* part;                               // [blocks, J] out
};
hipError_t vn_fbcgrad_launch(const VnFbcGradArgs& a, int* blocks, hipStream_t s);

// ---- every vector.  One block: grad[j] = sum over the [blocks, J] partials in fp64 (blocks > 0; else grad as it stands), then
// with `update` the Adam step of the masked entries and the clamp.  `lanes` (16 or 64) is the fold's lane-group width: 256 / lanes
// groups each sum their chunk of the blocks in index order, then the group sums are added in group order.
// Prior (weight > 0): the fold adds weight (R (val - mean))_j in fp64 to the masked entries' gradient (blocks > 0 only), with val
// as the gradient evaluation read it.  l1: the update ends in the shrinkage by lr_t l1[j], before the clamp.  pen: evaluate only.
struct VnLearntApplyArgs {
  const float* part; int blocks; int J;
  double* grad;                              // [J]
  float* val; float* m; float* v;            // [J] each
  const float* lo; const float* hi;          // [J] each, device (+-inf: unbounded)
  unsigned long long mask;
  int update;
  float lr_t, b1, b2, eps;
  int lanes;
  const double* R;                           // [J, J] symmetric, device, or nullptr: the identity
  const double* mean;                        // [J] device (read with weight > 0)
  double weight;                             // alpha of 1/2 alpha d^T R d; 0: no quadratic prior
  const float* l1;                           // [J] device, or nullptr: no shrinkage
  double* pen;                               // [2] device, or nullptr; given: no fold, no update, pen = (Q, sum_j l1[j] |val[j]|)
};
hipError_t vn_learnt_apply_launch(const VnLearntApplyArgs& a, hipStream_t s);
