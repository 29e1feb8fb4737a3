// Observations (vn_set_observations): the seed kernel and the registration check (vn_obs.hip), and what the step's reduction
// folds in from the observed points, after the boundary-flux rows' and the periodic pairs' operands.  Kept out of vn_internal.h,
// which every kernel's source hash covers.
#pragma once
#include "vn_flux.h"

// Values u and directional derivatives ud = g . grad_x u of the n registered points in hand.  Observation i owns the points
// [rowptr[i], rowptr[i+1]) (rowptr nullptr: the point i alone):
//   l_i = sum_j (q_j u_j + ud_j),   r_i = l_i - value_i,   per-block partials of wgt_i r_i^2,
//   seeds ubar_j = s_i q_j, udbar_j = s_i with s_i = 2 lambda wgt_i r_i / nO.
// q nullptr: all 1; wgt nullptr: all 1; ud nullptr: no directions were registered -- no tangent stream, no derivative seed.
struct VnObsSeedArgs {
  const float* u; const float* ud;          // [n]; ud nullptr: values only
  const float* q;                           // [n] or nullptr
  const int* rowptr;                        // [nO + 1] or nullptr
  const float* value; const float* wgt;     // [nO]; wgt nullptr: 1
  long nO; float lambda;
  float* ubar; float* udbar;                // [n] out (nullptr: loss only)
  float* part;                              // [vn_obs_seed_blocks(nO)] out
};
int vn_obs_seed_blocks(long nO);
hipError_t vn_obs_seed_launch(const VnObsSeedArgs& a, hipStream_t s);

// *err_dev += number of violations of a registration: rowptr[0] == 0, rowptr strictly increasing, rowptr[nO] == n; value finite;
// wgt finite and >= 0; q and dir finite.  q, dir, rowptr, wgt may be nullptr (not checked then); err_dev must hold 0 on entry.
hipError_t vn_obs_check_launch(const float* q, const float* dir, const int* rowptr, const float* value, const float* wgt,
                               long n, long nO, int dim, int* err_dev, hipStream_t s);

// The reduction's operand: gradient partials and loss partials like the other two (nF: the number of observations nO), the
// weight lambda of the term in the loss, and the device slot that receives the unweighted misfit O = sum / nO.
struct VnObsSum {
  VnFluxSum sum;
  float lambda = 0.f;
  double* misfit = nullptr;
};
