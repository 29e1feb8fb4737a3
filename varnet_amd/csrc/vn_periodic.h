// Periodic boundary pairs (vn_set_periodic): the seed kernel (vn_periodic.hip) and what the step's reduction folds in from the
// paired rows, next to the boundary-flux rows' operand.  Kept out of vn_internal.h, which every kernel's source hash covers.
#pragma once
#include "vn_flux.h"
#include "vn_obs.h"

// Values u and directional derivatives ud = d . grad_x u of the 2 nP paired rows in hand (row i pairs with row i + nP):
// r0 = u_i - u_{i+nP}, r1 = ud_i - ud_{i+nP}, per-block partials of biDimVal (r0^2 + gamma r1^2), seeds
// ubar_i = s r0, ubar_{i+nP} = -s r0, udbar_i = s gamma r1, udbar_{i+nP} = -s gamma r1 with s = 2 w0 biDimVal / nP.
// gamma == 0: the values alone -- ud and udbar are nullptr, no tangent seed is produced.
struct VnPeriodicSeedArgs {
  const float* u; const float* ud;          // [2 nP]; ud nullptr: gamma == 0
  long nP; float gamma, biDimVal, w0;
  float* ubar; float* udbar;                // [2 nP] out (nullptr: loss only)
  float* part;                              // [vn_periodic_seed_blocks(nP)] out
};
int vn_periodic_seed_blocks(long nP);
hipError_t vn_periodic_seed_launch(const VnPeriodicSeedArgs& a, hipStream_t s);

// What the reduction adds to the interior and BC/IC rows: the boundary-flux rows' operand, then the periodic pairs' (the same
// kind: gradient partials, loss partials, and the number of rows -- here pairs -- of the mean), then the observations' (vn_obs.h:
// the same kind, with the term's weight and the slot of its misfit).  Default: none of them.
struct VnEdgeSums {
  VnFluxSum flux;
  VnFluxSum per;
  VnObsSum obs;
};
// vn_reduce_launch (vn_internal.h) plus the three operands; with `per` and `obs` empty exactly the reduction of vn_flux.h
hipError_t vn_reduce_launch(const float* partial, int nparts, int P, const float* losspart, int nlossparts, long bDof, long nB,
                            float w0, float w1, float w2, float* gradbuf, hipStream_t s, VnOptArgs opt, const VnEdgeSums& sums);
