// Boundary-flux rows (vn_set_flux_bc): the seed kernel and the reduction's extra operand, vn_generic.hip.  Kept out of
// vn_internal.h, which every kernel's source hash covers.
#pragma once
#include "vn_internal.h"

// Values u and normal derivatives ud = n . grad_x u of the flux rows in hand: residual r = ud + c u - l, per-block partials of
// biDimVal r^2, seeds ubar = 2 w0 biDimVal c r / nF, udbar = 2 w0 biDimVal r / nF.
struct VnFluxSeedArgs {
  const float* u; const float* ud;          // [nF]
  const float* coef; const float* label;    // [nF]: b/a, g/a
  long nF; float biDimVal, w0;
  float* ubar; float* udbar;                // [nF] out (nullptr: loss only)
  float* part;                              // [vn_flux_seed_blocks(nF)] out
};
int vn_flux_seed_blocks(long nF);
hipError_t vn_flux_seed_launch(const VnFluxSeedArgs& a, hipStream_t s);

// What the reduction folds in from the flux rows: their gradient partials, and the BC component's second mean
// (sum of the nlp loss partials) / nF.  Default: none (the reduction is then exactly the one without flux rows).
struct VnFluxSum {
  const float* partial = nullptr; int nparts = 0;   // [nparts, P] or none (loss only)
  const float* loss = nullptr; int nlp = 0;         // [nlp] partials of biDimVal * sum r^2
  long nF = 0;
};
// vn_reduce_launch (vn_internal.h) plus the flux rows' gradient partials and BC mean
hipError_t vn_reduce_launch(const float* partial, int nparts, int P, const float* losspart, int nlossparts, long bDof, long nB,
                            float w0, float w1, float w2, float* gradbuf, hipStream_t s, VnOptArgs opt, const VnFluxSum& flux);
