// Edge row sets: rows the network is evaluated on beside a batch -- boundary-flux rows (vn_set_flux_bc), periodic pairs
// (vn_set_periodic), observations (vn_set_observations).  Each set takes the same route (vn_api.hip, edge_pass): the generic
// forward kernel with the set's directions as tangents, the set's seed kernel (vn_edge.hip), the generic reverse kernel into
// partials of the set's own, and one operand of the step's reduction (vn_generic.hip).  Kept out of vn_internal.h, which every
// kernel's source hash covers.
#pragma once
#include "vn_internal.h"

// The sets, in the order in which every pass runs and every sum is folded.
enum VnEdgeId { VN_EDGE_FLUX, VN_EDGE_PERIODIC, VN_EDGE_OBS, VN_EDGE_N };

// Boundary-flux rows.  Values u and normal derivatives ud = n . grad_x u of the nF rows in hand: residual r = ud + c u - l,
// per-block partials of biDimVal r^2, seeds ubar = 2 w0 biDimVal c r / nF, udbar = 2 w0 biDimVal r / nF.
struct VnFluxSeedArgs {
  const float* u; const float* ud;          // [nF]
  const float* coef; const float* label;    // [nF]: b/a, g/a
  long nF; float biDimVal, w0;
  float* ubar; float* udbar;                // [nF] out (nullptr: loss only)
  float* part;                              // [vn_edge_seed_blocks(nF)] out
};
hipError_t vn_flux_seed_launch(const VnFluxSeedArgs& a, hipStream_t s);

// Periodic pairs.  Values u and directional derivatives ud = d . grad_x u of the 2 nP paired rows in hand (row i pairs with row
// i + nP): r0 = u_i - u_{i+nP}, r1 = ud_i - ud_{i+nP}, per-block partials of biDimVal (r0^2 + gamma r1^2), seeds
// ubar_i = s r0, ubar_{i+nP} = -s r0, udbar_i = s gamma r1, udbar_{i+nP} = -s gamma r1 with s = 2 w0 biDimVal / nP.
// gamma == 0: the values alone -- ud and udbar are nullptr, no tangent seed is produced.
struct VnPeriodicSeedArgs {
  const float* u; const float* ud;          // [2 nP]; ud nullptr: gamma == 0
  long nP; float gamma, biDimVal, w0;
  float* ubar; float* udbar;                // [2 nP] out (nullptr: loss only)
  float* part;                              // [vn_edge_seed_blocks(nP)] out
};
hipError_t vn_periodic_seed_launch(const VnPeriodicSeedArgs& a, hipStream_t s);

// Observations.  Values u and directional derivatives ud = g . grad_x u of the n registered points in hand.  Observation i owns
// the points [rowptr[i], rowptr[i+1]) (rowptr nullptr: the point i alone):
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
  float* part;                              // [vn_edge_seed_blocks(nO)] out
};
hipError_t vn_obs_seed_launch(const VnObsSeedArgs& a, hipStream_t s);

// Loss partials a seed kernel writes for `count` rows, pairs or observations: one thread each, one partial per block.
int vn_edge_seed_blocks(long count);

// *err_dev += number of violations of a registration: rowptr[0] == 0, rowptr strictly increasing, rowptr[nO] == n; value finite;
// wgt finite and >= 0; q and dir finite.  q, dir, rowptr, wgt may be nullptr (not checked then); err_dev must hold 0 on entry.
hipError_t vn_obs_check_launch(const float* q, const float* dir, const int* rowptr, const float* value, const float* wgt,
                               long n, long nO, int dim, int* err_dev, hipStream_t s);

// What the reduction folds in from one set: its gradient partials, and the mean (sum of the nlp loss partials) / count.
// Default: none (the reduction is then exactly the one without the set).
struct VnEdgeSum {
  const float* partial = nullptr; int nparts = 0;   // [nparts, P] or none (loss only)
  const float* loss = nullptr; int nlp = 0;         // [nlp] partials of the set's sum of squares
  long count = 0;                                   // rows, pairs or observations the mean divides by
};
// The three operands in VnEdgeId order.  The flux rows' and the pairs' means join the BC component; the observations' mean is
// the unweighted misfit O: it goes to the device slot `misfit` and enters the loss as lambda O.
struct VnEdgeSums {
  VnEdgeSum set[VN_EDGE_N];
  float lambda = 0.f;
  double* misfit = nullptr;
};
// vn_reduce_launch (vn_internal.h) plus the three operands
hipError_t vn_reduce_launch(const float* partial, int nparts, int P, const float* losspart, int nlossparts, long bDof, long nB,
                            float w0, float w1, float w2, float* gradbuf, hipStream_t s, VnOptArgs opt, const VnEdgeSums& sums);
