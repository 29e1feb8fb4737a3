// The training objective of a batch and its gradient in double precision (vn_objective_f64): vn_obj64.hip.  Kept out of
// vn_internal.h, which every kernel's source hash covers.
#pragma once
#include "vn_internal.h"
#include "vn_weights.h"
#include "vn_bicadapt.h"

// Engine-owned work buffers of the evaluation, sized at the call that first needs them and released by vn_obj64_free.
struct VnObj64Work {
  double* img = nullptr;   long img_cap = 0;     // zero-padded weight images of theta
  double* u = nullptr;     long u_cap = 0;       // [rows]: forward values, then the value seeds in place
  double* ud = nullptr;    long ud_cap = 0;      // [rows]: directional derivatives, then the tangent seeds in place
  double* act = nullptr;   long act_cap = 0;     // [waves][L][2][16][64]: a wave's activations of its current chunk
  double* part = nullptr;  long part_cap = 0;    // [waves][gradient image]
  double* lpart = nullptr; long lpart_cap = 0;   // [seed blocks][4]: var, bc, ic, flux partial sums; then [seed blocks]: periodic pairs; then [seed blocks]: observations
  double* out = nullptr;                         // [4] loss, BC, IC, var
  // per-test-function loss weights (vn_weights.hip), allocated by the first evaluation of a batch that has them
  double* lvec = nullptr;  long lvec_cap = 0;    // [n_k] the loss field when the caller passes none
  double* omega = nullptr; long omega_cap = 0;   // [n_k] omega_k in double
  double* wstat = nullptr; long wstat_cap = 0;   // causal: lsum [S * chunks], then omega_s [S]
  // weights on the BC/IC rows (vn_bicadapt.hip), allocated by the first evaluation that has them
  double* bwpart = nullptr; long bwpart_cap = 0; // [row blocks][2]: weighted bc, ic partial sums
};

// What the evaluation reads: the batch as registered (fp32 device arrays, widened exactly by the kernels).
struct VnObj64Problem {
  VnNet net;
  const double* theta;                                   // [P] device
  // interior rows
  const float* X; const float* G; const float* src;      // [n_k*q, d_in], [n_k*q, dim], [n_k*q] or nullptr
  const float* feN; const float* fedNt; const float* feW;
  const float* Nrow; const float* dNtrow; const float* detJv;
  double detJ; long n_k; int q; int td;
  // BC / IC rows
  const float* Xb; const float* label; long nB, bDof; double biDimVal;
  // boundary-flux rows
  const float* Xf; const float* Nf; const float* fcoef; const float* flabel; long nF; double fbiDimVal;
  // periodic pairs (vn_set_periodic): rows i and i + nP pair, Dp the common direction (nullptr with pgamma == 0); nP == 0: none
  const float* Xp; const float* Dp; long nP; double pgamma, pbiDimVal;
  // observations (vn_set_observations): on points in nO segments (orowptr nullptr: one point each); Qo, Do, owgt may be nullptr;
  // omisfit: device slot of the unweighted misfit; nO == 0: none
  const float* Xo; const float* Qo; const float* Do; const int* orowptr; const float* ovalue; const float* owgt;
  long on, nO; double olambda; double* omisfit;
  double w[3];
  // reaction term of the batch (vn_set_reaction): rate [n_k*q] or nullptr (1), coef c1..c3; react == 0: none
  int react; const float* rate; double coef[3];
  // flux term of the batch (vn_set_nlflux): phi [n_k*q], coefficients f1..f3; nlflux == 0: none
  int nlflux; const float* phi; double fcoef3[3];
  // diffusivity D(u) of the batch (vn_set_nldiff): psi [n_k*q] or nullptr, coefficients d0..d2; nldiff == 0: none
  int nldiff; const float* psi; double dcoef3[3];
  // per-test-function loss weights of the batch (vn_set_tf_weights / vn_set_causal); default: none
  VnWeightsReg wt;
  // weights on the BC/IC rows (vn_set_bic_weights / vn_set_bic_adapt): the committed omega of bc [bDof] and ic [nB - bDof], fp32,
  // widened exactly; nullptr: 1; default: none
  const float* bic_omega[2];
};

bool vn_obj64_supported(const VnNet& net);
// loss components into out_host[4]; grad_dev [P] and lossVec_dev [n_k] optional.  Synchronises the stream.
hipError_t vn_obj64_run(VnObj64Work& w, const VnObj64Problem& p, double* grad_dev, double* lossVec_dev, double out_host[4],
                        int ncu, hipStream_t s);
void vn_obj64_free(VnObj64Work& w);
