// Host-side declarations of vn_source.hip: source identification (vn_set_source_basis, vn_set_source_learn).  The source of a
// batch is s0 + sum_j a_j phi_j over J <= VN_SRC_MAX per-row basis streams; the amplitudes a_j are learnt next to the
// parameters.  Kept out of vn_internal.h, which every kernel's source hash covers.
#pragma once
#include "vn_internal.h"

constexpr int VN_SRC_JMAX = 64;              // == VN_SRC_MAX of the public header
constexpr int VN_SRC_JG = 8;                 // streams one workgroup of the gradient reduction carries
constexpr int VN_SRC_MAXBLK = 256;           // cap of the reduction grid along the rows: every partial sums a fixed set of rows

// s_mix[r] = s0[r] + sum_j amp[j] phi[j, r]: fp32, from s0[r], j ascending, one fused multiply-add per stream.
struct VnSrcMixArgs {
  const float* s0;                           // [nT]
  const float* phi;                          // [J, nT] stream-major
  const float* amp;                          // [J] device
  int J; long nT;
  float* out;                                // [nT]
};
hipError_t vn_source_mix_launch(const VnSrcMixArgs& a, hipStream_t s);

// part[b, j] = - sum_{r in block b's rows} s_r N_p(r) phi[j, r] for the masked j (0 for the others).
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

// One block: grad[j] = sum over the partials in index order, in fp64 (blocks > 0; else grad as it stands), then with `update`
// the Adam step of the masked entries and the clamp.
struct VnSrcApplyArgs {
  const float* part; int blocks; int J;
  double* grad;                              // [J]
  float* amp; float* m; float* v;            // [J] each
  const float* lo; const float* hi;          // [J] each, device (+-inf: unbounded)
  unsigned long long mask;
  int update;
  float lr_t, b1, b2, eps;
};
hipError_t vn_source_apply_launch(const VnSrcApplyArgs& a, hipStream_t s);
