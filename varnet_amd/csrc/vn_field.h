// Host-side declarations of vn_field.hip: field identification (vn_set_field_basis, vn_set_field_learn).  The tangent direction
// of a batch is gcoef = g0 + sum_j b_j G_j over J <= VN_FLD_MAX per-row basis streams of dim floats per row; the amplitudes b_j
// (of a diffusivity and a velocity basis: the engine does not know which stream is which) are learnt next to the parameters.
// The mix and the fold / Adam step / clamp are those of vn_source.hip through its launchers; only the reduction is new.
// Kept out of vn_internal.h, which every kernel's source hash covers.
#pragma once
#include "vn_internal.h"

constexpr int VN_FLD_JMAX = 32;              // == VN_FLD_MAX of the public header
constexpr int VN_FLD_JG = 8;                 // streams one workgroup of the gradient reduction carries
constexpr int VN_FLD_MAXBLK = 256;           // cap of the reduction grid along the rows: every partial sums a fixed set of rows

// part[b, j] = + sum_{r in block b's rows} s_r (grad u_r . G[j, r, :]) for the masked j (0 for the others).
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
