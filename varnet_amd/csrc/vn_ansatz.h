// Host-side declarations of vn_ansatz.hip: the hard-constraint ansatz u = A + B n around the network output n (maths and
// order contract: that file's header).  Kept out of vn_internal.h, which every kernel's source hash covers.
#pragma once
#include <hip/hip_runtime.h>

// One row set: the batch's interior rows, the BC/IC rows, or the rows of an edge set.  The same record serves the fold (v = u,
// vd = ud) and the adjoint (v = ubar, vd = udbar); both work in place.
struct VnAnsatzRowArgs {
  const float* A;                            // [n] or nullptr (zero): the data-carrying part              (fold only)
  const float* B;                            // [n] the factor that vanishes where the data must hold
  const float* a;                            // [n] or nullptr (zero): grad_x A . G_r along the row's direction  (fold only)
  const float* b;                            // [n] or nullptr (zero): grad_x B . G_r
  long n;
  float* v;                                  // [n] in/out: network value -> u            | value seed ubar -> seed of n
  float* vd;                                 // [n] in/out, or nullptr (a values-only set): tangent -> ud  | udbar -> seed of nd
};
// u[r] = A + B n;  ud[r] = a + b n + B nd   (n read before it is overwritten)
hipError_t vn_ansatz_fold_launch(const VnAnsatzRowArgs& r, hipStream_t s);
// ubar[r] = B ubar + b udbar;  udbar[r] = B udbar   (udbar nullptr: ubar[r] *= B)
hipError_t vn_ansatz_adjoint_launch(const VnAnsatzRowArgs& r, hipStream_t s);

// The unique points of a de-duplication map: the [U, 4] record (u, grad u) of the point pass and the gathered seeds.
struct VnAnsatzPointArgs {
  const float* A;                            // [U] or nullptr (zero)                                       (fold only)
  const float* B;                            // [U]
  const float* gA;                           // [U, dim] or nullptr (zero): grad_x A                        (fold only)
  const float* gB;                           // [U, dim] or nullptr (zero): grad_x B
  long U; int dim;                           // dim <= 3
  float* pack;                               // [U, 4] in/out: (n, grad n) -> (u, grad u), the value at offset 0   (fold only)
  float* seed_u;                             // [U] in/out                                                  (adjoint only)
  float* seed_g;                             // [U, dim] in/out                                             (adjoint only)
};
// u_j = A + B n;  grad u_j = grad A + n grad B + B grad n
hipError_t vn_ansatz_points_fold_launch(const VnAnsatzPointArgs& p, hipStream_t s);
// su_j = B su + grad B . sg (the sg of before);  sg_j = B sg
hipError_t vn_ansatz_points_adjoint_launch(const VnAnsatzPointArgs& p, hipStream_t s);

// *err_dev += number of non-finite entries of p[0 .. n); p nullptr or n <= 0: nothing launched.  err_dev holds 0 on entry
// or the count of the streams checked before this one.
hipError_t vn_ansatz_check_launch(const float* p, long n, int* err_dev, hipStream_t s);
