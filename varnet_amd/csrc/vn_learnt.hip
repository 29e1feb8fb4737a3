// The vectors learnt next to the parameters: their mix into the streams a step reads, the gradient of the loss with respect to
// them, and their optimizer step.
//   coefficients (vn_set_coef_learn)     the nine polynomial coefficients of vn_terms.hip: 0..2 = (c1, c2, c3) reaction, 3..5 =
//                                        (f1, f2, f3) flux, 6..8 = (d0, d1, d2) D(u).  The term kernels read them from the device.
//   source amplitudes (vn_set_source_*)  the source of a batch is s0(r) + sum_j a_j phi_j(r) over J <= 64 per-row streams.
//   field amplitudes (vn_set_field_*)    the tangent direction of a batch is gcoef_r = g0_r + sum_j b_j G_j[r, :] over J <= 32
//                                        streams of dim floats per row (G_j = chi_j dN/dx for a diffusivity stream, omega_j N for a
//                                        velocity stream; the engine does not know which is which).
//   boundary / initial amplitudes        the labels of a BC/IC row set are label0[k] + sum_j a_j B_j[k] over J <= 64 per-row streams
//   (vn_set_bic_*)                       (a Dirichlet basis stream is zero on the initial rows and on other edges, an initial one on
//                                        the boundary rows; the engine does not know which is which).
//   flux-row amplitudes (vn_set_fluxbc_*) the flux rows' residual ud_k + coef[k] u_k - label[k] reads label = label0 + sum_{j < Jl} a_j S_j
//                                        and coef = coef0 + sum_{j >= Jl} a_j S_j over J <= 64 per-row streams, the Jl of the flux datum
//                                        first: one vector, two mixes.
// Mix (vn_learnt_mix_kernel and its 4-row form): base + Sum_j amp[j] stream[j], which every kernel of the step then reads in
// place of the batch's source (n = nT), gcoef (n = nT dim), BC/IC labels (n = nB) or the flux rows' label and coefficient (n = nF).
//
// Gradients.  With u_r, A_r = grad u_r . gcoef_r, N_p, rate_r, phi_r as in vn_terms.hip's header, the row integrand is
// t_r = D(u_r) A_r - (source + reaction) N_p - flux (D = 1 without vn_set_nldiff), and seed_r is the tangent seed of row r:
//   d loss / d c_m = - sum_r seed_r N_p rate_r u_r^m     m = 1, 2, 3   (rate_r = 1 when the stream is null)
//   d loss / d f_m = - sum_r seed_r phi_r u_r^m          m = 1, 2, 3
//   d loss / d d_m = + sum_r seed_r A_r u_r^m            m = 0, 1, 2
//   d loss / d a_j = - sum_r seed_r N_p phi_j[r]
//   d loss / d b_j = + sum_r seed_r (grad u_r . G_j[r, :])
// and over the BC/IC rows k, with ubar_b[k] the value seed of row k (vn_bicseed.h; the label enters through u_b[k] - label[k] only),
//   d loss / d a_j = - sum_k ubar_b[k] B_j[k]       k < bDof on a steady problem, whose initial rows are never evaluated
// and over the flux rows k, with udbar[k] = d loss / d r_k the tangent seed vn_flux_seed_kernel stores,
//   d loss / d a_j = - sum_k udbar[k] S_j[k]  (j < Jl),    d loss / d a_j = + sum_k udbar[k] u[k] S_j[k]  (j >= Jl)
// Where each reads its seed.  The coefficients and the source read udbar[r] as vn_seed_kernel writes it (2 w2 detJ R_k W_p), BEFORE
// vn_nldiff_seed_kernel rescales it by D(u); the field reads it AFTER that rescale (its integrand carries D(u)).  On the
// de-duplicated step the source takes seed_r = stf[r / q] W_p with stf the per-test-function seed of vn_dedup_seed_kernel, the
// field that times D(u_j), j = uid[r], with grad u of point j, and the coefficients need no second walk over the rows:
//   d loss / d c_m = - sum_j u_j^m accR_j,  d loss / d f_m = - sum_j u_j^m accF_j,  d loss / d d_m = + sum_j u_j^m gs_j
// with accR_j, accF_j the CSR sums of vn_react_gather_kernel / vn_nlflux_gather_kernel and gs_j the dot product
// grad u_j . seed_g[j,:] of vn_nldiff_point_kernel (unscaled seed_g), which those kernels store.
//
// Determinism.  No atomics, plain vector stores.  Every reduction is a grid-stride loop over a capped grid (learnt_blocks), so a
// partial covers a fixed set of rows; fp32 accumulators per thread in compile-time-indexed registers (no scratch at any J), for
// the masked entries only; per block the order of block_sum (vn_blocksum.h); one [blocks, J] partial array per vector, folded in
// fp64 in index order by the single block of vn_learnt_apply_kernel, which also takes the Adam step and clamps.  Two evaluations
// give the same bits.  The amplitude reductions run on a grid (row blocks, ceil(J / 8)): a workgroup carries eight streams and
// re-reads the seed once per group.  All HBM-bound.  The source and the field reduction stay two kernels over the shared helpers:
// the source has a 4-row form with its own weight paths, the field a record load and DIM products per stream.
#include "vn_bicseed.h"
#include "vn_blocksum.h"
#include "vn_learnt.h"
#include "vn_rows4.h"

namespace {

constexpr int TB = 256;
constexpr int JG = VN_LEARNT_JG;

// ---- what the reductions share ----
// blocks a reduction launches for n threads' worth of work
int learnt_blocks(long n) {
  const long b = (n + TB - 1) / TB;
  return (int)(b < 1 ? 1 : b < VN_LEARNT_MAXBLK ? b : VN_LEARNT_MAXBLK);
}

// the learnt streams of this workgroup's group of eight, as bits 0..7
template <class Args>
__device__ __forceinline__ unsigned group_mask(const Args& a, int j0) {
  const int left = a.J - j0;
  const unsigned in = left >= JG ? 0xFFu : (1u << left) - 1u;
  return (unsigned)(a.mask >> j0) & in;
}

// One partial: the block's sum of a masked accumulator (0 for the others), stored to part[i] by the one thread that has `store`,
// negated where the term enters the row integrand with a minus.  (`on` is uniform: every thread takes the same branch.)
__device__ __forceinline__ void write_partial(float acc, bool on, bool minus, bool store, float* part, long i) {
  __shared__ float red[4];
  float t = 0.f;
  if (on) t = block_sum(acc, red);
  if (store) part[i] = minus ? -t : t;
}

// the eight partials of an amplitude reduction's workgroup
__device__ __forceinline__ void write_group(const float* acc, unsigned m, bool minus, int j0, int J, float* part) {
#pragma unroll
  for (int c = 0; c < JG; ++c) write_partial(acc[c], m >> c & 1u, minus, threadIdx.x == 0 && j0 + c < J, part, (long)blockIdx.x * J + j0 + c);
}

// ---- mix ----
__global__ __launch_bounds__(TB) void vn_learnt_mix_kernel(VnMixArgs a) {
  const long r = (long)blockIdx.x * TB + threadIdx.x;
  if (r >= a.n) return;
  float s = a.base[r];
#pragma unroll 8
  for (int j = 0; j < a.J; ++j) s = fmaf(a.amp[j], a.stream[(long)j * a.n + r], s);
  a.out[r] = s;
}

__global__ __launch_bounds__(TB) void vn_learnt_mix4_kernel(VnMixArgs a) {           // n % 4 == 0, 16-byte aligned pointers
  const long i = (long)blockIdx.x * TB + threadIdx.x, n4 = a.n / 4;
  if (i >= n4) return;
  f32x4t s = load4(a.base, i);
#pragma unroll 8
  for (int j = 0; j < a.J; ++j) {
    const float aj = a.amp[j];
    const f32x4t p = load4(a.stream + (long)j * a.n, i);
    s[0] = fmaf(aj, p[0], s[0]); s[1] = fmaf(aj, p[1], s[1]); s[2] = fmaf(aj, p[2], s[2]); s[3] = fmaf(aj, p[3], s[3]);
  }
  store4(a.out, i, s);
}

// ---- coefficients ----
// acc[3 g + m] += w x^(m + first) for the masked entries of group g
__device__ __forceinline__ void add_powers(float* acc, unsigned mask, int g, float w, float x, bool from_one) {
  float p = from_one ? w * x : w;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    if (mask >> (3 * g + m) & 1u) acc[3 * g + m] += p;
    p *= x;
  }
}

__device__ __forceinline__ void add_row(const VnCoefRowsArgs& a, float* acc, long r, float u, float s, float rate, float phi, float A) {
  if (a.react && (a.mask & 0x7u)) {
    const float N = a.Nrow ? a.Nrow[r] : a.feN[r % a.q];
    add_powers(acc, a.mask, 0, a.rate ? s * N * rate : s * N, u, true);
  }
  if (a.phi && (a.mask & 0x38u)) add_powers(acc, a.mask, 1, s * phi, u, true);
  if (a.A && (a.mask & 0x1C0u)) add_powers(acc, a.mask, 2, s * A, u, false);
}

// signs: the reaction and the flux enter the row integrand with a minus
__device__ __forceinline__ void write_coef(const float* acc, unsigned mask, float* part) {
#pragma unroll
  for (int i = 0; i < VN_COEF_N; ++i) write_partial(acc[i], mask >> i & 1u, i < 6, threadIdx.x == 0, part, (long)blockIdx.x * VN_COEF_N + i);
}

__global__ __launch_bounds__(TB) void vn_coefgrad_rows_kernel(VnCoefRowsArgs a) {
  float acc[VN_COEF_N] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool wr = a.react && a.rate && (a.mask & 0x7u), wf = a.phi && (a.mask & 0x38u), wd = a.A && (a.mask & 0x1C0u);
  for (long r = (long)blockIdx.x * TB + threadIdx.x; r < a.nT; r += (long)gridDim.x * TB)
    add_row(a, acc, r, a.u[r], a.udbar[r], wr ? a.rate[r] : 1.f, wf ? a.phi[r] : 0.f, wd ? a.A[r] : 0.f);
  write_coef(acc, a.mask, a.part);
}

__global__ __launch_bounds__(TB) void vn_coefgrad_rows4_kernel(VnCoefRowsArgs a) {     // nT % 4 == 0, 16-byte aligned pointers
  float acc[VN_COEF_N] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool wr = a.react && a.rate && (a.mask & 0x7u), wf = a.phi && (a.mask & 0x38u), wd = a.A && (a.mask & 0x1C0u);
  const f32x4t zero = {0.f, 0.f, 0.f, 0.f}, one = {1.f, 1.f, 1.f, 1.f};
  for (long i = (long)blockIdx.x * TB + threadIdx.x; i < a.nT / 4; i += (long)gridDim.x * TB) {
    const f32x4t u = load4(a.u, i), s = load4(a.udbar, i);
    const f32x4t rt = wr ? load4(a.rate, i) : one, ph = wf ? load4(a.phi, i) : zero, A = wd ? load4(a.A, i) : zero;
#pragma unroll
    for (int c = 0; c < 4; ++c) add_row(a, acc, 4 * i + c, u[c], s[c], rt[c], ph[c], A[c]);
  }
  write_coef(acc, a.mask, a.part);
}

__global__ __launch_bounds__(TB) void vn_coefgrad_points_kernel(VnCoefPointsArgs a) {
  float acc[VN_COEF_N] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long j = (long)blockIdx.x * TB + threadIdx.x; j < a.U; j += (long)gridDim.x * TB) {
    const float u = a.upack[j * 4];
    if (a.accR && (a.mask & 0x7u)) add_powers(acc, a.mask, 0, a.accR[j], u, true);
    if (a.accF && (a.mask & 0x38u)) add_powers(acc, a.mask, 1, a.accF[j], u, true);
    if (a.gs && (a.mask & 0x1C0u)) add_powers(acc, a.mask, 2, a.gs[j], u, false);
  }
  write_coef(acc, a.mask, a.part);
}

// ---- source amplitudes ----
// seed_r N_p of row r
__device__ __forceinline__ float row_weight(const VnSrcGradArgs& a, long r) {
  const int p = (int)(r % a.q);
  const float N = a.Nrow ? a.Nrow[r] : a.feN[p];
  const float s = a.udbar ? a.udbar[r] : (a.feW ? a.stf[r / a.q] * a.feW[p] : a.stf[r / a.q]);
  return s * N;
}

__global__ __launch_bounds__(TB) void vn_srcgrad_rows_kernel(VnSrcGradArgs a) {
  const int j0 = blockIdx.y * JG;
  const unsigned m = group_mask(a, j0);
  float acc[JG] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m)
    for (long r = (long)blockIdx.x * TB + threadIdx.x; r < a.nT; r += (long)gridDim.x * TB) {
      const float w = row_weight(a, r);
#pragma unroll
      for (int c = 0; c < JG; ++c)
        if (m >> c & 1u) acc[c] += w * a.phi[(long)(j0 + c) * a.nT + r];
    }
  write_group(acc, m, true, j0, a.J, a.part);
}

__global__ __launch_bounds__(TB) void vn_srcgrad_rows4_kernel(VnSrcGradArgs a) {     // nT % 4 == 0, 16-byte aligned streams
  const int j0 = blockIdx.y * JG;
  const unsigned m = group_mask(a, j0);
  float acc[JG] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m)
    for (long i = (long)blockIdx.x * TB + threadIdx.x; i < a.nT / 4; i += (long)gridDim.x * TB) {
      f32x4t w;
      if (a.udbar && a.Nrow) {
        w = load4(a.udbar, i) * load4(a.Nrow, i);
      } else if (a.udbar) {
        const f32x4t s = load4(a.udbar, i);
        const int p = (int)((4 * i) % a.q);
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = s[c] * a.feN[(p + c) % a.q];
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = row_weight(a, 4 * i + c);
      }
#pragma unroll
      for (int c = 0; c < JG; ++c)
        if (m >> c & 1u) {
          const f32x4t p = load4(a.phi + (long)(j0 + c) * a.nT, i);
          acc[c] += w[0] * p[0]; acc[c] += w[1] * p[1]; acc[c] += w[2] * p[2]; acc[c] += w[3] * p[3];
        }
    }
  write_group(acc, m, true, j0, a.J, a.part);
}

// ---- field amplitudes ----
template <int DIM>
__global__ __launch_bounds__(TB) void vn_fldgrad_rows_kernel(VnFldGradArgs a) {
  const int j0 = blockIdx.y * JG;
  const unsigned m = group_mask(a, j0);
  const long stride = a.nT * DIM;                                // floats between two streams
  float c0 = 1.f, c1 = 0.f, c2 = 0.f;
  if (a.nldiff) {
    if (a.cp) { c0 = a.cp[0]; c1 = a.cp[1]; c2 = a.cp[2]; }
    else { c0 = a.c[0]; c1 = a.c[1]; c2 = a.c[2]; }
  }
  float acc[JG] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m)
    for (long r = (long)blockIdx.x * TB + threadIdx.x; r < a.nT; r += (long)gridDim.x * TB) {
      const long j = a.uid ? (long)a.uid[r] : r;                 // (uid validated against U by vn_set_dedup)
      const f32x4t pd = load4(a.pack, j);
      float s;
      if (a.udbar) {
        s = a.udbar[r];
      } else {
        s = a.stf[r / a.q];
        if (a.feW) s *= a.feW[r % a.q];
        if (a.nldiff) s *= c0 + pd[0] * (c1 + pd[0] * c2);       // D(u_j), the form of quad() in vn_terms.hip
      }
      float w[DIM];
#pragma unroll
      for (int d = 0; d < DIM; ++d) w[d] = s * pd[1 + d];
#pragma unroll
      for (int c = 0; c < JG; ++c)
        if (m >> c & 1u) {
          const float* g = a.G + (long)(j0 + c) * stride + r * DIM;
#pragma unroll
          for (int d = 0; d < DIM; ++d) acc[c] += w[d] * g[d];
        }
    }
  write_group(acc, m, false, j0, a.J, a.part);
}

// ---- boundary / initial amplitudes ----
// (one row per thread: nB is small against nT and the launch, not the bytes, is what the step pays -- DESIGN.md section 27)
__global__ __launch_bounds__(TB) void vn_bicgrad_kernel(VnBicGradArgs a) {
  const int j0 = blockIdx.y * JG;
  const unsigned m = group_mask(a, j0);
  const long rows = a.steady ? a.bDof : a.nB;
  float acc[JG] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m)
    for (long k = (long)blockIdx.x * TB + threadIdx.x; k < rows; k += (long)gridDim.x * TB) {
      const float w = vn_bic_value_seed(k, a.ub[k] - a.label[k], rows, a.bDof, a.biDimVal, a.w0, a.w1);
#pragma unroll
      for (int c = 0; c < JG; ++c)
        if (m >> c & 1u) acc[c] += w * a.B[(long)(j0 + c) * a.nB + k];
    }
  write_group(acc, m, true, j0, a.J, a.part);
}

// ---- flux-row amplitudes ----
// (one row per thread, as above: nF is small against nT.)  The part of stream j0 + c decides its row weight; a group of eight may
// carry streams of both parts, so both weights are formed per row and the choice is a uniform select per stream.
__global__ __launch_bounds__(TB) void vn_fbcgrad_kernel(VnFbcGradArgs a) {
  const int j0 = blockIdx.y * JG;
  const unsigned m = group_mask(a, j0);
  const int nl = a.Jl - j0;                                      // streams of this group that belong to the flux datum (may be <= 0, >= 8)
  float acc[JG] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m)
    for (long k = (long)blockIdx.x * TB + threadIdx.x; k < a.nF; k += (long)gridDim.x * TB) {
      const float s = a.udbar[k];
      const float wl = -s, wc = s * a.u[k];
#pragma unroll
      for (int c = 0; c < JG; ++c)
        if (m >> c & 1u) acc[c] += (c < nl ? wl : wc) * a.S[(long)(j0 + c) * a.nF + k];
    }
  write_group(acc, m, false, j0, a.J, a.part);
}

// ---- fold, Adam step, clamp ----
// TB / LANES groups of LANES lanes: lane j < J of group g adds the partials of the blocks [g chunk, (g + 1) chunk) in index order,
// then thread j adds the group sums in group order.  (16 lanes for the nine coefficients, 64 for the amplitudes: the order each
// gradient has had since its vector was added, and its bits depend on it.)  The same holds for the second-moment update: while
// each vector had its own kernel the compiler contracted b2 v + (1 - b2) g g into fma(b2, v, ((1 - b2) g) g) for the coefficients
// and into fma((1 - b2) g, g, b2 v) for the amplitudes, which round differently; both are written out here, so neither vector's
// trajectory moves.  (One form for all is a change of behaviour, to be made on purpose.)
// Prior.  With weight > 0 the quadratic prior Q(a) = 1/2 weight d^T R d, d = a - mean, adds weight (R d)_j
// in fp64 to the folded gradient of the masked entries, inside the fold (blocks > 0) only, so an apply after a gradient evaluation
// does not add it twice.  d is staged in shared memory before the barrier: no thread reads a value another has stepped.  Thread j
// walks column j of R, i ascending -- by symmetry row j, and a wave reads consecutive doubles.  With l1 the step ends in the
// proximal shrinkage c <- sign(c) max(|c| - lr_t l1[j], 0), fp32, after Adam's move and before the clamp; an entry with l1[j] == 0
// keeps the arithmetic it had.  pen != nullptr: evaluate only -- no fold, no update; pen[0] = Q and pen[1] = sum_j l1[j] |a_j|,
// each summed in index order by thread 0 from per-entry fp64 products.
template <int LANES>
__global__ __launch_bounds__(TB) void vn_learnt_apply_kernel(VnLearntApplyArgs a) {
  constexpr int GROUPS = TB / LANES;
  __shared__ double sub[GROUPS][LANES];
  __shared__ double dsh[VN_SRC_JMAX], qsh[VN_SRC_JMAX], lsh[VN_SRC_JMAX];
  const int j = threadIdx.x % LANES, g = threadIdx.x / LANES;
  const bool in = (int)threadIdx.x < a.J;                      // (J <= LANES: these are the threads of group 0, and j == threadIdx.x)
  const bool quad = a.weight > 0.0;
  if (a.blocks > 0 && !a.pen) {
    const int chunk = (a.blocks + GROUPS - 1) / GROUPS;
    const int b1 = (g + 1) * chunk < a.blocks ? (g + 1) * chunk : a.blocks;
    double t = 0.0;
    if (j < a.J)
      for (int b = g * chunk; b < b1; ++b) t += (double)a.part[(long)b * a.J + j];
    sub[g][j] = t;
  }
  if (quad && in) dsh[j] = (double)a.val[j] - a.mean[j];
  __syncthreads();
  double rd = 0.0;                                             // (R d)_j
  if (quad && in && (a.pen || a.blocks > 0)) {
    if (a.R)
      for (int i = 0; i < a.J; ++i) rd += a.R[(long)i * a.J + j] * dsh[i];
    else
      rd = dsh[j];
  }
  if (a.pen) {                                                 // (uniform: every thread takes the branch, and its barrier)
    if (in) {
      qsh[j] = quad ? dsh[j] * rd : 0.0;
      lsh[j] = a.l1 ? (double)a.l1[j] * fabs((double)a.val[j]) : 0.0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double q = 0.0, l = 0.0;
      for (int i = 0; i < a.J; ++i) { q += qsh[i]; l += lsh[i]; }
      a.pen[0] = 0.5 * a.weight * q;
      a.pen[1] = l;
    }
    return;
  }
  if (!in) return;                                             // (no barrier below)
  const bool on = a.mask >> j & 1ull;
  double gr = a.grad[j];
  if (a.blocks > 0) {
    gr = 0.0;
    for (int k = 0; k < GROUPS; ++k) gr += sub[k][j];
    if (quad) gr += a.weight * rd;
    if (!on) gr = 0.0;
    a.grad[j] = gr;
  }
  if (a.update && on) {                                        // same arithmetic as vn_adam_kernel, then the shrinkage and the clamp
    const float gi = (float)gr;
    const float mi = fmaf(1.f - a.b1, gi, a.b1 * a.m[j]);
    const float vi = LANES == 16 ? fmaf(a.b2, a.v[j], (1.f - a.b2) * gi * gi) : fmaf((1.f - a.b2) * gi, gi, a.b2 * a.v[j]);
    a.m[j] = mi;
    a.v[j] = vi;
    float c = a.val[j] - a.lr_t * mi / (sqrtf(vi) + a.eps);
    const float lam = a.l1 ? a.l1[j] : 0.f;
    if (lam > 0.f) c = copysignf(fmaxf(fabsf(c) - __fmul_rn(a.lr_t, lam), 0.f), c);
    a.val[j] = fminf(fmaxf(c, a.lo[j]), a.hi[j]);
  }
}

}  // namespace

// ---- launches: the 4-row kernels by the rule of vn_rows4.h, else the 1-row kernels ----
// (the streams of a basis are n floats apart, so its base decides for all of them)
hipError_t vn_learnt_mix_launch(const VnMixArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const bool four = rows4_ok(a.n, {a.base, a.stream, a.out});
  const long n = four ? a.n / 4 : a.n;
  hipLaunchKernelGGL(four ? vn_learnt_mix4_kernel : vn_learnt_mix_kernel, dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_coefgrad_rows_launch(const VnCoefRowsArgs& a, int* blocks, hipStream_t s) {
  const bool four = rows4_ok(a.nT, {a.u, a.udbar, a.rate, a.phi, a.A});
  *blocks = learnt_blocks(four ? a.nT / 4 : a.nT);
  hipLaunchKernelGGL(four ? vn_coefgrad_rows4_kernel : vn_coefgrad_rows_kernel, dim3((unsigned)*blocks), dim3(TB), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_coefgrad_points_launch(const VnCoefPointsArgs& a, int* blocks, hipStream_t s) {
  *blocks = learnt_blocks(a.U);
  hipLaunchKernelGGL(vn_coefgrad_points_kernel, dim3((unsigned)*blocks), dim3(TB), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_srcgrad_rows_launch(const VnSrcGradArgs& a, int* blocks, hipStream_t s) {
  const bool four = a.nT > 0 && rows4_ok(a.nT, {a.udbar, a.Nrow, a.phi});
  *blocks = learnt_blocks(four ? a.nT / 4 : a.nT);
  const dim3 grid((unsigned)*blocks, (unsigned)((a.J + JG - 1) / JG));
  hipLaunchKernelGGL(four ? vn_srcgrad_rows4_kernel : vn_srcgrad_rows_kernel, grid, dim3(TB), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_fldgrad_rows_launch(const VnFldGradArgs& a, int* blocks, hipStream_t s) {
  if (a.dim < 1 || a.dim > 3 || a.J < 1 || a.J > VN_FLD_JMAX) return hipErrorInvalidValue;
  *blocks = learnt_blocks(a.nT);
  const dim3 grid((unsigned)*blocks, (unsigned)((a.J + JG - 1) / JG));
  switch (a.dim) {
    case 1: hipLaunchKernelGGL(vn_fldgrad_rows_kernel<1>, grid, dim3(TB), 0, s, a); break;
    case 2: hipLaunchKernelGGL(vn_fldgrad_rows_kernel<2>, grid, dim3(TB), 0, s, a); break;
    default: hipLaunchKernelGGL(vn_fldgrad_rows_kernel<3>, grid, dim3(TB), 0, s, a); break;
  }
  return hipGetLastError();
}

hipError_t vn_bicgrad_launch(const VnBicGradArgs& a, int* blocks, hipStream_t s) {
  if (a.J < 1 || a.J > VN_BIC_JMAX || a.bDof < 0 || a.bDof > a.nB) return hipErrorInvalidValue;
  *blocks = learnt_blocks(a.steady ? a.bDof : a.nB);
  const dim3 grid((unsigned)*blocks, (unsigned)((a.J + JG - 1) / JG));
  hipLaunchKernelGGL(vn_bicgrad_kernel, grid, dim3(TB), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_fbcgrad_launch(const VnFbcGradArgs& a, int* blocks, hipStream_t s) {
  if (a.J < 1 || a.J > VN_FBC_JMAX || a.Jl < 0 || a.Jl > a.J || a.nF < 1) return hipErrorInvalidValue;
  *blocks = learnt_blocks(a.nF);
  const dim3 grid((unsigned)*blocks, (unsigned)((a.J + JG - 1) / JG));
  hipLaunchKernelGGL(vn_fbcgrad_kernel, grid, dim3(TB), 0, s, a);
  return hipGetLastError();
}

hipError_t vn_learnt_apply_launch(const VnLearntApplyArgs& a, hipStream_t s) {
  if (a.lanes != 16 && a.lanes != 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(a.lanes == 16 ? vn_learnt_apply_kernel<16> : vn_learnt_apply_kernel<64>, dim3(1), dim3(TB), 0, s, a);
  return hipGetLastError();
}
