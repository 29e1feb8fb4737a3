// Value and input gradient of the network at a set of points in ONE pass: value forward, then the value-adjoint
// sweep back to the inputs with seed 1 -- the reference's own tf.gradients(model(Input), Input) (TFModel.py:536-541):
// 2 F_pt per point whatever the number of coordinates, where one forward-tangent pass per coordinate costs dim * 2 F_pt.
// Serves the de-duplicated formulation (vn_dedup.hip), which needs (u, du/dx_d) once per unique quadrature point
// before the weak-form assembly over rows, vn_forward_grad, and -- without the adjoint sweep (out_g == nullptr) -- vn_forward:
// the value alone at F_pt per point (the fused kernel's forward-only mode carries a tangent stream of zeros through every
// layer for such calls: twice the matrix work).
//
// Same geometry and data layout as vn_fused16.hip (8 waves, 16 points per wave, v_mfma_f32_16x16x4_f32, feature f in
// k-step f/4 / lane group f%4, layers chained in registers, weight images [in-feature][out-position] with row stride 65
// in LDS: forward fragments and the transposed fragments of the sweep come from the one copy), with ONE stream per
// direction instead of two, no weight gradient, hence no transposition images, no workgroup barrier after the prologue:
// every wave walks its own 16-point chunks.  The activations of all layers stay in registers between the two sweeps
// (KS * L values per lane: 65 at 5x50).
#include "vn_points16.h"
#include "vn_pgrad16.h"

namespace {
using namespace vn16;

struct VnPgradArgsD {
  VnNet net;
  const float* theta;
  const float* X;            // [n, d_in]
  long n;
  float* out_u;              // [n]
  float* out_g;              // [n, dim]: du/dx_d, d < dim (the leading coordinates of X)
  float* out_pack;           // [n, 4] = (u, du/dx_0, du/dx_1, du/dx_2) or nullptr
};

template <int L, int KS, bool TANH>
__global__ __launch_bounds__(NTHREADS, 2) VN_NO_LDS_PAIRING void vn_pgrad16_kernel(VnPgradArgsD A) {
  using LY = PLay<L, KS>;
  using GE = Geo<KS>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const VnNet& net = A.net;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* W1 = lds + LY::W1_OFF;
  float* WH = lds + LY::WH_OFF;
  float* BI = lds + LY::BI_OFF;
  float* WO = lds + LY::WO_OFF;
  const float bo = A.theta[net.boff[L + 1]];
  stage_weight_images<L, KS>(net, A.theta, lds, tid);      // vn_points16.h
  __syncthreads();

  const int g = lane >> 4, c = lane & 15;
  const int offF = g * WS + c;                       // forward A fragment: in-feature 4ks+g, out-position 16m+c
  static_assert(16 * GE::MTM <= LY::HP, "backward fragment rows stay inside the weight image");
  const int offB0 = vfeat(c) * WS + 4 * g;           // transposed A fragment of row tile 0: in-feature vfeat(c), out-position vpos(ks, g)

  const long nchunks = (A.n + CW - 1) / CW;
  for (long chunk = (long)blockIdx.x * NW + wave; chunk < nchunks; chunk += (long)gridDim.x * NW) {
    asm volatile("" ::: "memory");                   // keep LDS fragment loads inside the loop
    const long row = chunk * CW + c;
    const bool valid = row < A.n;
    float xin[KS0];
#pragma unroll
    for (int s = 0; s < KS0; ++s) {
      const int f = 4 * s + g;
      xin[s] = (valid && f < net.d_in) ? A.X[row * net.d_in + f] : 0.f;
    }

    PA<KS> a[L];
    // ---------------------------------------------------------------- value forward
    f32x4 pv[GE::MT];
#pragma unroll
    for (int m = 0; m < GE::MT; ++m) pv[m] = *reinterpret_cast<const f32x4a*>(&BI[m * 16 + g * 4]);
#pragma unroll
    for (int s = 0; s < KS0; ++s) {
      if (4 * s < net.d_in) {
#pragma unroll
        for (int m = 0; m < GE::MT; ++m) pv[m] = mfma16(W1[4 * s * WS + offF + 16 * m], xin[s], pv[m]);
      }
    }
#pragma unroll
    for (int l = 2; l <= L; ++l) {
      const float* Wl = WH + (l - 2) * LY::HPWS;
      int k_in = (net.H[l - 1] + 3) >> 2, m_out = (net.H[l] + 15) >> 4;
      f32x4 nv[GE::MT];
#pragma unroll
      for (int m = 0; m < GE::MT; ++m) nv[m] = *reinterpret_cast<const f32x4a*>(&BI[(l - 1) * 64 + m * 16 + g * 4]);
      // activation of the previous layer pipelined under this layer's MFMAs in pairs of k-steps: stage A (packed scale + 2 v_exp)
      // of pair j+3 after the first k-step of pair j, stage B (packed 1+e + 2 v_rcp) of pair j+2 after the second
      constexpr int NP = PA<KS>::NP;
      auto zin2 = [&](int j) { return f32x2{pv[(2 * j) >> 2][(2 * j) & 3], pv[(2 * j) >> 2][((2 * j) & 3) + 1]}; };
      float wf[GE::MTM > 0 ? GE::MTM : 1], we[GE::NVE], ev[GE::NVE];
#pragma unroll
      for (int m = 0; m < GE::MTM; ++m) wf[m] = Wl[offF + 16 * m];
#pragma unroll
      for (int v = 0; v < GE::NVE; ++v) {
        we[v] = GE::EDGE ? Wl[offF - c + GE::EPOS + 4 * v] : 0.f;
        ev[v] = 0.f;
      }
      f32x2 cs2 = act_fin2<TANH>(act_exp2<TANH>(zin2(0)));
      a[l - 2].p[0] = cs2;
      f32x2 s1 = (NP > 1) ? act_fin2<TANH>(act_exp2<TANH>(zin2(1))) : f32x2{0.f, 0.f};
      f32x2 e2 = (NP > 2) ? act_exp2<TANH>(zin2(2)) : f32x2{0.f, 0.f};
      f32x2 e3 = {0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int j = ks >> 1;
        float wn[GE::MTM > 0 ? GE::MTM : 1], wen[GE::NVE];
#pragma unroll
        for (int m = 0; m < GE::MTM; ++m) wn[m] = (ks + 1 < KS) ? Wl[4 * (ks + 1) * WS + offF + 16 * m] : 0.f;
#pragma unroll
        for (int v = 0; v < GE::NVE; ++v) wen[v] = (GE::EDGE && ks + 1 < KS) ? Wl[4 * (ks + 1) * WS + offF - c + GE::EPOS + 4 * v] : 0.f;
        const float cs = cs2[ks & 1];
        __builtin_amdgcn_sched_barrier(0);
        if (GE::live_k(ks, k_in)) {
#pragma unroll
          for (int m = 0; m < GE::MTM; ++m) {
            if (!GE::live_m(m, m_out)) continue;
            nv[m] = mfma16(wf[m], cs, nv[m]);
          }
        }
        if (GE::EDGE) {
#pragma unroll
          for (int v = 0; v < GE::NVE; ++v) ev[v] += we[v] * cs;
        }
        if ((ks & 1) == 0) {
          if (j + 3 < NP) e3 = act_exp2<TANH>(zin2(j + 3));
          __builtin_amdgcn_sched_barrier(0);
        } else {
          f32x2 s2 = s1;
          if (j + 2 < NP) s2 = act_fin2<TANH>(e2);
          if (j + 1 < NP) a[l - 2].p[j + 1] = s1;
          __builtin_amdgcn_sched_barrier(0);
          cs2 = s1; s1 = s2; e2 = e3;
        }
#pragma unroll
        for (int m = 0; m < GE::MTM; ++m) wf[m] = wn[m];
#pragma unroll
        for (int v = 0; v < GE::NVE; ++v) we[v] = wen[v];
      }
      if (GE::EDGE) nv[GE::MT - 1][0] += edge_reduce_scatter<GE::NVE>(ev, g);       // bias was loaded above
#pragma unroll
      for (int m = 0; m < GE::MT; ++m) pv[m] = nv[m];
    }
    auto pairOf = [](const f32x4 (&t)[GE::MT], int j) { return f32x2{t[(2 * j) >> 2][(2 * j) & 3], t[(2 * j) >> 2][((2 * j) & 3) + 1]}; };
#pragma unroll
    for (int j = 0; j < PA<KS>::NP; ++j) a[L - 1].p[j] = act_fin2<TANH>(act_exp2<TANH>(pairOf(pv, j)));

    // ---------------------------------------------------------------- output layer and its adjoint (seed 1)
    PA<KS> zb;
    float u = 0.f;
    {
      f32x2 u2 = {0.f, 0.f};
#pragma unroll
      for (int j = 0; j < PA<KS>::NP; ++j) {
        const bool full = 2 * j + 1 < KS;
        const f32x2 wv = {WO[4 * (2 * j) + g], full ? WO[4 * (2 * j + 1) + g] : 0.f};
        const f32x2 av = a[L - 1].p[j];
        u2 += wv * av;
        zb.p[j] = wv * act_d1_2<TANH>(av);             // d u / d z_L
      }
      u = rowsum4(u2[0] + u2[1]) + bo;
    }
    if (A.out_g == nullptr && A.out_pack == nullptr) {   // value only (vn_forward): F_pt per point, no adjoint sweep
      if (valid && g == 3 && A.out_u) A.out_u[row] = u;
      continue;
    }

    // ---------------------------------------------------------------- value-adjoint sweep to the inputs
#pragma unroll
    for (int l = L; l >= 2; --l) {
      const float* Wl = WH + (l - 2) * LY::HPWS;
      int k_out = (net.H[l] + 3) >> 2, m_in = (net.H[l - 1] + 15) >> 4;
      f32x4 accv[GE::MT];
#pragma unroll
      for (int m = 0; m < GE::MT; ++m) accv[m] = f32x4{0.f, 0.f, 0.f, 0.f};
      float wf[GE::MTM > 0 ? GE::MTM : 1], we[GE::NVE], ev[GE::NVE];
#pragma unroll
      for (int m = 0; m < GE::MTM; ++m) wf[m] = Wl[offB0 + 16 * m * WS + vpos(0, 0)];
#pragma unroll
      for (int v = 0; v < GE::NVE; ++v) {
        we[v] = GE::EDGE ? Wl[(4 * (KS - 1) + v) * WS + 4 * g + vpos(0, 0)] : 0.f;
        ev[v] = 0.f;
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        float wn[GE::MTM > 0 ? GE::MTM : 1], wen[GE::NVE];
#pragma unroll
        for (int m = 0; m < GE::MTM; ++m) wn[m] = (ks + 1 < KS) ? Wl[offB0 + 16 * m * WS + vpos(ks + 1, 0)] : 0.f;
#pragma unroll
        for (int v = 0; v < GE::NVE; ++v) wen[v] = (GE::EDGE && ks + 1 < KS) ? Wl[(4 * (KS - 1) + v) * WS + 4 * g + vpos(ks + 1, 0)] : 0.f;
        __builtin_amdgcn_sched_barrier(0);
        if (GE::live_k(ks, k_out)) {
#pragma unroll
          for (int m = 0; m < GE::MTM; ++m) {
            if (!GE::live_m(m, m_in)) continue;
            accv[m] = mfma16(wf[m], zb[ks], accv[m]);
          }
        }
        if (GE::EDGE) {
#pragma unroll
          for (int v = 0; v < GE::NVE; ++v) ev[v] += we[v] * zb[ks];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < GE::MTM; ++m) wf[m] = wn[m];
#pragma unroll
        for (int v = 0; v < GE::NVE; ++v) we[v] = wen[v];
      }
      if (GE::EDGE) accv[GE::MT - 1][0] = edge_reduce_scatter<GE::NVE>(ev, g);
#pragma unroll
      for (int j = 0; j < PA<KS>::NP; ++j) {
        const int ks = 2 * j;
        if (ks + 1 < KS) {
          const f32x2 ab = {accv[ks >> 2][ks & 3], accv[ks >> 2][(ks & 3) + 1]};
          zb.p[j] = ab * act_d1_2<TANH>(a[l - 2].p[j]);
        } else {
          zb.set(ks, accv[ks >> 2][ks & 3] * act_d1<TANH>(a[l - 2][ks]));
        }
      }
    }
    // input layer: du/dx_d = sum_f W_1[d][f] zbar_1[f]; this lane holds feature 4ks+g of every k-step, the four lane
    // groups are summed by row swaps (same pairing in every lane: all agree bit for bit)
    float xg[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d < net.dim) {
        float t = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) t += W1[d * WS + vpos(ks, 0) + 4 * g] * zb[ks];
        xg[d] = rowsum4(t);
      }
    }
    if (valid) {
      const float mine = (g == 3) ? u : (g == 0) ? xg[0] : (g == 1) ? xg[1] : xg[2];       // xg of an absent coordinate is 0
      if (A.out_pack) A.out_pack[row * 4 + ((g + 1) & 3)] = mine;                          // (u, g0, g1, g2): lane group 3 holds u
      if (g == 3) { if (A.out_u) A.out_u[row] = u; }
      else if (g < net.dim && A.out_g) A.out_g[row * net.dim + g] = mine;
    }
  }
}

}  // namespace

hipError_t vn_pgrad16_launch(const VnNet& net, const float* theta, const float* X, long n, float* out_u, float* out_g,
                             float* out_pack, int ncu, int wgs_per_cu, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (((out_g || out_pack) && net.dim > 3) || net.d_in > 4 * KS0) return hipErrorInvalidValue;
  VnPgradArgsD a;
  a.net = net; a.theta = theta; a.X = X; a.n = n; a.out_u = out_u; a.out_g = out_g; a.out_pack = out_pack;
  // in the product library the networks the bf16-piece kernels do NOT serve (VN16_F32_POINT_CASES)
  return visit_f32_point(net, hipErrorInvalidValue, [&](auto I) {
    using T = decltype(I);
    return launch_chunks<vn_pgrad16_kernel<T::L, T::KS, T::TANH>, true>(a, n, (size_t)PLay<T::L, T::KS>::TOTAL * sizeof(float), ncu,
                                                                     wgs_per_cu, s);
  });
}
