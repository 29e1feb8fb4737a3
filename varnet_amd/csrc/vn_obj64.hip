// vn_objective_f64: the weak-form training objective of a batch -- interior rows, BC/IC rows, boundary-flux rows, periodic pairs, observed points, exactly what
// vn_grad / vn_eval_loss define -- and its gradient, with every operation after the exact widening of the registered fp32 arrays
// in double precision and every product of a layer on the fp64 matrix pipe (v_mfma_f64_16x16x4_f64).  A checking path in the
// plain style of vn_taylor16d.hip (see its header for the instruction's row interleave: register i of lane group g holds row
// 4i + g, so the accumulator row of a feature is the feature index and a layer's output registers are the next layer's B operand).
//
//   pack     theta [P] -> zero-padded weight images in global memory, [in-feature][64] per layer.  The images are NOT staged in
//            LDS: six layers of 64 need 166 KB as doubles, more than a workgroup has, and a checking path wants one code path for
//            its whole range (1..6 hidden layers, width <= 64, ragged widths) -- so every wave reads its A operands through
//            L1 / L2 (the images are <= 170 KB, shared by all waves), coalesced along the output feature.
//   forward  a wave carries 16 rows (one chunk) through the layers: value stream, plus one tangent stream along the row's gcoef
//            (interior rows), outward normal (flux rows) or pair direction (periodic rows); BC/IC rows carry none.  Writes u and the directional derivative.
//   seed     one thread per test function / BC-IC row / flux row / periodic pair (integ_num need not divide a tile): R_k, lossVec, the loss
//            partials per block, and -- with a gradient wanted -- the two adjoint seeds of every row, in place of (u, ud).
//   reverse  recomputes the chunk's forward pass, keeping each layer's (a, a') in a per-wave scratch in [feature][point] order,
//            sweeps both adjoints back on the matrix pipe (A operand = the same images read transposed), and contracts the
//            weight gradients over the chunk's 16 points on the matrix pipe: the transposed operands are the per-wave scratch
//            (activations, global) and an LDS copy of (zbar, zbar') read with the other index order.  Accumulators are the
//            wave's own gradient image in global memory (read-modify-write by the lane that owns the element: no atomics);
//            bias / output-weight gradients are kept per (feature, point slot) and summed over the 16 slots by the reduction.
//   reduce   folds the waves' images in wave order, the loss partials lane-strided plus a fixed shuffle tree.
// Every order is fixed by the sizes alone, so two calls return the same bits.
#include "vn_obj64.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int OW = 4;            // waves per workgroup
constexpr int OT = 64 * OW;
constexpr int CW = 16;           // rows per chunk
constexpr int IS = 64;           // image row stride
constexpr int LAYER = 2048;      // a wave's scratch per layer: a [16][64] | a' [16][64]

// offsets in doubles; W(l) is shared by the weight image and the gradient image
__host__ __device__ constexpr int img_w(int l) { return l == 1 ? 0 : 8 * IS + (l - 2) * 64 * IS; }
__host__ __device__ constexpr int img_tail(int L) { return 8 * IS + (L - 1) * 64 * IS; }
struct WImg {   // weights
  __host__ __device__ static constexpr int bi(int L) { return img_tail(L); }              // [L][64]
  __host__ __device__ static constexpr int wo(int L) { return bi(L) + L * 64; }           // [64]
  __host__ __device__ static constexpr int bo(int L) { return wo(L) + 64; }
  __host__ __device__ static constexpr int total(int L) { return bo(L) + 8; }
};
struct GImg {   // gradient accumulators of one wave
  __host__ __device__ static constexpr int gb(int L) { return img_tail(L); }              // [L][16][64] per (k-step, lane)
  __host__ __device__ static constexpr int gwo(int L) { return gb(L) + L * 1024; }        // [16][64]
  __host__ __device__ static constexpr int gbo(int L) { return gwo(L) + 1024; }           // [64]
  __host__ __device__ static constexpr int total(int L) { return gbo(L) + 64; }
};

struct Seg {
  const float* X;      // [n, d_in]
  const float* G;      // [n, dim] tangent direction, or nullptr: value stream only
  long n, off;         // rows; offset of row 0 in u / ud
};

struct ObjArgs {
  VnNet net;
  const double* img;
  Seg seg[5];          // interior, BC/IC, flux, periodic pairs (side A rows, then side B rows), observed points
  double* u; double* ud;
  double* act; double* part;
};

template <bool TANH>
__device__ __forceinline__ double actd(double z) { return TANH ? tanh(z) : 1.0 / (1.0 + exp(-z)); }
template <bool TANH>
__device__ __forceinline__ double actd_d1(double a) { return TANH ? 1.0 - a * a : a * (1.0 - a); }
template <bool TANH>
__device__ __forceinline__ double actd_d2r(double a) { return TANH ? -2.0 * a : 1.0 - 2.0 * a; }      // sigma'' / sigma'

__device__ __forceinline__ f64x4 mfma16d(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ double rowsum4d(double x) {       // over the four 16-lane rows of the wave, in every lane
  x += __shfl_xor(x, 16, 64);
  x += __shfl_xor(x, 32, 64);
  return x;
}
__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

__global__ __launch_bounds__(256) void vn_obj64_pack_kernel(VnNet net, const double* __restrict__ theta, double* __restrict__ img) {
  const int L = net.L;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= WImg::total(L)) return;
  double v = 0.0;
  if (idx < 8 * IS) {
    const int k = idx / IS, f = idx % IS;
    if (k < net.d_in && f < net.H[1]) v = theta[net.woff[1] + k * net.H[1] + f];
  } else if (idx < img_tail(L)) {
    const int j = idx - 8 * IS, l = j / (64 * IS) + 2, r = j % (64 * IS), k = r / IS, f = r % IS;
    if (k < net.H[l - 1] && f < net.H[l]) v = theta[net.woff[l] + k * net.H[l] + f];
  } else if (idx < WImg::wo(L)) {
    const int j = idx - WImg::bi(L), l = j / 64 + 1, f = j % 64;
    if (f < net.H[l]) v = theta[net.boff[l] + f];
  } else if (idx < WImg::bo(L)) {
    const int f = idx - WImg::wo(L);
    if (f < net.H[L]) v = theta[net.woff[L + 1] + f];
  } else if (idx == WImg::bo(L)) {
    v = theta[net.boff[L + 1]];
  }
  img[idx] = v;
}

template <bool TANH, bool REV>
__global__ __launch_bounds__(OT) void vn_obj64_kernel(ObjArgs A) {
  __shared__ double zs_all[REV ? OW * LAYER : 1];
  const VnNet& net = A.net;
  const int L = net.L;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const long wg = (long)blockIdx.x * OW + wave, nwaves = (long)gridDim.x * OW;
  const double* img = A.img;
  const double* BI = img + WImg::bi(L);
  const double* WO = img + WImg::wo(L);
  const double bo = img[WImg::bo(L)];
  double* act = REV ? A.act + wg * ((long)L * LAYER) : nullptr;
  double* part = REV ? A.part + wg * (long)GImg::total(L) : nullptr;
  double* zs = zs_all + (REV ? wave * LAYER : 0);
  const long c0 = (A.seg[0].n + CW - 1) / CW, c1 = c0 + (A.seg[1].n + CW - 1) / CW, c2 = c1 + (A.seg[2].n + CW - 1) / CW;
  const long c3 = c2 + (A.seg[3].n + CW - 1) / CW, c4 = c3 + (A.seg[4].n + CW - 1) / CW;
  const int d_in = net.d_in, dim = net.dim;

  for (long chunk = wg; chunk < c4; chunk += nwaves) {
    const int si = chunk < c0 ? 0 : chunk < c1 ? 1 : chunk < c2 ? 2 : chunk < c3 ? 3 : 4;
    const float* X = si == 0 ? A.seg[0].X : si == 1 ? A.seg[1].X : si == 2 ? A.seg[2].X : si == 3 ? A.seg[3].X : A.seg[4].X;
    const float* G = si == 0 ? A.seg[0].G : si == 1 ? A.seg[1].G : si == 2 ? A.seg[2].G : si == 3 ? A.seg[3].G : A.seg[4].G;
    const long n = si == 0 ? A.seg[0].n : si == 1 ? A.seg[1].n : si == 2 ? A.seg[2].n : si == 3 ? A.seg[3].n : A.seg[4].n;
    const long off = si == 0 ? A.seg[0].off : si == 1 ? A.seg[1].off : si == 2 ? A.seg[2].off : si == 3 ? A.seg[3].off : A.seg[4].off;
    const long base = (chunk - (si == 0 ? 0 : si == 1 ? c0 : si == 2 ? c1 : si == 3 ? c2 : c3)) * CW;
    const long row = base + c;
    const bool valid = row < n;
    const bool tangent = G != nullptr;                     // wave-uniform
    double xin[2], gin[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int f = 4 * s + g;
      xin[s] = (valid && f < d_in) ? (double)X[row * d_in + f] : 0.0;
      gin[s] = (valid && tangent && f < dim) ? (double)G[row * dim + f] : 0.0;
    }
    // ---- forward
    f64x4 pv[4], pt[4];
    {
      const double* W1 = img + img_w(1);
      const int H1 = net.H[1];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        pv[m] = f64x4{BI[m * 16 + g], BI[m * 16 + 4 + g], BI[m * 16 + 8 + g], BI[m * 16 + 12 + g]};
        pt[m] = f64x4{0.0, 0.0, 0.0, 0.0};
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (4 * s < d_in) {
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            if (16 * m < H1) {
              const double wf = W1[(4 * s + g) * IS + c + 16 * m];
              pv[m] = mfma16d(wf, xin[s], pv[m]);
              if (tangent) pt[m] = mfma16d(wf, gin[s], pt[m]);
            }
          }
        }
      }
    }
    double a[16], ad[16];
#pragma unroll 1
    for (int l = 1; l <= L; ++l) {
      const int Hl = net.H[l];
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        a[ks] = 0.0; ad[ks] = 0.0;
        if (4 * ks < Hl) {
          const double z = pv[ks >> 2][ks & 3], zd = pt[ks >> 2][ks & 3];
          a[ks] = actd<TANH>(z);
          ad[ks] = actd_d1<TANH>(a[ks]) * zd;
          if (REV) {
            act[(l - 1) * LAYER + ks * 64 + lane] = a[ks];
            act[(l - 1) * LAYER + 1024 + ks * 64 + lane] = ad[ks];
          }
        }
      }
      if (l == L) break;
      const double* Wl = img + img_w(l + 1);
      const double* bl = BI + l * 64;
      const int Hout = net.H[l + 1];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        pv[m] = f64x4{bl[m * 16 + g], bl[m * 16 + 4 + g], bl[m * 16 + 8 + g], bl[m * 16 + 12 + g]};
        pt[m] = f64x4{0.0, 0.0, 0.0, 0.0};
      }
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        if (4 * ks < Hl) {
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            if (16 * m < Hout) {
              const double wf = Wl[(4 * ks + g) * IS + c + 16 * m];
              pv[m] = mfma16d(wf, a[ks], pv[m]);
              if (tangent) pt[m] = mfma16d(wf, ad[ks], pt[m]);
            }
          }
        }
      }
    }
    if (!REV) {
      double u = 0.0, ud = 0.0;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        const double wv = WO[4 * ks + g];
        u += wv * a[ks];
        ud += wv * ad[ks];
      }
      u = rowsum4d(u) + bo;
      ud = rowsum4d(ud);
      if (valid && g == 0) {
        A.u[off + row] = u;
        A.ud[off + row] = ud;
      }
      continue;
    }
    // ---- reverse (REV only)
    if (REV) {
      wave_fence();                                        // the scratch of this chunk is read back with another lane order
      const double ubar = valid ? A.u[off + row] : 0.0;
      const double udbar = (valid && tangent) ? A.ud[off + row] : 0.0;
      double ab[16], adb[16];
      {
        double* gwo = part + GImg::gwo(L);
        const int HL = net.H[L];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          if (4 * ks < HL) gwo[ks * 64 + lane] += a[ks] * ubar + ad[ks] * udbar;
          const double wv = WO[4 * ks + g];
          ab[ks] = wv * ubar;
          adb[ks] = wv * udbar;
        }
        if (g == 0) part[GImg::gbo(L) + c] += ubar;
      }
#pragma unroll 1
      for (int l = L; l >= 1; --l) {
        const int Hout = net.H[l], Hin = net.H[l - 1];
        double zb[16], zdb[16];
        double* gb = part + GImg::gb(L) + (l - 1) * 1024;
        wave_fence();                                      // the previous layer's reads of zs are done
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          zb[ks] = 0.0; zdb[ks] = 0.0;
          if (4 * ks < Hout) {
            double al = a[ks], adl = ad[ks];
            if (l < L) {
              al = act[(l - 1) * LAYER + ks * 64 + lane];
              adl = act[(l - 1) * LAYER + 1024 + ks * 64 + lane];
            }
            const double s1 = actd_d1<TANH>(al);
            zb[ks] = s1 * ab[ks] + actd_d2r<TANH>(al) * adl * adb[ks];
            zdb[ks] = s1 * adb[ks];
            gb[ks * 64 + lane] += zb[ks];
          }
          zs[ks * 64 + lane] = zb[ks];
          zs[1024 + ks * 64 + lane] = zdb[ks];
        }
        wave_fence();
        // weight gradient: gW[i][o] += sum over the chunk's points of a_{l-1}[i] zbar[o] + a'_{l-1}[i] zbar'[o]
        double* gw = part + img_w(l);
        const double* prev = act + (l - 2) * LAYER;        // (l == 1: the input rows instead)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          if (l == 1 ? mi == 0 : 16 * mi < Hin) {
            double aT[4], adT[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
              if (l > 1) {
                const int idx = (c + 16 * mi) * 16 + 4 * kk + g;
                aT[kk] = prev[idx];
                adT[kk] = prev[1024 + idx];
              } else {
                const long r2 = base + 4 * kk + g;
                const bool v2 = r2 < n;
                aT[kk] = (v2 && c < d_in) ? (double)X[r2 * d_in + c] : 0.0;
                adT[kk] = (v2 && tangent && c < dim) ? (double)G[r2 * dim + c] : 0.0;
              }
            }
#pragma unroll
            for (int mo = 0; mo < 4; ++mo) {
              if (16 * mo < Hout) {
                f64x4 C;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                  C[r] = (l > 1 || r < 2) ? gw[(16 * mi + 4 * r + g) * IS + 16 * mo + c] : 0.0;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                  const int idx = (c + 16 * mo) * 16 + 4 * kk + g;
                  C = mfma16d(aT[kk], zs[idx], C);
                  if (tangent) C = mfma16d(adT[kk], zs[1024 + idx], C);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
                  if (l > 1 || r < 2) gw[(16 * mi + 4 * r + g) * IS + 16 * mo + c] = C[r];
              }
            }
          }
        }
        if (l == 1) break;
        // adjoints of layer l - 1: (abar, abar') = W_l (zbar, zbar'), the image read transposed
        const double* Wl = img + img_w(l);
        f64x4 nab[4], nadb[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          nab[m] = f64x4{0.0, 0.0, 0.0, 0.0};
          nadb[m] = f64x4{0.0, 0.0, 0.0, 0.0};
        }
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          if (4 * ks < Hout) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              if (16 * m < Hin) {
                const double wf = Wl[(c + 16 * m) * IS + 4 * ks + g];
                nab[m] = mfma16d(wf, zb[ks], nab[m]);
                if (tangent) nadb[m] = mfma16d(wf, zdb[ks], nadb[m]);
              }
            }
          }
        }
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          ab[ks] = nab[ks >> 2][ks & 3];
          adb[ks] = nadb[ks >> 2][ks & 3];
        }
      }
      wave_fence();                                        // ... before the next chunk's forward overwrites the scratch
    }
  }
}

// ---- weak-form epilogue in double: the arithmetic of vn_seed_kernel / vn_flux_seed_kernel (vn_generic.hip) ----------------
struct SeedArgs {
  double* u; double* ud;                      // interior rows at 0, BC/IC rows at offB, flux rows at offF, periodic rows at offP, observed points at offO
  long offB, offF, offP, offO;
  const float* source; const float* feN; const float* fedNt; const float* feW;
  const float* Nrow; const float* dNtrow; const float* detJv; double detJ;
  long n_k; int q; int td;
  const float* label; long nB, bDof; double biDimVal;
  const float* fcoef; const float* flabel; long nF; double fbiDimVal;
  long nP; double pgamma, pbiDimVal; double* ppart;   // periodic pairs (i, i + nP); ppart [gridDim.x]
  // observations: segment k = points [orowptr[k], orowptr[k+1]) (nullptr: point k); oq, owgt nullptr: 1; odir: ud is live
  const float* oq; const int* orowptr; const float* ovalue; const float* owgt; long nO; int odir; double olambda; double* opart;
  double w0, w1, w2;
  int seeds;                                  // write the adjoint seeds in place of (u, ud)
  int react; const float* rate; double c1, c2, c3;   // reaction rate p(u), p = c1 u + c2 u^2 + c3 u^3 (react == 0: none)
  int nlflux; const float* phi; double f1, f2, f3;   // flux term -F(u) phi, F = f1 u + f2 u^2 + f3 u^3 (nlflux == 0: none)
  int nldiff; const float* psi; double d0, d1, d2;   // D(u) ud - u psi for ud, D = d0 + d1 u + d2 u^2 (nldiff == 0: none; psi may be nullptr)
  double* lossVec; double* lpart;             // [n_k] or nullptr; [gridDim.x][4]
};

__device__ __forceinline__ double block_sum_d(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void vn_obj64_seed_kernel(SeedArgs a) {
  __shared__ double red[4];
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  double lv = 0.0, bc = 0.0, ic = 0.0, fl = 0.0, pe = 0.0, oe = 0.0;
  if (k < a.n_k) {
    const int q = a.q;
    const long base = k * q;
    double R = 0.0;
    for (int p = 0; p < q; ++p) {
      const long r = base + p;
      double t = a.ud[r];
      if (a.nldiff) {                               // quasilinear diffusion: the tangent part scaled by D(u), advection as -u psi
        const double uu = a.u[r];
        t *= a.d0 + uu * (a.d1 + uu * a.d2);
        if (a.psi) t -= uu * (double)a.psi[r];
      }
      if (a.td) t -= a.u[r] * (double)(a.dNtrow ? a.dNtrow[r] : a.fedNt[p]);
      if (a.react) {
        const double uu = a.u[r];
        const double pu = uu * (a.c1 + uu * (a.c2 + uu * a.c3));
        const double se = (a.source ? (double)a.source[r] : 0.0) + (a.rate ? (double)a.rate[r] * pu : pu);
        t -= se * (double)(a.Nrow ? a.Nrow[r] : a.feN[p]);
      } else if (a.source) t -= (double)a.source[r] * (double)(a.Nrow ? a.Nrow[r] : a.feN[p]);
      if (a.nlflux) {
        const double uu = a.u[r];
        t -= uu * (a.f1 + uu * (a.f2 + uu * a.f3)) * (double)a.phi[r];
      }
      if (a.feW) t *= (double)a.feW[p];
      R += t;
    }
    const double dj = a.detJv ? (double)a.detJv[k] : a.detJ;
    lv = dj * R * R;
    if (a.lossVec) a.lossVec[k] = lv;
    if (a.seeds) {
      const double s0 = 2.0 * a.w2 * dj * R;
      for (int p = 0; p < q; ++p) {
        const long r = base + p;
        const double s = a.feW ? s0 * (double)a.feW[p] : s0;
        const double A = a.ud[r];                   // the forward's directional derivative, before the seed takes its place
        a.ud[r] = s;
        double ub = a.td ? -(double)(a.dNtrow ? a.dNtrow[r] : a.fedNt[p]) * s : 0.0;
        if (a.react) {                              // u[r] still holds the forward value here
          const double uu = a.u[r];
          const double dp = a.c1 + uu * (2.0 * a.c2 + 3.0 * a.c3 * uu);
          ub -= (double)(a.Nrow ? a.Nrow[r] : a.feN[p]) * (a.rate ? (double)a.rate[r] * dp : dp) * s;
        }
        if (a.nlflux) {                             // d t / d u of the flux term: -phi F'(u)
          const double uu = a.u[r];
          ub -= (double)a.phi[r] * (a.f1 + uu * (2.0 * a.f2 + 3.0 * a.f3 * uu)) * s;
        }
        if (a.nldiff) {                             // d t / d u = D'(u) A - psi; the tangent seed scaled by D(u)
          const double uu = a.u[r];
          ub += ((a.d1 + 2.0 * a.d2 * uu) * A - (a.psi ? (double)a.psi[r] : 0.0)) * s;
          a.ud[r] = (a.d0 + uu * (a.d1 + uu * a.d2)) * s;
        }
        a.u[r] = ub;
      }
    }
  }
  if (k < a.nB) {
    const double e = a.u[a.offB + k] - (double)a.label[k];
    const double e2 = a.biDimVal * e * e;
    const bool isbc = k < a.bDof;
    if (isbc) bc = e2; else ic = e2;
    if (a.seeds) {
      const long nI = a.nB - a.bDof;
      const double cb = 2.0 * a.w0 * a.biDimVal / (double)a.bDof;
      const double ci = nI > 0 ? 2.0 * a.w1 * a.biDimVal / (double)nI : 0.0;
      a.u[a.offB + k] = (isbc ? cb : ci) * e;
    }
  }
  if (k < a.nF) {
    const double cf = (double)a.fcoef[k];
    const double r = a.ud[a.offF + k] + cf * a.u[a.offF + k] - (double)a.flabel[k];
    fl = a.fbiDimVal * r * r;
    if (a.seeds) {
      const double s = 2.0 * a.w0 * a.fbiDimVal / (double)a.nF;
      a.ud[a.offF + k] = s * r;
      a.u[a.offF + k] = s * cf * r;
    }
  }
  if (k < a.nP) {                                 // the arithmetic of vn_periodic_seed_kernel (vn_edge.hip)
    const long i = a.offP + k, j = i + a.nP;
    const double r0 = a.u[i] - a.u[j];
    const double r1 = a.pgamma > 0.0 ? a.ud[i] - a.ud[j] : 0.0;
    pe = a.pbiDimVal * (r0 * r0 + a.pgamma * r1 * r1);
    if (a.seeds) {
      const double s = 2.0 * a.w0 * a.pbiDimVal / (double)a.nP;
      a.u[i] = s * r0; a.u[j] = -s * r0;
      a.ud[i] = s * a.pgamma * r1; a.ud[j] = -s * a.pgamma * r1;
    }
  }
  if (k < a.nO) {                                 // the arithmetic of vn_obs_seed_kernel (vn_edge.hip), additions in CSR order
    const long e0 = a.orowptr ? (long)a.orowptr[k] : k, e1 = a.orowptr ? (long)a.orowptr[k + 1] : k + 1;
    double acc = 0.0;
    for (long e = e0; e < e1; ++e) {
      double t = a.oq ? (double)a.oq[e] * a.u[a.offO + e] : a.u[a.offO + e];
      if (a.odir) t += a.ud[a.offO + e];
      acc += t;
    }
    const double wk = a.owgt ? (double)a.owgt[k] : 1.0;
    const double r = acc - (double)a.ovalue[k];
    oe = wk * r * r;
    if (a.seeds) {
      const double s = 2.0 * a.olambda * wk * r / (double)a.nO;
      for (long e = e0; e < e1; ++e) {
        a.u[a.offO + e] = a.oq ? s * (double)a.oq[e] : s;
        if (a.odir) a.ud[a.offO + e] = s;
      }
    }
  }
  const double s0 = block_sum_d(lv, red);
  const double s1 = block_sum_d(bc, red);
  const double s2 = block_sum_d(ic, red);
  const double s3 = block_sum_d(fl, red);
  if (threadIdx.x == 0) {
    double* o = a.lpart + (long)blockIdx.x * 4;
    o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
  }
  if (a.nP > 0) {                                 // (block-uniform)
    const double s4 = block_sum_d(pe, red);
    if (threadIdx.x == 0) a.ppart[blockIdx.x] = s4;
  }
  if (a.nO > 0) {                                 // (block-uniform)
    const double s5 = block_sum_d(oe, red);
    if (threadIdx.x == 0) a.opart[blockIdx.x] = s5;
  }
}

// loss scalars: one wave, lane-strided over the seed blocks, then a fixed shuffle tree
__global__ __launch_bounds__(64) void vn_obj64_loss_kernel(const double* __restrict__ lpart, int nblk, long bDof, long nB, long nF,
                                                          const double* __restrict__ ppart, long nP, const double* __restrict__ opart, long nO,
                                                          double olambda, double* __restrict__ omisfit, double w0, double w1, double w2,
                                                          double* __restrict__ out) {
  const int lane = threadIdx.x;
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = lane; b < nblk; b += 64)
    for (int j = 0; j < 4; ++j) t[j] += lpart[(long)b * 4 + j];
  for (int o = 32; o > 0; o >>= 1)
    for (int j = 0; j < 4; ++j) t[j] += __shfl_down(t[j], o, 64);
  double tp = 0.0;                                // periodic pairs: the same fold over their own partials
  if (nP > 0) {
    for (int b = lane; b < nblk; b += 64) tp += ppart[b];
    for (int o = 32; o > 0; o >>= 1) tp += __shfl_down(tp, o, 64);
  }
  double to = 0.0;                                // observations: the same fold over their own partials
  if (nO > 0) {
    for (int b = lane; b < nblk; b += 64) to += opart[b];
    for (int o = 32; o > 0; o >>= 1) to += __shfl_down(to, o, 64);
  }
  if (lane == 0) {
    const double var = t[0];
    double bc = bDof > 0 ? t[1] / (double)bDof : 0.0;
    if (nF > 0) bc += t[3] / (double)nF;
    if (nP > 0) bc += tp / (double)nP;
    const double ic = (nB - bDof) > 0 ? t[2] / (double)(nB - bDof) : 0.0;
    double loss = w0 * bc + w1 * ic + w2 * var;
    if (nO > 0) {
      const double O = to / (double)nO;
      loss += olambda * O;
      *omisfit = O;
    }
    out[0] = loss;
    out[1] = bc; out[2] = ic; out[3] = var;
  }
}

// grad[p] = the waves' images folded in wave order (bias and output-layer entries: the 16 point slots first)
__global__ __launch_bounds__(256) void vn_obj64_reduce_kernel(VnNet net, const double* __restrict__ part, long nw,
                                                            double* __restrict__ grad) {
  const int L = net.L;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= net.P) return;
  int idx = 0, nc = 1;
  for (int l = 1; l <= L + 1; ++l) {
    if (p < net.woff[l]) continue;
    if (p < net.boff[l]) {
      const int j = p - net.woff[l];
      if (l <= L) {
        const int i = j / net.H[l], o = j % net.H[l];
        idx = img_w(l) + i * IS + o; nc = 1;
      } else {
        idx = GImg::gwo(L) + (j >> 2) * 64 + (j & 3) * 16; nc = 16;
      }
    } else if (p < net.boff[l] + net.H[l]) {
      const int f = p - net.boff[l];
      if (l <= L) idx = GImg::gb(L) + (l - 1) * 1024 + (f >> 2) * 64 + (f & 3) * 16;
      else idx = GImg::gbo(L);
      nc = 16;
    }
  }
  const long GT = GImg::total(L);
  double acc = 0.0;
  for (long w = 0; w < nw; ++w) {
    const double* src = part + w * GT + idx;
    double t = src[0];
    for (int cc = 1; cc < nc; ++cc) t += src[cc];
    acc += t;
  }
  grad[p] = acc;
}

hipError_t ensure_d(double** p, long* cap, long need) {
  if (need <= *cap) return hipSuccess;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  hipError_t e = hipMalloc((void**)p, (size_t)need * sizeof(double));
  if (e == hipSuccess) *cap = need;
  return e;
}

#define OCHK(expr)                       \
  do {                                   \
    hipError_t e_ = (expr);              \
    if (e_ != hipSuccess) return e_;     \
  } while (0)

}  // namespace

bool vn_obj64_supported(const VnNet& net) { return vn_net_in_kernel_range(net) && net.dim <= 3; }

void vn_obj64_free(VnObj64Work& w) {
  double** ps[] = {&w.img, &w.u, &w.ud, &w.act, &w.part, &w.lpart, &w.out, &w.lvec, &w.omega, &w.wstat, &w.bwpart};
  for (double** p : ps) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  w.img_cap = w.u_cap = w.ud_cap = w.act_cap = w.part_cap = w.lpart_cap = w.lvec_cap = w.omega_cap = w.wstat_cap = w.bwpart_cap = 0;
}

hipError_t vn_obj64_run(VnObj64Work& w, const VnObj64Problem& p, double* grad_dev, double* lossVec_dev, double out_host[4],
                        int ncu, hipStream_t s) {
  if (!vn_obj64_supported(p.net)) return hipErrorInvalidValue;
  const VnNet& net = p.net;
  const int L = net.L;
  const long n0 = p.n_k * p.q, nB = p.nB, nF = p.nF, nP = p.nP, nP2 = 2 * p.nP, nO = p.nO, on = nO > 0 ? p.on : 0;
  const long rows = n0 + nB + nF + nP2 + on;
  const long chunks = (n0 + CW - 1) / CW + (nB + CW - 1) / CW + (nF + CW - 1) / CW + (nP2 + CW - 1) / CW + (on + CW - 1) / CW;
  OCHK(ensure_d(&w.img, &w.img_cap, WImg::total(L)));
  OCHK(ensure_d(&w.u, &w.u_cap, rows > 0 ? rows : 1));
  OCHK(ensure_d(&w.ud, &w.ud_cap, rows > 0 ? rows : 1));
  if (!w.out) OCHK(hipMalloc((void**)&w.out, 4 * sizeof(double)));
  long most = p.n_k > nB ? (p.n_k > nF ? p.n_k : nF) : (nB > nF ? nB : nF);
  if (nP > most) most = nP;
  if (nO > most) most = nO;
  const int sblk = (int)(((most > 0 ? most : 1) + 255) / 256);
  OCHK(ensure_d(&w.lpart, &w.lpart_cap, (long)sblk * (4 + (nP > 0 ? 1 : 0) + (nO > 0 ? 1 : 0))));

  hipLaunchKernelGGL(vn_obj64_pack_kernel, dim3((WImg::total(L) + 255) / 256), dim3(256), 0, s, net, p.theta, w.img);
  OCHK(hipGetLastError());

  ObjArgs a{};
  a.net = net; a.img = w.img; a.u = w.u; a.ud = w.ud;
  a.seg[0] = Seg{p.X, p.G, n0, 0};
  a.seg[1] = Seg{p.Xb, nullptr, nB, n0};
  a.seg[2] = Seg{p.Xf, p.Nf, nF, n0 + nB};
  a.seg[3] = Seg{p.Xp, p.pgamma > 0.0 ? p.Dp : nullptr, nP2, n0 + nB + nF};
  a.seg[4] = Seg{p.Xo, p.Do, on, n0 + nB + nF + nP2};
  const bool tanh_ = net.act == VN_ACT_TANH;
  const long wgs = (chunks + OW - 1) / OW;
  if (chunks > 0) {
    const int grid = (int)(wgs < 2L * ncu ? wgs : 2L * ncu);
    if (tanh_) hipLaunchKernelGGL((vn_obj64_kernel<true, false>), dim3(grid), dim3(OT), 0, s, a);
    else hipLaunchKernelGGL((vn_obj64_kernel<false, false>), dim3(grid), dim3(OT), 0, s, a);
    OCHK(hipGetLastError());
  }
  SeedArgs sa{};
  sa.u = w.u; sa.ud = w.ud; sa.offB = n0; sa.offF = n0 + nB;
  sa.source = p.src; sa.feN = p.feN; sa.fedNt = p.fedNt; sa.feW = p.feW;
  sa.Nrow = p.Nrow; sa.dNtrow = p.dNtrow; sa.detJv = p.detJv; sa.detJ = p.detJ;
  sa.n_k = p.n_k; sa.q = p.q; sa.td = p.td;
  sa.label = p.label; sa.nB = nB; sa.bDof = p.bDof; sa.biDimVal = p.biDimVal;
  sa.fcoef = p.fcoef; sa.flabel = p.flabel; sa.nF = nF; sa.fbiDimVal = p.fbiDimVal;
  sa.offP = n0 + nB + nF; sa.nP = nP; sa.pgamma = p.pgamma; sa.pbiDimVal = p.pbiDimVal; sa.ppart = w.lpart + (long)sblk * 4;
  sa.offO = n0 + nB + nF + nP2; sa.nO = nO; sa.oq = p.Qo; sa.orowptr = p.orowptr; sa.ovalue = p.ovalue; sa.owgt = p.owgt;
  sa.odir = p.Do ? 1 : 0; sa.olambda = p.olambda; sa.opart = w.lpart + (long)sblk * (nP > 0 ? 5 : 4);
  sa.w0 = p.w[0]; sa.w1 = p.w[1]; sa.w2 = p.w[2];
  sa.seeds = grad_dev ? 1 : 0;
  sa.react = p.react; sa.rate = p.rate; sa.c1 = p.coef[0]; sa.c2 = p.coef[1]; sa.c3 = p.coef[2];
  sa.nlflux = p.nlflux; sa.phi = p.phi; sa.f1 = p.fcoef3[0]; sa.f2 = p.fcoef3[1]; sa.f3 = p.fcoef3[2];
  sa.nldiff = p.nldiff; sa.psi = p.psi; sa.d0 = p.dcoef3[0]; sa.d1 = p.dcoef3[1]; sa.d2 = p.dcoef3[2];
  sa.lossVec = lossVec_dev; sa.lpart = w.lpart;
  const bool weighted = vn_weights_on(p.wt) && p.n_k > 0;
  if (weighted) {
    // the same objective as the fp32 steps (vn_weights.hip): the weights in double from this evaluation's own loss field
    if (!sa.lossVec) { OCHK(ensure_d(&w.lvec, &w.lvec_cap, p.n_k)); sa.lossVec = w.lvec; }
    OCHK(ensure_d(&w.omega, &w.omega_cap, p.n_k));
    if (p.wt.S > 0) OCHK(ensure_d(&w.wstat, &w.wstat_cap, (long)p.wt.S * (p.wt.chunks + 1)));
  }
  // weights on the BC/IC rows (vn_bicadapt.hip): the weighted partial sums from the forward values before the seed kernel puts
  // the seeds in their place, then those partials in place of the unweighted ones and the rows' seeds scaled
  VnBicRows64Args bw;
  const bool bweighted = (p.bic_omega[0] || p.bic_omega[1]) && nB > 0;
  if (bweighted) {
    OCHK(ensure_d(&w.bwpart, &w.bwpart_cap, 2L * vn_bic_rows_blocks(nB)));
    bw.u = w.u + n0; bw.label = p.label; bw.nB = nB; bw.bDof = p.bDof; bw.biDimVal = p.biDimVal;
    bw.omega[0] = p.bic_omega[0]; bw.omega[1] = p.bic_omega[1]; bw.wpart = w.bwpart; bw.lpart = w.lpart; bw.seeds = sa.seeds;
    OCHK(vn_bic_rows_f64_launch(bw, 0, s));
  }
  hipLaunchKernelGGL(vn_obj64_seed_kernel, dim3(sblk), dim3(256), 0, s, sa);
  OCHK(hipGetLastError());
  if (bweighted) OCHK(vn_bic_rows_f64_launch(bw, 1, s));
  if (weighted) {
    VnWeightsWork wk;
    wk.lsum = w.wstat; wk.oslab = w.wstat ? w.wstat + (long)p.wt.S * p.wt.chunks : nullptr;
    OCHK(vn_weights_apply_f64(p.wt, wk, sa.lossVec, p.n_k, w.omega, w.lpart, s));    // var partials weighted, lossVec as it is
    if (grad_dev) OCHK(vn_weights_rows_f64(w.omega, p.n_k, p.q, w.u, w.ud, s));       // the interior seeds in u / ud scaled
  }
  hipLaunchKernelGGL(vn_obj64_loss_kernel, dim3(1), dim3(64), 0, s, w.lpart, sblk, p.bDof, nB, nF, sa.ppart, nP, sa.opart, nO, p.olambda, p.omisfit,
                     p.w[0], p.w[1], p.w[2], w.out);
  OCHK(hipGetLastError());

  if (grad_dev) {
    const int grid = (int)(wgs < 1 ? 1 : wgs < ncu ? wgs : ncu);
    const long nw = (long)grid * OW;
    OCHK(ensure_d(&w.act, &w.act_cap, nw * L * LAYER));
    OCHK(ensure_d(&w.part, &w.part_cap, nw * GImg::total(L)));
    OCHK(hipMemsetAsync(w.part, 0, (size_t)(nw * GImg::total(L)) * sizeof(double), s));
    a.act = w.act; a.part = w.part;
    if (chunks > 0) {
      if (tanh_) hipLaunchKernelGGL((vn_obj64_kernel<true, true>), dim3(grid), dim3(OT), 0, s, a);
      else hipLaunchKernelGGL((vn_obj64_kernel<false, true>), dim3(grid), dim3(OT), 0, s, a);
      OCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(vn_obj64_reduce_kernel, dim3((net.P + 255) / 256), dim3(256), 0, s, net, w.part, nw, grad_dev);
    OCHK(hipGetLastError());
  }
  OCHK(hipMemcpyAsync(out_host, w.out, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  return hipStreamSynchronize(s);
}
