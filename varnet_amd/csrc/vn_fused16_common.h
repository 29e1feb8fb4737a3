// Device helpers shared by the 8-wave kernels of the fused family (vn_fused16.hip: the training step;
// vn_pgrad16.hip: value + input gradient at points; vn_split16.hip: point kernels on the bf16 pipe): the feature <->
// (k-step, lane group, accumulator row) layout, activation arithmetic on register pairs, cross-lane sums, and the
// bf16-piece machinery of the hidden-layer products (exact three-way split, 1 KB-block weight images, fragment reads).
// Also what the five translation units of the family share beyond device helpers: the table of instantiations, the tile
// geometry of an instantiation (Geo), and -- host side, at the end -- the one dispatch walk and the one launcher.
#pragma once
#include "vn_internal.h"

#include <atomic>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef f32x4 f32x4a __attribute__((may_alias));

namespace vn16 {

constexpr int NW = 8;
constexpr int NTHREADS = 64 * NW;
constexpr int TILE = 128;
constexpr int CW = 16;        // points per wave
constexpr int WS = 65;        // weight image row stride
constexpr int KS0 = 2;        // input layer k-steps (d_in <= 8)

__host__ __device__ constexpr int al4(int x) { return (x + 3) & ~3; }
__host__ __device__ constexpr int vpos(int ks, int g) { return 16 * (ks >> 2) + 4 * g + (ks & 3); }
__host__ __device__ constexpr int vks(int pos) { return 4 * (pos >> 4) + (pos & 3); }
__host__ __device__ constexpr int vfeat(int pos) { return 4 * vks(pos) + ((pos >> 2) & 3); }

// What the branches over padding-only k-steps / row tiles (KSKIP, live_k / live_m) rely on: k-step ks holds features 4ks..4ks+3 and
// nothing else, row tile m (positions 16m..16m+15) holds features 16m..16m+15 and nothing else -- so "width H" bounds the live
// k-steps by ceil(H/4) and the live row tiles by ceil(H/16).  A change of vpos / vfeat that breaks this must not compile.
__host__ __device__ constexpr bool layout_ties_ksteps_and_tiles_to_features() {
  for (int ks = 0; ks < 16; ++ks)
    for (int g = 0; g < 4; ++g)
      if (vks(vpos(ks, g)) != ks || vfeat(vpos(ks, g)) != 4 * ks + g) return false;
  for (int pos = 0; pos < 64; ++pos)
    if (vfeat(pos) < 16 * (pos >> 4) || vfeat(pos) >= 16 * (pos >> 4) + 16 || vpos(vks(pos), (pos >> 2) & 3) != pos) return false;
  return true;
}
static_assert(layout_ties_ksteps_and_tiles_to_features(), "KSKIP: k-step = feature >> 2, row tile = feature >> 4");
__host__ __device__ constexpr int mtiles(int KS) { return (KS + 3) / 4; }

// ---- the instantiations of the family: (hidden layers L, k-steps per hidden layer KS) ---------------------------------------
// KS = 5 | 8 | 13 | 16 serves hidden widths up to 20 | 32 | 50 | 64 (vn_fused16_ks).  Every pair is written ONCE, under the list
// it belongs to, so the two lists are disjoint by construction and adding an instantiation is a one-line change here:
//   S  the bf16-piece networks -- hidden widths 33..64 (KS = 13, 16) with 2..7 hidden layers, 6 beyond 50 wide (L = 1 has no
//      hidden product; 8 x 24 KB of images do not fit): their point kernels are those of vn_split16.hip; the f32-MFMA forms
//      (vn_pgrad16 / vn_taylor16) are what the tests compare them with and are instantiated in the tests' cross-check library
//      only (-DVN_XCHECK_F32_POINT, Makefile target xcheck);
//   F  the rest: vn_pgrad16 / vn_taylor16 serve them in the product library.
// The fused step kernel (vn_fused16.hip) is instantiated for the union, and vn_fused16_net_supported -- hence the engine's
// route -- accepts exactly the union; vn_taylor16d.hip walks the union and keeps the pairs whose double images fit the LDS.
// The two lists share one table, KS-major, because the compiler emits kernels into a code object in the order of the walk.
#define VN16_TABLE(F, S) \
  F(1, 5)  F(2, 5)  F(3, 5)  F(4, 5)  F(5, 5)  F(6, 5)  F(7, 5)  F(8, 5)   \
  F(1, 8)  F(2, 8)  F(3, 8)  F(4, 8)  F(5, 8)  F(6, 8)  F(7, 8)  F(8, 8)   \
  F(1, 13) S(2, 13) S(3, 13) S(4, 13) S(5, 13) S(6, 13) S(7, 13) F(8, 13)  \
  F(1, 16) S(2, 16) S(3, 16) S(4, 16) S(5, 16) S(6, 16)
#define VN16_NOT_LISTED(L, KS)
#define VN16_SPLIT_CASES(X) VN16_TABLE(VN16_NOT_LISTED, X)
#define VN16_F32_ONLY_CASES(X) VN16_TABLE(X, VN16_NOT_LISTED)
#define VN16_CASES(X) VN16_TABLE(X, X)
#ifdef VN_XCHECK_F32_POINT
#define VN16_F32_POINT_CASES(X) VN16_F32_ONLY_CASES(X) VN16_SPLIT_CASES(X)
#else
#define VN16_F32_POINT_CASES(X) VN16_F32_ONLY_CASES(X)
#endif

// The machine-level load/store optimizer pairs LDS reads into ds_read2_b32, whose 8-bit offsets force a
// VALU address add per pair; vector instructions share the datapath with the f32 MFMAs here, LDS issue
// does not, so pairing is switched off for the f32-MFMA kernels (device pass only; -0.8 % kernel time).
#if defined(__HIP_DEVICE_COMPILE__)
#define VN_NO_LDS_PAIRING __attribute__((target("no-load-store-opt")))
#else
#define VN_NO_LDS_PAIRING
#endif

// Tile geometry of the f32-MFMA kernels (vn_fused16, vn_pgrad16, vn_taylor16) at KS k-steps per hidden layer.
template <int KS>
struct Geo {
  static constexpr int MT = mtiles(KS);
  // EDGE: the last 16-row tile holds a single k-step (features 4(KS-1) .. 4(KS-1)+3, e.g. 48,49 of a
  // 50-wide layer).  Producing those few rows with an MFMA tile costs a quarter of the matrix work of
  // the layer; instead every lane accumulates its share of their dot products on the VALU (which runs
  // under the partner wave's MFMAs) and the four lane groups are summed with two shuffles.
  static constexpr bool EDGE = (KS % 4) == 1 && KS > 1;
  static constexpr int MTM = EDGE ? MT - 1 : MT;            // row tiles produced by MFMA in hidden layers
  static constexpr int NVE = (KS == 13) ? 2 : 4;            // edge features that can be non-padding
  static constexpr int EPOS = 16 * (MT - 1);                // accumulator row of edge feature 0
  // KSKIP: nets up to 32 wide are padded to 4*KS features in EVERY layer; a small net's tile is bound by the matrix pipe like
  // any other (removing MFMAs scales the step: profiles/r3_small_sensitivity.txt), so the k-steps and row tiles that hold
  // only padding (zero weights: they add +0) are branched over, wave-uniformly, on the layer's real widths -- the [10,20,30]
  // net of Operator_1DtMOR.py:189 needs 3 and 5 of its 8 forward k-steps, and one of two row tiles in its last input gradient.
  static constexpr bool KSKIP = KS <= 8;
  // (the bound is made opaque at every use: left to itself the compiler hoists the loop-invariant compares out of the tile
  // loop as 64-bit lane masks, a pair of scalar registers per guard, and spills them through v_writelane)
  static __device__ __forceinline__ bool live_k(int ks, int& kn) {
    if (!KSKIP || ks == 0) return true;
    asm volatile("" : "+s"(kn));
    return ks < kn;
  }
  static __device__ __forceinline__ bool live_m(int m, int& mn) {
    if (!KSKIP || m == 0) return true;
    asm volatile("" : "+s"(mn));
    return m < mn;
  }
};

__device__ __forceinline__ float opaque(float x) {
  asm("" : "+v"(x));
  return x;
}

// Activation (uniform over the hidden layers): sigmoid, or tanh = 2*sigmoid(2z) - 1 (VarNet.py:97).  Everything the
// kernel needs is a function of the stored activation a:  sigma' = a(1-a) | 1-a^2,  sigma''/sigma' = 1-2a | -2a.
template <bool TANH>
__device__ __forceinline__ float act_exp(float z) {      // the exponential inside the sigmoid
  return __builtin_amdgcn_exp2f((TANH ? -2.8853900817779268f : -1.4426950408889634f) * z);
}
template <bool TANH>
__device__ __forceinline__ float act_fin(float e) {      // e = exp(-z) | exp(-2z)  ->  activation
  const float s = __builtin_amdgcn_rcpf(1.0f + e);
  return TANH ? __builtin_fmaf(2.f, s, -1.f) : s;
}
template <bool TANH>
__device__ __forceinline__ float act_d1(float a) { return TANH ? __builtin_fmaf(-a, a, 1.f) : a * (1.f - a); }
template <bool TANH>
__device__ __forceinline__ float act_d2r(float a) { return TANH ? -2.f * a : 1.f - 2.f * a; }

typedef float f32x2 __attribute__((ext_vector_type(2)));

// Per-lane value arrays indexed by k-step, kept as even-aligned REGISTER PAIRS: k-steps 2j and 2j+1 share a pair, so
// the elementwise chains of the reverse pass run as v_pk_mul_f32 / v_pk_fma_f32 on two k-steps per instruction
// (packed fp32 issues at the scalar rate on gfx950, and every vector instruction costs matrix time here).  A pair of
// accumulator rows (ks, ks+1), ks even, of an MFMA tile is a register pair already.
template <int N>
struct PA {
  static constexpr int NP = (N + 1) / 2;
  f32x2 p[NP];
  __device__ __forceinline__ float operator[](int i) const { return p[i >> 1][i & 1]; }
  __device__ __forceinline__ void set(int i, float v) { p[i >> 1][i & 1] = v; }
};
__device__ __forceinline__ f32x2 opaque2(f32x2 x) {
  asm("" : "+v"(x));
  return x;
}
template <bool TANH>
__device__ __forceinline__ f32x2 act_exp2(f32x2 z) {      // two exponentials: one packed scale, two v_exp
  const float c = TANH ? -2.8853900817779268f : -1.4426950408889634f;
  const f32x2 t = z * f32x2{c, c};
  return f32x2{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
}
template <bool TANH>
__device__ __forceinline__ f32x2 act_fin2(f32x2 e) {
  const f32x2 d = e + f32x2{1.f, 1.f};
  const f32x2 s = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
  return TANH ? (s * f32x2{2.f, 2.f} - f32x2{1.f, 1.f}) : s;
}
template <bool TANH>
__device__ __forceinline__ f32x2 act_d1_2(f32x2 a) {
  const f32x2 one = {1.f, 1.f};
  return TANH ? (one - a * a) : (a - a * a);
}
template <bool TANH>
__device__ __forceinline__ f32x2 act_d2r_2(f32x2 a) {
  const f32x2 one = {1.f, 1.f}, two = {2.f, 2.f};
  return TANH ? (-two * a) : (one - two * a);
}

// x summed over the four 16-lane rows of the wave, in every lane: (r0 + r1) + (r2 + r3)
__device__ __forceinline__ float rowsum4(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));     // a = [r0 r0 r2 r2], b = [r1 r1 r3 r3]
  const float s = a + b;
  float c = s, d = s;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(c), "+v"(d));     // c = [lo lo], d = [hi hi]
  return c + d;
}

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}

// x summed over the 16 lanes of its row, in every lane of the row (fixed order: quads, then 8, then 16)
__device__ __forceinline__ float rowsum16(float x) {
  x += dpp_f32<0xB1>(x);         // quad_perm [1,0,3,2]
  x += dpp_f32<0x4E>(x);         // quad_perm [2,3,0,1]
  x += dpp_f32<0x141>(x);        // row_half_mirror
  x += dpp_f32<0x140>(x);        // row_mirror
  return x;
}

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Edge rows: every lane group holds a partial sum (its share of the k index) of each of the NV edge features; group g
// must end up with the TOTAL of feature g.  A reduce-scatter instead of NV all-reduces: at each of the two exchange
// steps a lane sends only the partials its partner keeps, so NV = 2 takes 2 cross-lane moves instead of 4, NV = 4 takes
// 3 instead of 8 (ds_bpermute costs ~14 issue cycles on the shared vector path).  Groups >= NV get 0.
template <int NV>
__device__ __forceinline__ float edge_reduce_scatter(const float (&e)[NV], int g) {
  if constexpr (NV == 2) {
    // step 1 (partner g^1): keep feature g&1, hand the other one over
    const float keep = (g & 1) ? e[1] : e[0], give = (g & 1) ? e[0] : e[1];
    float t = keep + __shfl_xor(give, 16, 64);
    t += __shfl_xor(t, 32, 64);                       // step 2 (partner g^2): both hold the same feature
    return g < 2 ? t : 0.f;
  } else {
    static_assert(NV == 4, "edge features: 2 or 4");
    // step 1 (partner g^1): keep the two features with the parity of g
    const bool odd = (g & 1) != 0;
    const float k0 = odd ? e[1] : e[0], k1 = odd ? e[3] : e[2];
    const float g0 = odd ? e[0] : e[1], g1 = odd ? e[2] : e[3];
    const float a = k0 + __shfl_xor(g0, 16, 64);      // feature (g&1)
    const float b = k1 + __shfl_xor(g1, 16, 64);      // feature (g&1) + 2
    // step 2 (partner g^2): keep feature g
    const bool hi = (g & 2) != 0;
    return (hi ? b : a) + __shfl_xor(hi ? a : b, 32, 64);
  }
}

// ---- bf16-piece hidden-layer products (hidden widths 33..64: two K fragments of 32) ----------------------------------
// Every f32 operand is cut EXACTLY into three bf16 pieces x = h + m + l (3 x 8 significand bits, truncation), and a layer
// product is the six terms hh, hm, mh, hl, lh, mm with f32 accumulation, small terms first; the dropped terms (ml, lm, ll)
// are <= 3 * 2^-24 relative (profiles/r2_micro_split_bf16.md).
// Weight image of a hidden layer: 24 blocks [piece 3][q 2][row tile 4] of 1 KB = [g 4][c ^ 12(g&1)][8 bf16]: lane (g, c)
// reads the 8 in-features 4(8q+j)+g, j = 0..7, of out-position 16 mt + c with ONE conflict-free ds_read_b128.
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4a __attribute__((may_alias));

constexpr int BLK = 1024;                                  // bytes of one (piece, q, row tile) block
constexpr int IMG = 24 * BLK;                              // bytes of one hidden layer's image
// The fused step kernel's image (stage_split_hidden, FOLD13): 20 blocks per layer.  Neither of its sweeps reads row tile 3 of a
// piece-1 or piece-2 image (the folded tile lives in piece 0: three_folded, three_khalf), so those four blocks do not exist:
// piece 0 keeps its eight blocks [q][row tile 4], pieces 1 and 2 have six each, [q][row tile 3].  Block (piece, q, row tile) is
// at fblk * BLK; the transposed reads rely on row tiles 2q, 2q + 1 (q == 0) being neighbours in every piece.
constexpr int IMGF = 20 * BLK;
__host__ __device__ constexpr int fblk(int p, int q, int mt) { return p == 0 ? q * 4 + mt : 8 + ((p - 1) * 2 + q) * 3 + mt; }

__device__ __forceinline__ u32 fu(float x) { return __builtin_bit_cast(u32, x); }
__device__ __forceinline__ float uf(u32 x) { return __builtin_bit_cast(float, x); }
__device__ __forceinline__ u32 pack_hi(u32 u1, u32 u0) { return __builtin_amdgcn_perm(u1, u0, 0x07060302u); }   // (hi16(u1) << 16) | hi16(u0)

// exact three-way split of two f32 values into packed bf16 pairs (truncation: h = the top 8 significand bits, m the next 8 of
// the remainder, l the next 8).  Scalar subtracts: packed f32 instructions are expensive beside bf16 MFMAs (the study's raw table).
__device__ __forceinline__ void split2(float x0, float x1, u32& h, u32& m, u32& l) {
  const u32 u0 = fu(x0), u1 = fu(x1);
  h = pack_hi(u1, u0);
  const float r0 = x0 - uf(u0 & 0xffff0000u), r1 = x1 - uf(u1 & 0xffff0000u);
  const u32 v0 = fu(r0), v1 = fu(r1);
  m = pack_hi(v1, v0);
  const float s0 = r0 - uf(v0 & 0xffff0000u), s1 = r1 - uf(v1 & 0xffff0000u);
  l = pack_hi(fu(s1), fu(s0));
}

__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// the six products of one (row tile, K fragment), small terms first; the streams that share the weight fragment are interleaved
// product by product (independent accumulators: no MFMA waits for its predecessor's result)
template <int N>
__device__ __forceinline__ void six(const u32x4 (&A)[3], const u32x4 (*const (&B)[N])[3], f32x4* const (&acc)[N]) {
  constexpr int pa[6] = {1, 2, 0, 1, 0, 0}, pb[6] = {1, 0, 2, 0, 1, 0};
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int s = 0; s < N; ++s) *acc[s] = mfma_bf16(A[pa[i]], (*B[s])[pb[i]], *acc[s]);
  }
}

// The bf16-piece images of hidden layers 2..L at img (L - 1 consecutive IMG-byte images): one 16-byte entry (8 in-features of
// one out-position) per thread and layer, cut into its three pieces here; padding exact zeros.  Ends with the images written
// but not yet visible to other waves: the caller synchronises.
//
// FOLD13 (the fused step kernel at KS == 13, widths 33..50): the edge k-step 12 holds features 48, 49 only, so the fourth row
// tile of the forward sweep has two real rows (4g' + 0, g' = 0, 1) and the fourth row tile of the sweep back likewise.  Their
// idle neighbours carry the other two pieces of the same weights, in the PIECE-0 blocks:
//   out-fold: rows 4g' + 1 and 4g' + 2 of row tile 3 hold the m- and the l-pieces of out-feature 48 + g' -- one MFMA per B
//             piece leaves Ah.B, Am.B, Al.B in accumulator registers 0, 1, 2 (three MFMAs and one fragment instead of six
//             and three; all nine piece products instead of six);
//   in-fold:  slots j = 5, 6 of the q == 1 entries (k-steps 13, 14) hold the m- and the l-piece of slot 4 (in-feature 48 + g):
//             the transposed read of piece 0 hands the sweep back the same three rows.
//             Row tile 3 itself has no in-fold: its rows already are the three pieces.
// What makes this safe: k-steps 13..15 never hold a feature at KS == 13 (features >= 52), and so the bias image is zero there.
// First K fragment (q == 0, `six` / three_folded): no folded slot is touched.  Second K fragment (K halves, below): the B
// operands FEED slots 5, 6 (E_h, E_m), so every A fragment must hold there either the in-fold of its own slot 4 or an exact zero:
//   * row tiles 0..2: the in-fold (forward), the out-fold rows of the same out-feature (sweep back);
//   * row tile 3 (the corner, rows 4g' + 0, 1, 2 x slots 4, 5, 6): h, m, l in slot 4 and zeros in slots 5, 6 -- each weight
//     piece once; an in-fold on row 4g' + 0 would count mh, lh and mm of the corner twice;
//   * slot 7 (k-step 15) and row 4g' + 3 (features >= 60) are zero in every piece.
// The image has 20 blocks per layer (fblk): row tile 3 of the piece-1 and piece-2 images is read by neither sweep.  The q == 1
// entries of pieces 1, 2 carry in their edge half what the forward sweep's paired operands need ([A1 | A1], [A2 | 0]).
template <int L, bool FOLD13 = false>
__device__ __forceinline__ void stage_split_hidden(const VnNet& net, const float* theta, char* img, int tid) {
  static_assert(NTHREADS == 2 * 4 * 4 * 16, "one entry per thread and layer");
  const int q = tid >> 8, mt = (tid >> 6) & 3, g = (tid >> 4) & 3, c = tid & 15;
  const int pos = 16 * mt + c;
  const int fold_r = (FOLD13 && mt == 3) ? (c & 3) : 0;                      // 1 | 2: an out-fold row (m- | l-pieces)
  const bool ofold = fold_r == 1 || fold_r == 2;
  const int fo = ofold ? 48 + (c >> 2) : vfeat(pos);
  const int ent = (g * 16 + (c ^ (12 * (g & 1)))) * 16;
#pragma unroll
  for (int l = 2; l <= L; ++l) {
    const int Hin = net.H[l - 1], Hout = net.H[l];
    const float* src = theta + net.woff[l];
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int fi = 4 * (8 * q + j) + g;
      w[j] = (fi < Hin && fo < Hout) ? src[fi * Hout + fo] : 0.f;
    }
    u32x4 ph, pm, pl;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      u32 h, m, lo;
      split2(w[2 * jj], w[2 * jj + 1], h, m, lo);
      ph[jj] = h; pm[jj] = m; pl[jj] = lo;
    }
    if constexpr (FOLD13) {
      if (ofold) {             // slots 5..7 of q == 1 are in-features >= 52: zero in every piece, so the corners stay zero
        ph = fold_r == 1 ? pm : pl;
        pm = u32x4{0u, 0u, 0u, 0u};
        pl = u32x4{0u, 0u, 0u, 0u};
      } else if (q == 1 && mt != 3) {   // slot 4 = low half of word 2; slot 5 = its high half, slot 6 = low half of word 3 (both zero so far)
        // (not in row tile 3: the corner holds every weight piece once -- K halves below)
        ph[2] = (ph[2] & 0xffffu) | (pm[2] << 16);
        ph[3] = (ph[3] & 0xffff0000u) | (pl[2] & 0xffffu);
        // K halves: the edge half of the piece-1 and piece-2 entries is read by neither sweep (five_khalf; the sweep back reads
        // slots 4..7 of a q == 1 entry for its folded row tile only, from piece 0).  The forward sweep reads its operands
        // [A1 | A1] and [A2 | 0] as they stand: the piece-1 entry repeats its T half, the piece-2 entry ends in zeros.
        pm[2] = pm[0];
        pm[3] = pm[1];
        pl[2] = 0u;
        pl[3] = 0u;
      }
    }
    if constexpr (FOLD13) {
      char* il = img + (l - 2) * IMGF;
      *reinterpret_cast<u32x4a*>(il + fblk(0, q, mt) * BLK + ent) = ph;
      if (mt != 3) {
        *reinterpret_cast<u32x4a*>(il + fblk(1, q, mt) * BLK + ent) = pm;
        *reinterpret_cast<u32x4a*>(il + fblk(2, q, mt) * BLK + ent) = pl;
      }
      continue;
    }
    char* il = img + (l - 2) * IMG;
    *reinterpret_cast<u32x4a*>(il + ((0 * 2 + q) * 4 + mt) * BLK + ent) = ph;
    *reinterpret_cast<u32x4a*>(il + ((1 * 2 + q) * 4 + mt) * BLK + ent) = pm;
    *reinterpret_cast<u32x4a*>(il + ((2 * 2 + q) * 4 + mt) * BLK + ent) = pl;
  }
}

// Lane bases into the images.  Row read (forward: contraction over a layer's IN-features): lane (g, c) reads its entry of a
// block.  Transposed read (sweep back: contraction over the OUT-features 4(8q+j)+g, row tile over the IN-positions 16 mt + c):
// lane 4r + p of its group supplies row r (c_out = 4g + r), columns 4p..4p+3 (entry g_in = p) of a ds_read_b64_tr_b16.
__device__ __forceinline__ int split_row_base(int g, int c) { return (g * 16 + (c ^ (12 * (g & 1)))) * 16; }
__device__ __forceinline__ int split_tr_base(int g, int c) {
  const int tr_r = c >> 2, tr_p = c & 3;
  return (tr_p * 16 + ((4 * g + tr_r) ^ (12 * (tr_p & 1)))) * 16;
}
// A fragment (three pieces) of row tile mt, K fragment q, from a layer's image at rl = image + split_row_base
__device__ __forceinline__ u32x4 split_frag_row1(const char* rl, int p, int q, int mt) {
  return *reinterpret_cast<const u32x4a*>(rl + ((p * 2 + q) * 4 + mt) * BLK);
}
__device__ __forceinline__ void split_frag_row(const char* rl, int q, int mt, u32x4 (&Af)[3]) {
#pragma unroll
  for (int p = 0; p < 3; ++p) Af[p] = split_frag_row1(rl, p, q, mt);
}
// Transposed A fragment of in-position row tile mt, out-feature K fragment q, from tl = image + split_tr_base: in the forward
// image those are element 4(mt&1) + (c&3) of the entries (g_in = (c>>2)&3, c_out = 4g + (j&3)) of blocks (q_in = mt>>1,
// mt_out = 2q + (j>>2)): two transposed reads per piece (EXEC must be all ones).
__device__ __forceinline__ u32x4 split_frag_tr1(const char* tl, int p, int q, int mt) {
  const char* b0 = tl + ((p * 2 + (mt >> 1)) * 4 + 2 * q) * BLK + 8 * (mt & 1);
  const s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(b0));
  const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(b0 + BLK));
  const unsigned long long l64 = __builtin_bit_cast(unsigned long long, lo4), h64 = __builtin_bit_cast(unsigned long long, hi4);
  return u32x4{(u32)l64, (u32)(l64 >> 32), (u32)h64, (u32)(h64 >> 32)};
}
__device__ __forceinline__ void split_frag_tr(const char* tl, int q, int mt, u32x4 (&At)[3]) {
#pragma unroll
  for (int p = 0; p < 3; ++p) At[p] = split_frag_tr1(tl, p, q, mt);
}

// The folded edge tile (stage_split_hidden, FOLD13): ONE fragment -- piece 0, whose rows / slots 0, 1, 2 of every group of four
// hold the h-, m- and l-pieces of the same weights -- against the B pieces l, m, h (small terms first), one MFMA each and stream.
// Registers 0, 1, 2 of the accumulators then hold Ah.B, Am.B, Al.B: fold_rows adds them up once the K fragments are through.
template <int N>
__device__ __forceinline__ void three_folded(const u32x4& A0, const u32x4 (*const (&B)[N])[3], f32x4* const (&acc)[N]) {
#pragma unroll
  for (int p = 2; p >= 0; --p) {
#pragma unroll
    for (int s = 0; s < N; ++s) *acc[s] = mfma_bf16(A0, (*B[s])[p], *acc[s]);
  }
}
// registers 1, 2 keep their partial sums (finite, never NaN: sums of products of finite pieces).  Nothing reads them unguarded:
// at KS == 13 they are k-steps 13, 14, which every consumer of an accumulator tile either skips (ks < KS) or multiplies by a
// zero weight (the output layer's padding weights).
// The order of the two adds is free as far as accuracy goes (they differ by an ulp of the m- and l-rows, 2^-8 and 2^-16 of the
// result); h + m first, then l, is the order the whole suite was verified with: an L-BFGS trajectory test that hangs on
// the last bit of a loss of 10.5 stalls with l + m first (DESIGN_LOG G.3).
__device__ __forceinline__ void fold_rows(f32x4& t) { t[0] = (t[0] + t[1]) + t[2]; }

// ---- K halves (the fused step kernel at KS == 13: stage_split_hidden, FOLD13) -------------------------------------------------
// A K half of a 16x16x32 MFMA is 16 K entries: words 0, 1 or words 2, 3 of an A fragment (one row tile of the image: half an
// entry in the forward sweep, one transposed read in the sweep back) against registers e = 0, 1 or e = 2, 3 of a B operand.  Any
// two halves can share an MFMA as long as the A half and the B half of each pair match.  The second K fragment (q == 1) of a
// 50-wide layer is one full half T (k-steps 8..11) and one edge half E (k-step 12 and padding), and the in-fold / out-fold put
// the m- and the l-piece of the edge entry into slots 5, 6 of the PIECE-0 fragment, next to its h-piece in slot 4.  The six B
// halves of the fragment -- T_h, T_m, T_l and, with b the k-step-12 value, E_h = h(b) h(b) h(b) 0, E_m = m(b) m(b) 0 0,
// E_l = l(b) 0 0 0 -- are held as THREE operands, as many registers as the plain pieces take (khalf_pack):
//   K0 = [T_h | T_m]     K1 = [T_l | E_h]     K2 = [E_m | E_l]
// and a row tile 0..2 takes five MFMAs per stream instead of six (five_khalf; A0, A1, A2 the T halves of the three weight pieces,
// E0 the edge half of piece 0; a product is written weight piece first):
//   [A2 | 0 ] x K0    lh                          [A1 | A1] x K0    mh + mm
//   [E0 | E0] x K2    hm + mm, hl of the edge     [A0 | E0] x K1    hl, and hh + mh + lh of the edge
//   [A0 | A0] x K0    hh + hm
// -- the six products of every (in, out) pair exactly once; the edge halves of the piece-1 and piece-2 fragments are not read.
// The folded row tile (mt == 3), whose rows 0, 1, 2 are the h-, m- and l-pieces of the same weights, takes the same operands in
// three MFMAs (three_khalf): [E | E] x K2, [T | E] x K1, [T | T] x K0.  Its CORNER (folded rows x edge slots) must hold each
// weight piece once: rows 0, 1, 2 x slot 4 = h, m, l and zeros in slots 5, 6 (the in-fold skips row tile 3), else E_h and E_m
// would count mh, lh and mm twice.  The forward sweep then sums all nine piece products of the corner (rows against E_h, E_m,
// E_l in slot 4), the sweep back -- which sees the corner transposed: one row, slots 4, 5, 6 = h, m, l -- the six.
// Exact zeros this relies on: slot 7 of every A fragment and B operand (k-step 15), the high half of the k-step-12 B words
// (`full ? .. : 0.f`) and the k-step-14 B word (0u), the second half of the piece-2 operand.
// Order: small terms first inside each accumulator, as in `six`; the streams are interleaved product by product.
__device__ __forceinline__ u32 dup_lo16(u32 x) { return x | (x << 16); }        // x < 2^16: the bf16 in both halves
__device__ __forceinline__ void khalf_pack(const u32x4 (&B)[3], u32x4 (&K)[3]) {   // plain pieces h, m, l of k-steps 8..15 -> K0, K1, K2
  K[0] = u32x4{B[0][0], B[0][1], B[1][0], B[1][1]};
  K[1] = u32x4{B[2][0], B[2][1], dup_lo16(B[0][2]), B[0][2]};
  K[2] = u32x4{dup_lo16(B[1][2]), 0u, B[2][2], 0u};
}
// Aa = [A0 | A0], Ab = [A1 | A1], Ac = [A2 | 0], Ad = [A0 | E0], Ae = [E0 | E0]
template <int N>
__device__ __forceinline__ void five_khalf(const u32x4& Aa, const u32x4& Ab, const u32x4& Ac, const u32x4& Ad, const u32x4& Ae,
                                           const u32x4 (*const (&K)[N])[3], f32x4* const (&acc)[N]) {
#pragma unroll
  for (int s = 0; s < N; ++s) *acc[s] = mfma_bf16(Ac, (*K[s])[0], *acc[s]);
#pragma unroll
  for (int s = 0; s < N; ++s) *acc[s] = mfma_bf16(Ab, (*K[s])[0], *acc[s]);
#pragma unroll
  for (int s = 0; s < N; ++s) *acc[s] = mfma_bf16(Ae, (*K[s])[2], *acc[s]);
#pragma unroll
  for (int s = 0; s < N; ++s) *acc[s] = mfma_bf16(Ad, (*K[s])[1], *acc[s]);
#pragma unroll
  for (int s = 0; s < N; ++s) *acc[s] = mfma_bf16(Aa, (*K[s])[0], *acc[s]);
}
// the folded row tile: At = [T | T], Ad = [T | E], Ae = [E | E] of its one (piece-0) fragment
template <int N>
__device__ __forceinline__ void three_khalf(const u32x4& At, const u32x4& Ad, const u32x4& Ae, const u32x4 (*const (&K)[N])[3],
                                            f32x4* const (&acc)[N]) {
#pragma unroll
  for (int s = 0; s < N; ++s) *acc[s] = mfma_bf16(Ae, (*K[s])[2], *acc[s]);
#pragma unroll
  for (int s = 0; s < N; ++s) *acc[s] = mfma_bf16(Ad, (*K[s])[1], *acc[s]);
#pragma unroll
  for (int s = 0; s < N; ++s) *acc[s] = mfma_bf16(At, (*K[s])[0], *acc[s]);
}
__device__ __forceinline__ u32x4 lo_lo(const u32x4& a) { return u32x4{a[0], a[1], a[0], a[1]}; }
__device__ __forceinline__ u32x4 hi_hi(const u32x4& a) { return u32x4{a[2], a[3], a[2], a[3]}; }
__device__ __forceinline__ u32x4 halves(unsigned long long lo, unsigned long long hi) {
  return u32x4{(u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32)};
}

// Fragment reads of the fused kernel's image (IMGF, fblk)
__device__ __forceinline__ u32x4 ffrag_row1(const char* rl, int p, int q, int mt) {
  return *reinterpret_cast<const u32x4a*>(rl + fblk(p, q, mt) * BLK);
}
__device__ __forceinline__ void ffrag_row(const char* rl, int q, int mt, u32x4 (&Af)[3]) {
#pragma unroll
  for (int p = 0; p < 3; ++p) Af[p] = ffrag_row1(rl, p, q, mt);
}
// one transposed read: out-feature row tile mo (a K half of the sweep back) of in-position row tile mt
__device__ __forceinline__ unsigned long long ffrag_tr_half(const char* tl, int p, int mo, int mt) {
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(tl + fblk(p, mt >> 1, mo) * BLK + 8 * (mt & 1)));
  return __builtin_bit_cast(unsigned long long, v);
}
__device__ __forceinline__ u32x4 ffrag_tr1(const char* tl, int p, int q, int mt) {
  const unsigned long long l64 = ffrag_tr_half(tl, p, 2 * q, mt), h64 = ffrag_tr_half(tl, p, 2 * q + 1, mt);
  return u32x4{(u32)l64, (u32)(l64 >> 32), (u32)h64, (u32)(h64 >> 32)};
}
__device__ __forceinline__ void ffrag_tr(const char* tl, int q, int mt, u32x4 (&At)[3]) {
#pragma unroll
  for (int p = 0; p < 3; ++p) At[p] = ffrag_tr1(tl, p, q, mt);
}
// ---- host side: one dispatch walk, one launcher ----------------------------------------------------------------------------
template <int L_, int KS_, bool TANH_>
struct Inst {
  static constexpr int L = L_, KS = KS_;
  static constexpr bool TANH = TANH_;
};

// visit_*(net, none, f): f(Inst<L, KS, TANH>{}) for the pair of the list that serves `net`, `none` where the list has no such
// pair.  f is a generic lambda; what it does not instantiate (if constexpr) does not exist.
#define VN16_VISIT(LL, KK) \
  if (net.L == LL && ks == KK) return net.act == VN_ACT_TANH ? f(Inst<LL, KK, true>{}) : f(Inst<LL, KK, false>{});
#define VN16_DEFINE_VISIT(NAME, CASES)            \
  template <class R, class F>                     \
  R NAME(const VnNet& net, R none, F f) {         \
    const int ks = vn_fused16_ks(net);            \
    CASES(VN16_VISIT)                             \
    return none;                                  \
  }
VN16_DEFINE_VISIT(visit_all, VN16_CASES)
VN16_DEFINE_VISIT(visit_f32_point, VN16_F32_POINT_CASES)
VN16_DEFINE_VISIT(visit_split, VN16_SPLIT_CASES)
#undef VN16_DEFINE_VISIT
#undef VN16_VISIT

// The attribute that allows KERNEL (one instantiation: the state lives here) lds_bytes of dynamic LDS is per device and sticky:
// it is set once per device (bit mask; engines on different devices may be driven from different threads).  OCC: the workgroups
// of this instantiation a CU holds (registers, LDS) are asked for at the same time and cached; *occ receives them (else 1).
template <auto KERNEL, bool OCC = false>
hipError_t allow_lds_once(size_t lds_bytes, int* occ = nullptr) {
  static std::atomic<unsigned long long> attr_done{0};
  static std::atomic<int> occ_cached{1};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev & 63);
  if (!(attr_done.load(std::memory_order_acquire) & bit)) {
    hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    if (OCC) {
      int nb = 1;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)KERNEL, NTHREADS, lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        nb = 1;
      }
      occ_cached.store(nb < 1 ? 1 : nb, std::memory_order_relaxed);
    }
    attr_done.fetch_or(bit, std::memory_order_release);
  }
  if (occ) *occ = occ_cached.load(std::memory_order_relaxed);
  return hipSuccess;
}

// Launch of a point kernel: every wave walks 16-point chunks with a grid stride, so the grid is the workgroups the n points fill,
// capped at per_cu workgroups per CU.  per_cu <= 0: two where the cached occupancy allows it (OCC), else one.  Waves are
// independent in these kernels (no workgroup barrier in the chunk loop), so a second resident workgroup per CU -- where the
// instantiation's registers (<= 128) and weight images (<= 80 KB) allow it -- hides more of the LDS / transcendental latencies
// under the partner's MFMAs: 395 -> 382 us on the bench network with vn_pgrad16 (profiles/r5_dedup_ab.txt).
template <auto KERNEL, bool OCC, class ARGS>
hipError_t launch_chunks(const ARGS& a, long n, size_t lds_bytes, int ncu, int per_cu, hipStream_t s) {
  int occ = 1;
  const hipError_t e = allow_lds_once<KERNEL, OCC>(lds_bytes, &occ);
  if (e != hipSuccess) return e;
  if (per_cu <= 0) per_cu = occ >= 2 ? 2 : 1;
  const long wgs = ((n + CW - 1) / CW + NW - 1) / NW;
  const long cap = (long)ncu * per_cu;
  const int grid = (int)(wgs < cap ? wgs : cap);
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(NTHREADS), lds_bytes, s, a);
  return hipGetLastError();
}

}  // namespace vn16
