// Fused gfx950 kernel, 8-wave geometry: the same algorithm as vn_fused.hip (forward with one
// tangent, weak-form epilogue, full reverse pass in one persistent launch), two waves per SIMD.
//
// Cost model that shaped it (measured, tools/micro/*.hip): on gfx950 the f32 MFMA and the
// f32 VALU share one datapath -- kernel time ~ sum of MFMA cycles + sum of vector-instruction issue
// cycles + exposed waits, whatever the interleaving; a second wave per SIMD only hides latencies.  So the
// kernel minimises matrix cycles (padding), vector instructions and barrier phases, not "overlap".
//
// Geometry: workgroup = 8 waves (512 threads), 128-point tiles, 16 points per wave,
// v_mfma_f32_16x16x4_f32.  Feature f lives in k-step ks = f/4, lane group g = f%4 (lane = 16g+c,
// c = point), accumulator row ("position") pos(ks,g) = 16(ks>>2) + 4g + (ks&3).  Layers are chained in
// registers (the accumulator tile of layer l is the B operand of layer l+1); weights sit in LDS images
// with row stride 65.
//   * H = 50 (KS = 13): rows 48, 49 of every GEMM are accumulated on the VALU instead of a 4th MFMA tile.
//   * Weight gradients: operands are transposed through LDS images; 50-wide hidden layers use lane-major
//     images written with ds_write_addtid_b32, 3x3 core tiles + two v_mfma_f32_4x4x1 border jobs (H13);
//     output and (d_in <= 3) input layer are contracted per wave with 4x4x1 MFMAs, no workgroup barrier;
//     other shapes use the generic cooperative tiles (wgrad_layer).
//   * Accumulators persist across tiles in registers, those of up to three hidden layers in an LDS stash
//     (registers are short while the forward pass stores 2*KS*L activation values; scratch spills would go
//     through L2 to HBM).  Fixed summation order everywhere: results are bitwise reproducible.
//   * Hidden widths 33..50 with 2..5 hidden layers (bf_sweeps): forward and input-gradient sweeps as bf16-piece
//     products on the bf16 matrix pipe (vn_fused16_common.h); their images (20 KB per layer) leave the stash room for one
//     layer.  The fourth row tile of either sweep (features 48, 49) is folded: its idle rows carry the m- and l-pieces, three
//     MFMAs per K fragment and stream instead of six (stage_split_hidden, FOLD13); the second K fragment of the other row
//     tiles pairs its K halves, five MFMAs instead of six (five_khalf).
// Register budget: 256 VGPRs per wave (stored activations 2*KS*L = 130 at 5x50; 18 spilled at 5x50).
#include "vn_internal.h"
#include "vn_fused16_common.h"

namespace {
using namespace vn16;

constexpr int TSW = 132;      // transposition image row stride
// Rows of a transposition image.  Positions are accumulator rows 16(ks>>2)+4g+(ks&3); a 50-wide layer
// (KS == 13) uses positions 0..47, 48 (feature 48), 52 (feature 49), 49 (bias row) and one all-zero row,
// so its images are packed into 52 rows (position 52 -> row 51, every unused position -> the zero row 50):
// the 12 KB this frees hold another layer's accumulators (Lay::NST).
// Nets up to 32 wide (KS <= 8) use positions 0..31 only: their images keep 32 rows + one all-zero row (33).
__host__ __device__ constexpr int t_rows(int KS) { return KS == 13 ? 52 : KS <= 8 ? 33 : 64; }
template <int KS>
__device__ __forceinline__ int trow(int pos) {
  if (KS == 13) return pos < 50 ? pos : pos == 52 ? 51 : 50;
  if (KS <= 8) return pos < 32 ? pos : 32;
  return pos;
}
// Position of the constant-one row that carries the bias gradient: the first position past the layer's k-steps.
// KS == 16 (widths 51..64) has no position to spare, so the row of feature 63 is used where the layer does not have
// that feature; behind a 64-wide layer the bias gradient is summed by thin_bias instead (ones_row = false).
// KS == 8 (widths 21..32) likewise: the first spare position would be 32, i.e. a third 16-row tile -- 4 x 2 weight-gradient
// tiles for a gradient that fits 2 x 2 (the [10,20,30] net of Operator_1DtMOR.py:189 spent a quarter of its matrix work
// there) -- so the bias row rides at the position of feature 31 unless the layer is exactly 32 wide.
__host__ __device__ constexpr bool fullpos(int KS) { return KS == 16 || KS == 8; }      // 4*KS fills whole 16-row tiles
__host__ __device__ constexpr int vones(int KS) {
  if (fullpos(KS)) return 4 * KS - 1;
  for (int p = 0; p < 64; ++p)
    if (vks(p) >= KS) return p;
  return -1;
}
static_assert(vfeat(63) == 63 && vfeat(31) == 31 && vpos(7, 3) == 31, "position 4*KS-1 is feature 4*KS-1");
#ifndef VN_MERGED_ROUNDS
#define VN_MERGED_ROUNDS 1
#endif
__host__ __device__ constexpr bool merged_rounds(int L, int KS) { return VN_MERGED_ROUNDS && KS <= 8 && L >= 2; }   // one publish/contract round per hidden layer
// Hidden-layer sweeps (forward value + tangent, input-gradient z-bar + z-bar-dot) as bf16-piece products (vn_fused16_common.h):
// hidden widths 33..50 with 2..5 hidden layers.  The f32 MFMA shares its datapath with the f32 vector unit on gfx950, the bf16
// MFMA does not.  Each hidden layer's 20 KB piece image (IMGF) replaces its f32 image; the one stashed layer of weight-gradient
// accumulators stays in LDS where it fits (Lay::NST), else in global memory.  The second K fragment of both sweeps runs as paired
// K halves (five_khalf: 11 MFMAs per row tile and stream instead of 12).  64-wide layers and L > 5 keep the f32 sweeps.
__host__ __device__ constexpr bool bf_sweeps(int L, int KS) { return KS == 13 && L >= 2 && L <= 5; }

template <int L, int KS>
struct Lay {
  static constexpr int HP = 4 * KS;
  static constexpr bool BF = bf_sweeps(L, KS);
  static constexpr int HPWS = BF ? IMGF / 4 : al4(HP * WS);  // floats per hidden layer image
  static constexpr int W1_OFF = 0;                          // [8][WS]
  static constexpr int WH_OFF = al4(8 * WS);                // [L-1][HP][WS] | [L-1] bf16-piece images (BF)
  static constexpr int BI_OFF = WH_OFF + (L - 1) * HPWS;    // [L][64] biases in (tile, g, i) order
  static constexpr int WO_OFF = BI_OFF + L * 64;            // [4*KS]
  static constexpr int MISC_OFF = WO_OFF + al4(4 * KS);     // sInt[128] (+128 spare)
  static constexpr int T_OFF = MISC_OFF + 256;              // TA | TB
  static constexpr int G1_SZ = (4 * KS0 + 1) * HP;
  static constexpr int GH_SZ = (HP + 1) * HP;
  static constexpr int GO_OFF = G1_SZ + (L - 1) * GH_SZ;
  static constexpr int G_SZ = al4(GO_OFF + HP + 1);
  static constexpr bool MERGE = merged_rounds(L, KS);
  static constexpr int T_IMG = (MERGE ? 2 : 1) * 2 * t_rows(KS) * TSW;     // TA | TB ( | TA' | TB' : wgrad_layer)
  static constexpr int T_H13 = (KS == 13) ? 27 * (NW * 64 + 4) : 0;         // lane-major images of the 50-wide path (H13)
  static constexpr int T_MAX = T_IMG > T_H13 ? T_IMG : T_H13;
  // The gradient image of the final flush normally shares the transposition region.  Where it is larger than that
  // region AND the layout would then exceed the 160 KB (six 64-wide layers), it is laid over the weight images
  // instead, which are dead once the tile loop has ended (G_LOW; it must end below sInt, which the flush still uses).
  static constexpr int T_SZ_SHARED = al4(T_MAX > G_SZ ? T_MAX : G_SZ);
  static constexpr bool G_LOW = (T_OFF + T_SZ_SHARED > 160 * 256) && G_SZ <= MISC_OFF;
  static constexpr int T_SZ = G_LOW ? al4(T_MAX) : T_SZ_SHARED;
  static constexpr int G_OFF = G_LOW ? 0 : T_OFF;
  // Weight-gradient accumulators of the first NST hidden layers live in LDS between their uses
  // (2 x f32x4 per lane and layer): registers are short while the forward pass stores activations,
  // and what the compiler spills instead goes to scratch, i.e. through L2 to HBM.
  // Final flush: the thin layers' partial sums (input layer with d_in <= 3, output layer: 2 x f32x4 per lane and wave) are
  // parked in one slot per wave and added in wave order by the store phase -- no serial round per wave.  The slots lie in
  // the transposition region behind the gradient image where that leaves room, else over the weight images (dead once
  // the tile loop has ended; they end below sInt, which the flush still uses).
  static constexpr int SLOT_SZ = NW * 2 * 4 * 64;
  static constexpr bool SLOT_IN_T = G_LOW || (T_SZ - al4(G_SZ) >= SLOT_SZ);
  static constexpr int SLOT_OFF = G_LOW ? T_OFF : (SLOT_IN_T ? T_OFF + al4(G_SZ) : 0);
  static_assert(SLOT_IN_T || SLOT_SZ <= MISC_OFF, "thin-layer slots fit neither behind the gradient image nor over the weight images");
  static constexpr int ST_OFF = T_OFF + T_SZ;
  static constexpr int ST_LAYER = NW * 2 * 64 * 4;
  static constexpr int ST_FIT = (160 * 256 - ST_OFF) / ST_LAYER;
  // BF: ONE stashed layer (layer 2, the last of the reverse sweep); the others stay in registers.  Measured at 5 x 50 with the
  // stash in global memory (DESIGN_LOG G.1): 4 layers in the stash 7.45 ms, 3: 7.24, 2: 7.18, 1: 7.12-7.17, 0: 7.32 -- each stashed
  // layer's load sits behind a publish round and a barrier, and costs more than the 8 VGPRs of spill traffic it saves, until the
  // last one.  It lives in LDS like the f32 form's where the 20-block images leave room (they do up to 5 x 50), else in a
  // per-workgroup buffer in global memory ([layer][wave][slot][lane] f32x4, ST_LAYER floats per layer; every lane re-reads only
  // what it wrote one tile earlier, L2-resident).
  static constexpr int NSTB = (BF && L >= 3) ? 1 : 0;
  static constexpr int NST = BF ? (ST_FIT >= NSTB ? NSTB : 0)
                                : (((KS != 13 && KS != 16) || L < 3) ? 0 : (ST_FIT < L - 1 ? ST_FIT : L - 1));
  static constexpr int TOTAL = ST_OFF + NST * ST_LAYER;
  static constexpr int NSTG = BF ? NSTB - NST : 0;         // layers stashed in global memory
  static constexpr int NSTK = NST + NSTG;                  // stashed layers, wherever the stash lives
  static_assert(!BF || TOTAL <= 160 * 256, "bf16-piece images must fit the LDS");
};


struct LaneC {
  int g, c;
  int offF;        // forward A-fragment lane offset: g*WS + c            (+ 16*m + 4*ks*WS)
  int offB0;       // backward A-fragment lane offset of row tile 0: fin*WS + 4g   (+ 16m*WS + vpos(ks,0)): the
                   // in-features of row tile m are fin(c) + 16m, and 16*MTM <= HP in every instantiation
  int twr;         // transposition write offset: 4g*TSW + wave*16 + c     (+ vpos(ks,0)*TSW)
};

template <int KSA, int KSB>
struct WG {
  static constexpr int ONES = vones(KSA);
  static constexpr int MTA0 = (mtiles(KSA) > (ONES >> 4) + 1) ? mtiles(KSA) : (ONES >> 4) + 1;
  static constexpr int MTA = MTA0 == 3 ? 4 : MTA0;             // 1, 2 or 4 row tiles
  static constexpr int NTB0 = mtiles(KSB);
  static constexpr int NTB = NTB0 == 3 ? 4 : NTB0;
  static constexpr int NT = MTA * NTB;                         // output tiles (16x16): 1..16
  static constexpr int TPW = (NT >= NW) ? NT / NW : 1;         // tiles per wave (same row tile m)
  static constexpr int NS = (NT >= NW) ? 1 : NW / NT;          // point splits
  static constexpr int PTS = TILE / NS;                        // points contracted by one wave
  static constexpr int PG = PTS / 4;                           // ... by one lane group
  static constexpr int ones_m = ONES >> 4;
  static constexpr int ones_i = ONES & 3;
  static constexpr int ones_g = (ONES >> 2) & 3;
  static_assert(NT == 1 || NT == 2 || NT == 4 || NT == 8 || NT == 16, "tile count must divide the waves");
  static_assert(NT < NW || NTB % TPW == 0, "a wave's tiles must share a row tile");
};



// store of one published value: lane (c, g) owns row vpos(ks,0)+4g, column wave*16+c
template <int KS>
__device__ __forceinline__ void t_write(float* T, const LaneC& lc, int ks, float v) {
  if (KS == 13 && ks == 12) {                       // features 48, 49 -> rows 48, 51; 50, 51 are padding
    if (lc.g < 2) T[lc.twr + (48 - lc.g) * TSW] = v;
  } else {
    T[lc.twr + vpos(ks, 0) * TSW] = v;
  }
}

// Cooperative weight gradient (see vn_fused.hip): all waves publish their 16 point-columns of
// the transposed operands, then each wave contracts its output tile(s) over its share of the
// 128 points into persistent accumulators.
// ones_row: the layer's input side has a position to spare for the constant-one row that carries the bias gradient
// (always, except for a 64-wide input side at KS == 16: then the bias gradient comes from thin_bias below).
template <int KSA, int KSB, bool RAWA, bool TANH, bool MERGE, int NACC, class AV, class BV>
__device__ __forceinline__ void wgrad_layer(const AV& av, const AV& azd, const BV& bv, const BV& bt, float* TA,
                                            float* TB, const LaneC& lc, int wave, f32x4 (&acc)[NACC], bool ones_row) {
  using W = WG<KSA, KSB>;
  static_assert(NACC == W::TPW, "accumulator count");
  const int t0 = (W::NT >= NW) ? wave * W::TPW : wave % W::NT;
  const int sidx = (W::NT >= NW) ? 0 : wave / W::NT;
  const int m = t0 / W::NTB, n0 = t0 % W::NTB;
  // ds_read_b128 is served in 16-lane groups that mix two neighbouring lane groups g over 64
  // banks: with the row stride == 4 (mod 64) the 16 rows of a group are conflict-free only if
  // the point offsets of g and g^1 differ by a multiple of 64 -> g = 0,1,2,3 start at 0,64,32,96.
  const int goff = (W::PG == 32) ? 64 * (lc.g & 1) + 32 * (lc.g >> 1) : lc.g * W::PG;
  const int rdA = trow<KSA>(16 * m + lc.c) * TSW + sidx * W::PTS + goff;
  int rdBt[W::TPW];
#pragma unroll
  for (int t = 0; t < W::TPW; ++t) rdBt[t] = trow<KSB>(16 * (n0 + t) + lc.c) * TSW + sidx * W::PTS + goff;
  // Nets up to 32 wide (KS <= 8) have LDS to spare: value and tangent operands are published side by side (a second
  // image pair T2 floats on) and contracted behind ONE barrier pair per layer instead of two -- a small net's tile is a chain
  // of short phases between barriers, not matrix work (profiles/r3_small_stamps.txt).
  constexpr int T2 = MERGE ? 2 * t_rows(KSB) * TSW : 0;
  auto contract = [&](const float* TAh, const float* TBh) {
    f32x4 a4 = *reinterpret_cast<const f32x4a*>(&TAh[rdA]);
    f32x4 b4[W::TPW];
#pragma unroll
    for (int t = 0; t < W::TPW; ++t) b4[t] = *reinterpret_cast<const f32x4a*>(&TBh[rdBt[t]]);
#pragma unroll
    for (int j = 0; j < W::PG / 4; ++j) {
      f32x4 an = a4, bn[W::TPW];
#pragma unroll
      for (int t = 0; t < W::TPW; ++t) bn[t] = b4[t];
      if (j + 1 < W::PG / 4) {
        an = *reinterpret_cast<const f32x4a*>(&TAh[rdA + 4 * (j + 1)]);
#pragma unroll
        for (int t = 0; t < W::TPW; ++t)
          bn[t] = *reinterpret_cast<const f32x4a*>(&TBh[rdBt[t] + 4 * (j + 1)]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < W::TPW; ++t) acc[t] = mfma16(a4[e], b4[t][e], acc[t]);
      __builtin_amdgcn_sched_barrier(0);
      a4 = an;
#pragma unroll
      for (int t = 0; t < W::TPW; ++t) b4[t] = bn[t];
    }
  };
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    float* TAh = TA + half * T2;
    float* TBh = TB + half * T2;
    if constexpr (RAWA) {
#pragma unroll
      for (int ks = 0; ks < KSA; ++ks) t_write<KSA>(TAh, lc, ks, half == 0 ? av[ks] : azd[ks]);
    } else {
#pragma unroll
      for (int j = 0; j < PA<KSA>::NP; ++j) {            // sigma'(a) * zdot for two k-steps per packed instruction
        f32x2 v2 = av.p[j];
        if (half == 1) v2 = act_d1_2<TANH>(opaque2(av.p[j])) * azd.p[j];
        t_write<KSA>(TAh, lc, 2 * j, v2[0]);
        if (2 * j + 1 < KSA) t_write<KSA>(TAh, lc, 2 * j + 1, v2[1]);
      }
    }
    if (ones_row && lc.g == W::ones_g) TAh[lc.twr - 4 * lc.g * TSW + W::ONES * TSW] = (half == 0) ? 1.f : 0.f;
#pragma unroll
    for (int ks = 0; ks < KSB; ++ks) t_write<KSB>(TBh, lc, ks, (half == 0) ? bv[ks] : bt[ks]);
    if (MERGE && half == 0) continue;
    __syncthreads();
    if (MERGE) contract(TA, TB);
    contract(TAh, TBh);
    __syncthreads();
  }
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0);
}

// ---- thin layers: output layer (one column) and input layer with d_in <= 3 (rows x0..x2 + bias) ---
// Few rows (or columns) against all 64 positions is one 4x4x1 MFMA per point, so there is nothing to
// share between waves: every wave transposes its own 16 points through its own 16 columns of the
// images and contracts them at once -- no workgroup barrier, 16 short MFMAs per round instead of 16
// long ones, and the partial sums of the 8 waves meet in the fixed-order flush.
__device__ __forceinline__ void wave_lds_sync() {
  // LDS operations of one wave complete in order; the fences stop the compiler from moving a
  // lane's loads across other lanes' stores (per-thread alias reasoning)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A side: 64 positions (lane = row), B side: rows brow(j) for j = lane & 3;  TRANSPOSED swaps the roles
template <int KS, bool A_IS_LANE>
__device__ __forceinline__ void thin_contract(const float* TA, const float* TB, int rowsel, int wave, int lane, f32x4& acc) {
  const int rdA = (A_IS_LANE ? trow<KS>(lane) : rowsel) * TSW + wave * CW;
  const int rdB = (A_IS_LANE ? rowsel : trow<KS>(lane)) * TSW + wave * CW;
  f32x4 a4[CW / 4], b4[CW / 4];
#pragma unroll
  for (int q = 0; q < CW / 4; ++q) {
    a4[q] = *reinterpret_cast<const f32x4a*>(&TA[rdA + 4 * q]);
    b4[q] = *reinterpret_cast<const f32x4a*>(&TB[rdB + 4 * q]);
  }
  f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < CW / 4; ++q) {
    acc = mfma4(a4[q][0], b4[q][0], acc);
    t = mfma4(a4[q][1], b4[q][1], t);
    acc = mfma4(a4[q][2], b4[q][2], acc);
    t = mfma4(a4[q][3], b4[q][3], t);
  }
  acc += t;
}

// output layer: d w_o[f] = sum_p (a[f][p] ubar[p] + adot[f][p] udbar[p]).  Both seeds are per-point scalars, so the two products
// are combined per element IN REGISTERS, c = a ubar + (sigma'(a) zdot) udbar, and ONE transposition pass contracts c against a
// column of ones (the bias row carries ubar itself: d b_o = sum_p ubar[p]) -- half the LDS round trips and 4x4x1 MFMAs of the
// two-pass form, on a stretch of the tile where the matrix pipe is idle anyway.  Lanes g == 0 publish the ones into row 0
// of TB, the other lane groups zeros into rows 4, 8, 12.
template <int KS, bool TANH, class AV>
__device__ __forceinline__ void thin_wgrad_out(const AV& av, const AV& azd, float ubar, float udbar,
                                               float* TA, float* TB, const LaneC& lc, int wave, int lane, f32x4& acc,
                                               bool ones_row) {
  using W = WG<KS, 1>;
  const f32x2 ub2 = {ubar, ubar}, ud2 = {udbar, udbar};
#pragma unroll
  for (int j = 0; j < PA<KS>::NP; ++j) {
    const f32x2 a2 = opaque2(av.p[j]);
    const f32x2 c2 = a2 * ub2 + (act_d1_2<TANH>(a2) * azd.p[j]) * ud2;
    t_write<KS>(TA, lc, 2 * j, c2[0]);
    if (2 * j + 1 < KS) t_write<KS>(TA, lc, 2 * j + 1, c2[1]);
  }
  if (ones_row && lc.g == W::ones_g) TA[lc.twr - 4 * lc.g * TSW + W::ONES * TSW] = ubar;
  TB[lc.twr] = (lc.g == 0) ? 1.f : 0.f;
  wave_lds_sync();
  thin_contract<KS, true>(TA, TB, (lane & 3) == 0 ? 0 : 4, wave, lane, acc);
  wave_lds_sync();
}

template <int KS>
__device__ __forceinline__ void thin_flush_out(const f32x4& acc, float* Gl, int lane, bool ones_row) {
  if ((lane & 3) != 0) return;                         // column j = 0 holds the products with ubar
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pos = lane + i;
    if (ones_row && pos == vones(KS)) Gl[4 * KS] += acc[i];
    else if (vks(pos) < KS) Gl[vfeat(pos)] += acc[i];
  }
}

// Bias gradient of a layer whose 64-wide input side leaves no position for the constant-one row (KS == 16 only):
// sum_p zbar[j][p] as a thin contraction of a ones row against the wave's own 16 columns of zbar -- one 4x4x1 MFMA
// per point, no workgroup barrier (the images are free between two cooperative rounds; every wave touches only its
// own columns).  bsum: this lane's position j = lane.
template <int KS, class BV>
__device__ __forceinline__ void thin_bias(const BV& bv, float* TA, float* TB, const LaneC& lc, int wave, int lane, float& bsum) {
  using W = WG<KS0, KS>;
  const int sel = lane & 3;
  const int rowsel = sel == 3 ? W::ONES : 4 * sel;
  TA[lc.twr] = 0.f;                                                               // rows 0, 4, 8, 12: unused
  if (lc.g == W::ones_g) TA[lc.twr - 4 * lc.g * TSW + W::ONES * TSW] = 1.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) t_write<KS>(TB, lc, ks, bv[ks]);
  wave_lds_sync();
  f32x4 t = {0.f, 0.f, 0.f, bsum};
  thin_contract<KS, false>(TA, TB, rowsel, wave, lane, t);
  bsum = t[3];
  wave_lds_sync();
}

// input layer, d_in <= 3: rows x0, x1, x2 (positions 0, 4, 8) and the bias row against all columns
template <int KS, class BV>
__device__ __forceinline__ void thin_wgrad_in(const float (&xv)[KS0], const float (&gv)[KS0], const BV& bv,
                                              const BV& bt, float* TA, float* TB, const LaneC& lc, int wave,
                                              int lane, f32x4& acc) {
  using W = WG<KS0, KS>;
  const int sel = lane & 3;
  const int rowsel = sel == 3 ? W::ONES : 4 * sel;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    TA[lc.twr] = (half == 0) ? xv[0] : gv[0];                                     // feature g at position 4g
    if (lc.g == W::ones_g) TA[lc.twr - 4 * lc.g * TSW + W::ONES * TSW] = (half == 0) ? 1.f : 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) t_write<KS>(TB, lc, ks, (half == 0) ? bv[ks] : bt[ks]);
    wave_lds_sync();
    thin_contract<KS, false>(TA, TB, rowsel, wave, lane, acc);
    wave_lds_sync();
  }
}

template <int KS, int GS>
__device__ __forceinline__ void thin_flush_in(const f32x4& acc, float* Gl, int lane) {
  const int col = vfeat(lane);                         // lane = 4b + j = column position
  if (vks(lane) < KS && col < GS) {
#pragma unroll
    for (int i = 0; i < 3; ++i) Gl[i * GS + col] += acc[i];
    Gl[4 * KS0 * GS + col] += acc[3];                  // bias row of the input layer's gradient image
  }
}

// ---- 50-wide hidden layers (KS == 13) -----------------------------------------------------------
// A 51 x 50 gradient (50 inputs + bias row, 50 outputs) padded to 4 x 4 tiles of 16 x 16 wastes 38 %
// of the matrix work.  Here the 48 x 48 core is 3 x 3 tiles of v_mfma_f32_16x16x4_f32 and the two
// thin borders -- rows {48, 49, bias} x all columns and columns {48, 49} x rows 0..47 -- are
// accumulated with v_mfma_f32_4x4x1_16B_f32: 16 independent 4 x 4 blocks per instruction, one point
// per instruction, so a border of 4 rows x 64 columns costs 8 cycles per point instead of 32.
// Jobs (w and w+4 share a SIMD; every SIMD gets 3 tile-times instead of 4).  The matrix pipe
// alternates between the two waves of a SIMD per instruction, so an 8-cycle 4x4x1 stream paired with a
// 32-cycle 16x16x4 stream would crawl at the partner's pace: the two border jobs share a SIMD.
//   w = 0,1,2: tile (w,0) over all 128 points + tile (w,2) over one half of the points
//   w = 4,5,6: tile (w-4,1) over all points   + tile (w-4,2) over the other half
//   w = 3: row border          w = 7: column border
// so the six tile waves run one instruction stream (48 MFMAs per round) and share the A fragment.
// D layout of the 4x4x1 MFMA: lane 4b+j, register i  =  sum_p A[lane 4b+i] * B[lane 4b+j].
// Image layout of this path ("lane-major"): element (position pos, point (w, c)) of an image sits at
//   vks(pos)*RS + w*64 + g(pos)*16 + c          (g(pos) = (pos>>2)&3, RS = 8*64 + 4 floats)
// i.e. one image row per k-step holds, per wave, the 64 lanes of that wave's register in lane order.  A
// publishing store is then `ds_write_addtid_b32` (address = M0 + offset + 4*lane, no address VGPR,
// 128 B/clk/CU instead of the 64 B/clk of ds_write_b32 -- the publish rounds are bound by the LDS store
// path), and a reader still finds 4 consecutive points of one feature in one ds_read_b128.
// TA: rows 0..12 = k-steps, row 13 = [bias ones | zeros | zeros | zeros]; TB: rows 0..12.
struct H13 {
  static constexpr int RS = NW * 64 + 4;
  static constexpr int TA_ROWS = 14, TB_ROWS = 13;
  static constexpr int P48 = vpos(12, 0), P49 = vpos(12, 1);          // positions of features 48, 49
  static constexpr int ONES = vones(13);                              // position (13, g=0): the bias row
  static constexpr int ZERO = ONES + 4;                               // position (13, g=1): always zero (TA only)
  __host__ __device__ static constexpr int off(int pos) { return vks(pos) * RS + ((pos >> 2) & 3) * 16; }
  __device__ static __forceinline__ int edge_row(int i) { return i == 0 ? P48 : i == 1 ? P49 : i == 2 ? ONES : ZERO; }
  // role 0: core tiles; 1: row border; 2: column border
  __device__ static __forceinline__ int role(int wave) { return wave == 3 ? 1 : wave == 7 ? 2 : 0; }
  __device__ static __forceinline__ int tile_m(int wave) { return wave & 3; }
  __device__ static __forceinline__ int tile_n(int wave) { return wave >= 4 ? 1 : 0; }
};
static_assert(H13::ZERO == 53 && vks(H13::ZERO) == 13, "zero position");
static_assert(Lay<5, 13>::T_H13 == (H13::TA_ROWS + H13::TB_ROWS) * H13::RS, "image size");

// ds_write_addtid_b32: LDS[M0 + OFF + 4*lane] = v.  M0 is written once per publishing round (the wait
// state is the documented SALU-writes-M0 -> add-TID hazard); nothing else in this kernel uses M0.
__device__ __forceinline__ void addtid_base(unsigned m0_bytes) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" ::"s"(m0_bytes) : "memory");
}
template <int OFF_BYTES>
__device__ __forceinline__ void addtid_store(float v) {
  static_assert(OFF_BYTES >= 0 && OFF_BYTES < 65536, "16-bit offset");
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("ds_write_addtid_b32 %0 offset:%1" ::"v"(v), "n"(OFF_BYTES) : "memory");
#endif
}
__device__ __forceinline__ void addtid_drain() {     // the compiler does not count these stores in lgkmcnt
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

__device__ __forceinline__ void h13_contract(const float* TA, const float* TB, const LaneC& lc, int wave, int lane,
                                             f32x4 (&acc)[2]) {
  const int role = H13::role(wave);
  if (role == 1 || role == 2) {
    // border job: every lane walks all 128 points, 4 per ds_read_b128; two accumulators alternate
    const int sel = lane & 3;
    // offsets relative to TA (TB = TA + TBO): one LDS base pointer, integer selects only
    constexpr int TBO = H13::TA_ROWS * H13::RS;
    const int lane_off = vks(lane) * H13::RS + ((lane >> 2) & 3) * 16;        // lane = position
    const int oA = (role == 1) ? H13::off(H13::edge_row(sel)) : lane_off;
    const int oB = (role == 1) ? TBO + lane_off
                               : (sel == 0 ? TBO + H13::off(H13::P48) : sel == 1 ? TBO + H13::off(H13::P49) : H13::off(H13::ZERO));
    // TA lies past the first 64 KB of the LDS, out of reach of a DS immediate from a zero base: the lane bases carry TA's own
    // address (formed here, once per round, and pinned), and a stage's eight reads differ by immediates only
    typedef const __attribute__((address_space(3))) f32x4a* lds4;
    unsigned aA = (unsigned)(unsigned long)(const __attribute__((address_space(3))) float*)TA + 4u * oA;
    unsigned aB = (unsigned)(unsigned long)(const __attribute__((address_space(3))) float*)TA + 4u * oB;
    asm volatile("" : "+v"(aA), "+v"(aB));
    // 8 points per stage (wave w's columns 0..7 or 8..15), two register buffers used alternately (no
    // rotation copies: a stage's loads are waited for one stage later, behind 16 MFMAs)
    constexpr int NSTG = TILE / 8;
    f32x4 a0[2], b0[2], a1[2], b1[2];
    auto load = [&](f32x4 (&a4)[2], f32x4 (&b4)[2], int stage) {
      const unsigned o = 4u * ((stage >> 1) * 64 + (stage & 1) * 8);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        a4[h] = *(lds4)(unsigned long)(aA + o + 16u * h);
        b4[h] = *(lds4)(unsigned long)(aB + o + 16u * h);
      }
    };
    auto compute = [&](const f32x4 (&a4)[2], const f32x4 (&b4)[2]) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[0] = mfma4(a4[0][e], b4[0][e], acc[0]);
        acc[1] = mfma4(a4[1][e], b4[1][e], acc[1]);
      }
    };
    load(a0, b0, 0);
#pragma unroll 1
    for (int q = 0; q < NSTG; q += 2) {
      load(a1, b1, q + 1);
      compute(a0, b0);
      if (q + 2 < NSTG) load(a0, b0, q + 2);
      compute(a1, b1);
    }
    return;
  }
  // core tiles: lane (c, g) reads feature position 16m+c; lane group g contracts the points of waves
  // 2g and 2g+1 (so g and g^1 are 128 floats apart: conflict-free ds_read_b128, rows 4 banks apart)
  const int m = H13::tile_m(wave), n0 = H13::tile_n(wave);
  const int fo = (lc.c & 3) * H13::RS + (lc.c >> 2) * 16 + lc.g * 128;     // + 4m*RS for tile row m
  const int rdA = 4 * m * H13::RS + fo;
  const int rdB = 4 * n0 * H13::RS + fo;
  const int rdC = 4 * 2 * H13::RS + fo;
  // the shared tile (m,2) is contracted over one of the lane group's two waves only
  const int base1 = (wave >= NW / 2) ? 64 : 0, base2 = 64 - base1;
  f32x4 a4 = *reinterpret_cast<const f32x4a*>(&TA[rdA + base1]);
  f32x4 b4 = *reinterpret_cast<const f32x4a*>(&TB[rdB + base1]);
  f32x4 c4 = *reinterpret_cast<const f32x4a*>(&TB[rdC + base1]);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 an, bn, cn = c4;
    if (j + 1 < 4) {
      an = *reinterpret_cast<const f32x4a*>(&TA[rdA + base1 + 4 * (j + 1)]);
      bn = *reinterpret_cast<const f32x4a*>(&TB[rdB + base1 + 4 * (j + 1)]);
      cn = *reinterpret_cast<const f32x4a*>(&TB[rdC + base1 + 4 * (j + 1)]);
    } else {
      an = *reinterpret_cast<const f32x4a*>(&TA[rdA + base2]);
      bn = *reinterpret_cast<const f32x4a*>(&TB[rdB + base2]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[0] = mfma16(a4[e], b4[e], acc[0]);
      acc[1] = mfma16(a4[e], c4[e], acc[1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    a4 = an; b4 = bn; c4 = cn;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 an = a4, bn = b4;
    if (j + 1 < 4) {
      an = *reinterpret_cast<const f32x4a*>(&TA[rdA + base2 + 4 * (j + 1)]);
      bn = *reinterpret_cast<const f32x4a*>(&TB[rdB + base2 + 4 * (j + 1)]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[0] = mfma16(a4[e], b4[e], acc[0]);
    __builtin_amdgcn_sched_barrier(0);
    a4 = an; b4 = bn;
  }
}

// OPQ: sigma'(a) is formed from an opaque copy of a (the f32-sweep instantiations: left plain, the compiler keeps the packed
// sigma' of the forward sweep alive across the tile and spills for it; the bf16-piece sweeps have no such value to reuse, and
// there the copy is seven register-pair moves per round for nothing)
template <int KS_, int I, bool TANH, bool OPQ>
struct H13Pub {      // unrolled stores with compile-time offsets (inline-asm immediates)
  static __device__ __forceinline__ void run(int half, const PA<13>& av, const PA<13>& azd, const PA<13>& bv,
                                             const PA<13>& bt) {
    // I even: this step publishes k-steps I and I+1 (one packed sigma'(a)*zdot for both)
    f32x2 v2 = av.p[I >> 1];
    if (half == 1) v2 = act_d1_2<TANH>(OPQ ? opaque2(av.p[I >> 1]) : av.p[I >> 1]) * azd.p[I >> 1];
    addtid_store<I * H13::RS * 4>(v2[0]);
    addtid_store<(H13::TA_ROWS + I) * H13::RS * 4>(half == 0 ? bv[I] : bt[I]);
    if constexpr (I + 1 < KS_) {
      addtid_store<(I + 1) * H13::RS * 4>(v2[1]);
      addtid_store<(H13::TA_ROWS + I + 1) * H13::RS * 4>(half == 0 ? bv[I + 1] : bt[I + 1]);
    }
    if constexpr (I + 2 < KS_) H13Pub<KS_, I + 2, TANH, OPQ>::run(half, av, azd, bv, bt);
  }
};

// both rounds of a 50-wide hidden layer; t_base_bytes = byte address of this wave's 64 columns of TA
template <bool TANH, bool OPQ>
__device__ __forceinline__ void h13_wgrad_layer(const PA<13>& av, const PA<13>& azd, const PA<13>& bv,
                                                const PA<13>& bt, float* TA, const LaneC& lc, int wave, int lane,
                                                unsigned t_base_bytes, f32x4 (&acc)[2]) {
  const float* TB = TA + H13::TA_ROWS * H13::RS;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    addtid_base(t_base_bytes);
    H13Pub<13, 0, TANH, OPQ>::run(half, av, azd, bv, bt);
    addtid_store<13 * H13::RS * 4>((half == 0 && lc.g == 0) ? 1.f : 0.f);      // bias row | zeros
    addtid_drain();
    __syncthreads();
    h13_contract(TA, TB, lc, wave, lane, acc);
    __syncthreads();
  }
}

template <int GS>
__device__ __forceinline__ void h13_flush(const f32x4 (&acc)[2], float* Gl, const LaneC& lc, int wave, int lane,
                                          int slot_lo, int slot_hi) {   // tile waves: slots [slot_lo, slot_hi)
  const int role = H13::role(wave);
  if (role == 1) {                                   // rows 48, 49, bias x every column position
    const int pos = lane;                            // 4b + j
    const int col = vfeat(pos);
    if (vks(pos) < 13 && col < GS) {
      Gl[48 * GS + col] += acc[0][0] + acc[1][0];
      Gl[49 * GS + col] += acc[0][1] + acc[1][1];
      Gl[52 * GS + col] += acc[0][2] + acc[1][2];    // bias row of the gradient image (row 4*KS)
    }
    return;
  }
  if (role == 2) {                                   // rows 0..47 x columns 48, 49
    const int j = lane & 3;
    if (j < 2 && 48 + j < GS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int pos = (lane & ~3) + i;             // 4b + i
        if (pos < 48) Gl[vfeat(pos) * GS + 48 + j] += acc[0][i] + acc[1][i];
      }
    }
    return;
  }
  const int m = H13::tile_m(wave), n0 = H13::tile_n(wave);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t < slot_lo || t >= slot_hi) continue;
    const int col = vfeat(16 * (t ? 2 : n0) + lc.c);           // slot 1: this wave's share of tile (m,2)
    if (col < GS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) Gl[(4 * (4 * m + i) + lc.g) * GS + col] += acc[t][i];
    }
  }
}

template <int KSA, int KSB, int GS, int NACC>
__device__ __forceinline__ void wgrad_flush(const f32x4 (&acc)[NACC], float* Gl, const LaneC& lc, int wave, bool ones_row = true) {
  using W = WG<KSA, KSB>;
  const int t0 = (W::NT >= NW) ? wave * W::TPW : wave % W::NT;
  const int m = t0 / W::NTB, n0 = t0 % W::NTB;
#pragma unroll
  for (int t = 0; t < W::TPW; ++t) {
    const int cpos = 16 * (n0 + t) + lc.c;
    const bool colok = (vks(cpos) < KSB) && (vfeat(cpos) < GS);
    const int col = vfeat(cpos);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ks = 4 * m + i;
      int row = -1;
      if (ones_row && m == W::ones_m && i == W::ones_i && lc.g == W::ones_g) row = 4 * KSA;
      else if (ks < KSA) row = 4 * ks + lc.g;
      if (row >= 0 && colok) Gl[row * GS + col] += acc[t][i];
    }
  }
}




struct VnFusedArgsD {
  VnNet net;
  const float* theta;
  const float* X; const float* G; const float* src;
  long nT, n_k; int integ_num;
  const float* feN; const float* fedNt; const float* feW;
  const float* Nrow; const float* dNtrow;
  const float* detJv; float detJ; int time_dependent;
  float* lossVec;
  const float* Xb; const float* label; long nB, bDof; float biDimVal;
  float w0, w1, w2;
  float* partial;
  float* losspart;
  float* stash;             // [grid][Lay::NSTG][ST_LAYER] weight-gradient stash (bf16-piece instantiations), else unused
  unsigned long long* stamps;
  // de-duplicated formulation (rows = unique quadrature points, no test-function grouping):
  int mode;                 // 0 fused step; 1 forward only -> out_u/out_ud; 2 reverse pass with external seeds
  int dir;                  // >= 0: tangent direction is the unit vector e_dir (G ignored)
  int ostride;              // element stride of out_ud / seed_ud
  float* out_u; float* out_ud;
  const float* seed_u; const float* seed_ud;   // seed_u nullptr = 0, seed_ud nullptr = 1
};

template <int L, int KS, bool TANH>
__global__ __launch_bounds__(NTHREADS, 2) VN_NO_LDS_PAIRING void vn_fused16_kernel(VnFusedArgsD A) {
  using LY = Lay<L, KS>;
  using GE = Geo<KS>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const VnNet& net = A.net;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int P = net.P;
  float* W1 = lds + LY::W1_OFF;
  float* WH = lds + LY::WH_OFF;
  float* BI = lds + LY::BI_OFF;
  float* WO = lds + LY::WO_OFF;
  float* sInt = lds + LY::MISC_OFF;
  float* TA = lds + LY::T_OFF;
  float* TB = TA + t_rows(KS) * TSW;
  const unsigned t_base_bytes = (unsigned)((LY::T_OFF + wave * 64) * 4);      // lane-major images: this wave's columns
  float* Gacc = lds + LY::G_OFF;

  // lane constants that come from global memory are requested first, so that their latency hides under the prologue:
  // the quadrature index of this lane's point is the same in every interior tile (tiles start at whole test functions),
  // so the periodic FE table entries are lane constants
  const int q = A.integ_num;
  const int pq_l = (wave * CW + (lane & 15)) % q;
  const int tf_l = (wave * CW + (lane & 15)) / q;    // ... and so is its test function within the tile
  const float tab_dnt = A.time_dependent ? A.fedNt[pq_l] : 0.f;
  const float tab_w = A.feW ? A.feW[pq_l] : 1.f;
  const float tab_N = A.feN[pq_l];
  const float bo = A.theta[net.boff[L + 1]];
  // ------------------------------------------------------------------ prologue: LDS images
  {
    // Parameters are read in their own (row-major) order -- consecutive lanes, consecutive floats: a destination-driven
    // walk of the images gathers 4-byte words all over a layer and costs 4 us per launch on the texture path -- and
    // scattered into the images [in-feature][out-position]; every load is issued before anything waits, the zero fill of
    // the images (padding rows / columns must be exact zeros) and of the transposition region runs under their latency.
    const int d_in = net.d_in, H1 = net.H[1];
    constexpr int NSRC = (LY::HP * LY::HP + NTHREADS - 1) / NTHREADS;
    static_assert(8 * 64 <= NTHREADS, "layer 1: one parameter per thread");
    float v1 = 0.f, vh[L > 1 ? L - 1 : 1][NSRC];
    if (tid < d_in * H1) v1 = A.theta[net.woff[1] + tid];
#pragma unroll
    for (int l = 2; l <= (LY::BF ? 1 : L); ++l) {
      const int n = net.H[l - 1] * net.H[l];
      const float* src = A.theta + net.woff[l];
#pragma unroll
      for (int it = 0; it < NSRC; ++it) {
        const int j = tid + it * NTHREADS;
        vh[l - 2][it] = j < n ? src[j] : 0.f;
      }
    }
    // biases (one per thread: L * 64 <= 512) and output weights ride in the same batch of loads
    static_assert(L * 64 <= NTHREADS && 4 * KS <= NTHREADS, "one bias / output weight per thread");
    float vb = 0.f, vo = 0.f;
    if (tid < L * 64) {
      const int l = tid / 64 + 1, idx = tid % 64;
      const int mt = idx >> 4, g = (idx >> 2) & 3, r = idx & 3;       // [tile][g][i]
      const int ks = 4 * mt + r, f = 4 * ks + g;
      vb = (ks < KS && f < net.H[l]) ? A.theta[net.boff[l] + f] : 0.f;
    }
    if (tid < 4 * KS) vo = (tid < net.H[L]) ? A.theta[net.woff[L + 1] + tid] : 0.f;
    static_assert(LY::BI_OFF % 4 == 0 && LY::T_OFF % 4 == 0 && LY::T_SZ % 4 == 0, "16-byte zero fill");
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < (LY::BF ? LY::WH_OFF : LY::BI_OFF) / 4; i += NTHREADS) reinterpret_cast<f32x4a*>(lds)[i] = z4;   // W1 | WH
    for (int i = tid; i < LY::T_SZ / 4; i += NTHREADS) reinterpret_cast<f32x4a*>(lds + LY::T_OFF)[i] = z4;
    __syncthreads();
    if (tid < d_in * H1) {
      const int k = tid / H1, f = tid - k * H1;
      W1[k * WS + vpos(f >> 2, f & 3)] = v1;
    }
    if constexpr (LY::BF) stage_split_hidden<L, true>(net, A.theta, reinterpret_cast<char*>(WH), tid);
#pragma unroll
    for (int l = 2; l <= (LY::BF ? 1 : L); ++l) {
      float* Wl = WH + (l - 2) * LY::HPWS;
      const int Hout = net.H[l], n = net.H[l - 1] * Hout;
      const int dq = NTHREADS / Hout, dr = NTHREADS - dq * Hout;      // j -> j + NTHREADS: k += dq, f += dr (one carry)
      int k = tid / Hout, f = tid - k * Hout;
#pragma unroll
      for (int it = 0; it < NSRC; ++it) {
        if (tid + it * NTHREADS < n) Wl[k * WS + vpos(f >> 2, f & 3)] = vh[l - 2][it];
        f += dr; k += dq;
        if (f >= Hout) { f -= Hout; ++k; }
      }
    }
    if (tid < L * 64) BI[tid] = vb;
    if (tid < 4 * KS) WO[tid] = vo;
  }
  __syncthreads();

  LaneC lc;
  lc.g = lane >> 4;
  lc.c = lane & 15;
  lc.offF = lc.g * WS + lc.c;
  static_assert(16 * GE::MTM <= LY::HP, "backward fragment rows stay inside the weight image");
  static_assert(vfeat(16 + 5) == 16 + vfeat(5), "row tile m holds features fin(c) + 16m");
  lc.offB0 = vfeat(lc.c) * WS + 4 * lc.g;
  lc.twr = 4 * lc.g * TSW + wave * CW + lc.c;

  // persistent weight-gradient accumulators
  using W1G = WG<KS0, KS>;
  using WHG = WG<KS, KS>;
  constexpr bool HID13 = (KS == 13);                 // 50-wide hidden layers: 3x3 core tiles + 4x4x1 borders
  constexpr int NHACC = HID13 ? 2 : WHG::TPW;
  constexpr int ST_L = LY::ST_LAYER / 4;
  f32x4a* stash = (LY::NSTG ? reinterpret_cast<f32x4a*>(A.stash) + (long)blockIdx.x * LY::NSTG * ST_L
                          : reinterpret_cast<f32x4a*>(lds + LY::ST_OFF)) + wave * 2 * 64 + lane;   // [layer][wave][slot][lane]
  // bf16-piece sweeps: lane bases of the row (forward) and transposed (sweep back) fragment reads.
  // The images of layers 2..5 span 80 KB and a DS instruction's immediate offset reaches 64 KB.  Layers 2-4 (60 KB) are read from
  // the lane bases below; layer 5 forms its own base ONCE per sweep (win_base: one vector add, pinned where it stands), so that
  // every (piece, q, row tile) block offset is an immediate of its read instead of a vector add in front of it.  A second pair
  // of loop-invariant bases would cost two registers for the whole tile (+7 spilled); two layers per base instead of three
  // spill 29 registers instead of 18 at L = 5 (DESIGN_LOG G.9).
  constexpr int WINL = 3;
  static_assert((WINL - 1) * IMGF + 19 * BLK + 8 + 16 <= 65536, "block offsets of the first window are DS immediates");
  constexpr int WIN = WINL * IMGF;
  const int rowb = split_row_base(lc.g, lc.c), trb = split_tr_base(lc.g, lc.c);
  auto win_base = [&](int lane_base, int l) {          // image of layer l (2..L) + lane_base
    const char* wh = reinterpret_cast<const char*>(WH);
    if (l - 2 < WINL) return wh + lane_base + (l - 2) * IMGF;
    int b = lane_base + WIN;
    asm volatile("" : "+v"(b));
    return wh + b + (l - 2 - WINL) * IMGF;
  };
  f32x4 wacc1[W1G::TPW], wacch[L > 1 ? L - 1 : 1][NHACC];
  float woacc = 0.f, boacc = 0.f;                    // output layer: lane (g, c) holds d w_o[4c + g]; d b_o in every lane
#pragma unroll
  for (int t = 0; t < W1G::TPW; ++t) wacc1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int l = 0; l < (L > 1 ? L - 1 : 1); ++l)
#pragma unroll
    for (int t = 0; t < NHACC; ++t) {
      wacch[l][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (l < LY::NSTK) stash[l * ST_L + t * 64] = wacch[l][t];
    }

  const bool thin_in = net.d_in <= 3;                // input-layer weight gradient without workgroup barriers
  // KS == 16 with a 64-wide layer: its output side has no position left for the constant-one row of the NEXT layer's
  // weight gradient, whose bias gradient is then summed by thin_bias (hidden) / a per-lane scalar (output layer)
  bool ones_h[L > 1 ? L - 1 : 1];                    // layer l = 2..L: input side H[l-1] < 64
#pragma unroll
  for (int l = 2; l <= L; ++l) ones_h[l - 2] = !fullpos(KS) || net.H[l - 1] < 4 * KS;
  float bsum_h[L > 1 ? L - 1 : 1];
#pragma unroll
  for (int l = 0; l < (L > 1 ? L - 1 : 1); ++l) bsum_h[l] = 0.f;
  const int TT = TILE / q;                                   // whole test functions per tile
  const int TPTS = TT * q;                                   // points used in an interior tile (<= TILE)
  const bool qtree = (TILE % q) == 0;                        // q divides the tile: shuffle-tree R_k
  const long ntiles_i = A.mode ? (A.nT + TILE - 1) / TILE : (A.n_k + TT - 1) / TT;
  const long ntiles = ntiles_i + (A.mode == 1 ? 0 : (A.nB + TILE - 1) / TILE);
  float loss_var = 0.f, loss_bc = 0.f, loss_ic = 0.f;
  const long nI = A.nB - A.bDof;
  const float cb = A.bDof > 0 ? 2.f * A.w0 * A.biDimVal / (float)A.bDof : 0.f;
  const float ci = nI > 0 ? 2.f * A.w1 * A.biDimVal / (float)nI : 0.f;
  // Launch-uniform predicates of the tile loop, one bit each of ONE scalar register.  Left as plain conditions the compiler
  // hoists every one of them out of the loop as a 64-bit lane mask -- a pair of scalar registers each, spilled through
  // v_writelane / v_readlane on the vector path -- and branches on it through VCC; fl() tests a bit of an opaque copy where the
  // condition is used (scalar compare, branch on SCC).  The scalars compared against lane values (d_in, dim, dir, q) are made
  // opaque at their use for the same reason (sc()).
  enum : unsigned {
    FL_MODE1 = 1u << 0, FL_MODE2 = 1u << 1, FL_DIR = 1u << 2, FL_TD = 1u << 3, FL_DNTROW = 1u << 4, FL_SRC = 1u << 5,
    FL_NROW = 1u << 6, FL_QTREE = 1u << 7, FL_DETJV = 1u << 8, FL_LOSSVEC = 1u << 9, FL_SEEDU = 1u << 10, FL_SEEDUD = 1u << 11,
    FL_OUTU = 1u << 12, FL_OUTUD = 1u << 13, FL_THIN_IN = 1u << 14
  };
  const unsigned flags = (A.mode == 1 ? FL_MODE1 : 0u) | (A.mode == 2 ? FL_MODE2 : 0u) | (A.dir >= 0 ? FL_DIR : 0u) |
                         (A.time_dependent ? FL_TD : 0u) | (A.dNtrow ? FL_DNTROW : 0u) | (A.src ? FL_SRC : 0u) |
                         (A.Nrow ? FL_NROW : 0u) | (qtree ? FL_QTREE : 0u) | (A.detJv ? FL_DETJV : 0u) |
                         (A.lossVec ? FL_LOSSVEC : 0u) | (A.seed_u ? FL_SEEDU : 0u) | (A.seed_ud ? FL_SEEDUD : 0u) |
                         (A.out_u ? FL_OUTU : 0u) | (A.out_ud ? FL_OUTUD : 0u) | (thin_in ? FL_THIN_IN : 0u);
  auto fl = [flags](unsigned bits) {
    unsigned f = flags;
    asm volatile("" : "+s"(f));
    return (f & bits) != 0u;
  };
  auto sc = [](int v) {
    asm volatile("" : "+s"(v));
    return v;
  };
  const int d_in_s = net.d_in, dim_s = net.dim, dir_s = A.dir;

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    asm volatile("" ::: "memory");                 // keep LDS fragment loads inside the loop
    const bool interior = tile < ntiles_i;
    const bool moded = fl(FL_MODE1 | FL_MODE2);    // mode != 0
    const long r0 = (interior && !moded) ? tile * TPTS : (interior ? tile : tile - ntiles_i) * TILE;
    const long nrows = interior ? A.nT : A.nB;
    const int pt = wave * CW + lc.c;
    const long row = r0 + pt;
    const bool valid = row < nrows && (!interior || moded || pt < TPTS);

    float xin[KS0], gin[KS0];
    {
      const float* Xp = interior ? A.X : A.Xb;
#pragma unroll
      for (int s = 0; s < KS0; ++s) {
        const int f = 4 * s + lc.g;
        xin[s] = (valid && f < sc(d_in_s)) ? Xp[row * net.d_in + f] : 0.f;
        if (fl(FL_DIR)) gin[s] = (valid && interior && f == sc(dir_s)) ? 1.f : 0.f;
        else gin[s] = (valid && interior && f < sc(dim_s)) ? A.G[row * net.dim + f] : 0.f;
      }
    }

    PA<KS> a[L], zd[L];

    // ---------------------------------------------------------------- layer 1 (also recomputed late)
    auto layer1_raw = [&](const float (&xi)[KS0], const float (&gi)[KS0], f32x4 (&ov)[GE::MT], f32x4 (&ot)[GE::MT]) {
#pragma unroll
      for (int m = 0; m < GE::MT; ++m) {
        ov[m] = *reinterpret_cast<const f32x4a*>(&BI[m * 16 + lc.g * 4]);
        ot[m] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int s = 0; s < KS0; ++s) {
        if (4 * s < sc(d_in_s)) {
#pragma unroll
          for (int m = 0; m < GE::MT; ++m) {
            const float wf = W1[4 * s * WS + lc.offF + 16 * m];
            ov[m] = mfma16(wf, xi[s], ov[m]);
            ot[m] = mfma16(wf, gi[s], ot[m]);
          }
        }
      }
    };

    // ---------------------------------------------------------------- forward
    f32x4 pv[GE::MT], ptn[GE::MT];
    layer1_raw(xin, gin, pv, ptn);
#pragma unroll
    for (int l = 2; l <= L; ++l) {
      if constexpr (LY::BF) {
        // bf16 pieces: all four row tiles on the matrix pipe (features 48, 49 land in row 48 + 4g as in the edge path), value
        // and tangent share each weight fragment; the activation and the split are scalar f32 forms (no v_pk_* beside bf16 MFMAs).
        // Invariants of the folded fourth tile: the plain B pieces below are exact zeros at k-steps 13..15 (0u, `full ? .. : 0.f`), the
        // bias image is zero there, and registers 1..3 of tile 3 (finite partial sums after fold_rows, not 0) are read only
        // under ks < KS guards (B operands, H13Pub, the z-bar step) or against the zero padding weights of the output layer.
        // Invariants of the K halves (second fragment): khalf_pack FEEDS slots 5, 6 (E_h, E_m), so every A fragment holds there the
        // in-fold of its own slot 4 or an exact zero -- the corner of the folded tile zeros, each weight piece once in slot 4
        // (stage_split_hidden skips the in-fold in row tile 3), else E_h and E_m would count its mh, lh and mm twice; slot 7 is
        // zero on both sides; the folded tile takes the same three operands (three_khalf), no plain operand outlives the pack.
        const char* rl = win_base(rowb, l);
        f32x4 nv[GE::MT], nt[GE::MT];
#pragma unroll
        for (int m = 0; m < GE::MT; ++m) {
          nv[m] = *reinterpret_cast<const f32x4a*>(&BI[(l - 1) * 64 + m * 16 + lc.g * 4]);
          nt[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int qf = 0; qf < 2; ++qf) {             // K fragment: k-steps 8qf..8qf+7, cut per fragment (registers)
          u32x4 Bv[3], Bt[3];
#pragma unroll
          for (int e = 0; e < 4; ++e) {              // pair e = k-steps 8qf+2e, 8qf+2e+1 (13..15: padding, zero weights)
            const int k0 = 8 * qf + 2 * e;
            if (k0 >= KS) {
#pragma unroll
              for (int p = 0; p < 3; ++p) { Bv[p][e] = 0u; Bt[p][e] = 0u; }
              continue;
            }
            const int t = k0 >> 2, i = k0 & 3;
            const bool full = k0 + 1 < KS;
            const float a0 = act_fin<TANH>(act_exp<TANH>(pv[t][i]));
            const float a1 = full ? act_fin<TANH>(act_exp<TANH>(pv[t][i + 1])) : 0.f;
            const float z0 = ptn[t][i], z1 = full ? ptn[t][i + 1] : 0.f;
            a[l - 2].p[k0 >> 1] = f32x2{a0, a1};
            zd[l - 2].p[k0 >> 1] = f32x2{z0, z1};
            u32 h, md, lo;
            split2(a0, a1, h, md, lo);
            Bv[0][e] = h; Bv[1][e] = md; Bv[2][e] = lo;
            split2(act_d1<TANH>(a0) * z0, act_d1<TANH>(a1) * z1, h, md, lo);
            Bt[0][e] = h; Bt[1][e] = md; Bt[2][e] = lo;
          }
          if (qf == 1) {                             // T + the edge entry as K halves: 5 + 5 + 5 + 3 MFMAs per stream (five_khalf)
            u32x4 Kv[3], Kt[3];
            khalf_pack(Bv, Kv);
            khalf_pack(Bt, Kt);
            const u32x4 (*const Ks[2])[3] = {&Kv, &Kt};
#pragma unroll
            for (int mi = 0; mi < GE::MT; ++mi) {
              const int mt = (mi + 3) & 3;             // the folded tile first: 8 fewer registers spilled at L = 5 (DESIGN_LOG G.9)
              f32x4* const as[2] = {&nv[mt], &nt[mt]};
              const u32x4 Ad = ffrag_row1(rl, 0, 1, mt);
              if (mt == 3) three_khalf<2>(lo_lo(Ad), Ad, hi_hi(Ad), Ks, as);     // features 48, 49: folded edge tile
              else five_khalf<2>(lo_lo(Ad), ffrag_row1(rl, 1, 1, mt), ffrag_row1(rl, 2, 1, mt), Ad, hi_hi(Ad), Ks, as);
            }
            continue;
          }
#pragma unroll
          for (int mt = 0; mt < GE::MT; ++mt) {
            const u32x4 (*const Bs[2])[3] = {&Bv, &Bt};
            f32x4* const as[2] = {&nv[mt], &nt[mt]};
            if (mt == 3) {                           // features 48, 49: folded edge tile (the bias image is zero in rows 1..3)
              three_folded<2>(ffrag_row1(rl, 0, qf, mt), Bs, as);
              continue;
            }
            u32x4 Af[3];
            ffrag_row(rl, qf, mt, Af);
            six<2>(Af, Bs, as);
          }
        }
        fold_rows(nv[3]);
        fold_rows(nt[3]);
#pragma unroll
        for (int m = 0; m < GE::MT; ++m) { pv[m] = nv[m]; ptn[m] = nt[m]; }
        continue;
      }
      const float* Wl = WH + (l - 2) * LY::HPWS;
      int k_in = (net.H[l - 1] + 3) >> 2, m_out = (net.H[l] + 15) >> 4;      // GE::KSKIP: live k-steps / row tiles of this layer (scalar)
      f32x4 nv[GE::MT], nt[GE::MT];
#pragma unroll
      for (int m = 0; m < GE::MT; ++m) {
        nv[m] = *reinterpret_cast<const f32x4a*>(&BI[(l - 1) * 64 + m * 16 + lc.g * 4]);
        nt[m] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      // Activation of the previous layer, pipelined under this layer's MFMAs in PAIRS of k-steps (rows 2j, 2j+1 of an
      // accumulator tile are a register pair): stage A = packed scale + 2 v_exp, stage B = packed 1+e + 2 v_rcp,
      // stage C = packed sigma' * zdot.  Pair j is consumed by k-steps 2j and 2j+1; A(j+3) is issued after the first
      // of them, B(j+2) and C(j+1) after the second, so no transcendental chain is longer than one stage.
      // (The edge rows stay scalar FMAs: packing them -- across the edge features with splat activations, or along k
      // with weight pairs -- was measured 2.4-3.8 % SLOWER: the extra register pairs push 25 -> 48 spilled VGPRs.)
      constexpr int NP = PA<KS>::NP;
      auto zin2 = [&](int j) { return f32x2{pv[(2 * j) >> 2][(2 * j) & 3], pv[(2 * j) >> 2][((2 * j) & 3) + 1]}; };
      auto zdin2 = [&](int j) { return f32x2{ptn[(2 * j) >> 2][(2 * j) & 3], ptn[(2 * j) >> 2][((2 * j) & 3) + 1]}; };
      float wf[GE::MTM], we[GE::NVE], ev[GE::NVE], et[GE::NVE];
#pragma unroll
      for (int m = 0; m < GE::MTM; ++m) wf[m] = Wl[lc.offF + 16 * m];
#pragma unroll
      for (int v = 0; v < GE::NVE; ++v) {
        we[v] = GE::EDGE ? Wl[lc.offF - lc.c + GE::EPOS + 4 * v] : 0.f;
        ev[v] = 0.f;
        et[v] = 0.f;
      }
      f32x2 cs2 = act_fin2<TANH>(act_exp2<TANH>(zin2(0)));
      f32x2 cq2 = act_d1_2<TANH>(cs2) * zdin2(0);
      a[l - 2].p[0] = cs2;
      zd[l - 2].p[0] = zdin2(0);
      f32x2 s1 = (NP > 1) ? act_fin2<TANH>(act_exp2<TANH>(zin2(1))) : f32x2{0.f, 0.f};
      f32x2 e2 = (NP > 2) ? act_exp2<TANH>(zin2(2)) : f32x2{0.f, 0.f};
      f32x2 e3 = {0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int j = ks >> 1;
        float wn[GE::MTM], wen[GE::NVE];
#pragma unroll
        for (int m = 0; m < GE::MTM; ++m) wn[m] = (ks + 1 < KS) ? Wl[4 * (ks + 1) * WS + lc.offF + 16 * m] : 0.f;
#pragma unroll
        for (int v = 0; v < GE::NVE; ++v)
          wen[v] = (GE::EDGE && ks + 1 < KS) ? Wl[4 * (ks + 1) * WS + lc.offF - lc.c + GE::EPOS + 4 * v] : 0.f;
        const float cs = cs2[ks & 1], cq = cq2[ks & 1];
        __builtin_amdgcn_sched_barrier(0);
        if (GE::live_k(ks, k_in)) {
#pragma unroll
          for (int m = 0; m < GE::MTM; ++m) {
            if (!GE::live_m(m, m_out)) continue;
            nv[m] = mfma16(wf[m], cs, nv[m]);
            nt[m] = mfma16(wf[m], cq, nt[m]);
          }
        }
        if (GE::EDGE) {
#pragma unroll
          for (int v = 0; v < GE::NVE; ++v) { ev[v] += we[v] * cs; et[v] += we[v] * cq; }
        }
        if ((ks & 1) == 0) {
          if (j + 3 < NP) e3 = act_exp2<TANH>(zin2(j + 3));                  // stage A of pair j+3
          __builtin_amdgcn_sched_barrier(0);
        } else {
          f32x2 s2 = s1, q1 = cq2;
          if (j + 2 < NP) s2 = act_fin2<TANH>(e2);                            // stage B of pair j+2
          if (j + 1 < NP) {                                                    // stage C of pair j+1
            const f32x2 zz = zdin2(j + 1);
            q1 = act_d1_2<TANH>(s1) * zz;
            a[l - 2].p[j + 1] = s1;
            zd[l - 2].p[j + 1] = zz;
          }
          __builtin_amdgcn_sched_barrier(0);
          cs2 = s1; cq2 = q1; s1 = s2; e2 = e3;
        }
#pragma unroll
        for (int m = 0; m < GE::MTM; ++m) wf[m] = wn[m];
#pragma unroll
        for (int v = 0; v < GE::NVE; ++v) we[v] = wen[v];
      }
      if (GE::EDGE) {
        // sum the four lane groups' shares; group g keeps edge feature g
        nv[GE::MT - 1][0] += edge_reduce_scatter<GE::NVE>(ev, lc.g);         // bias was loaded above
        nt[GE::MT - 1][0] = edge_reduce_scatter<GE::NVE>(et, lc.g);
      }
#pragma unroll
      for (int m = 0; m < GE::MT; ++m) { pv[m] = nv[m]; ptn[m] = nt[m]; }
    }
    // rows (2j, 2j+1) of an accumulator tile are a register pair: pairs of k-steps per packed instruction (the
    // second half of a last, odd pair is a padding row: computed, never used)
    auto pairOf = [](const f32x4 (&t)[GE::MT], int j) { return f32x2{t[(2 * j) >> 2][(2 * j) & 3], t[(2 * j) >> 2][((2 * j) & 3) + 1]}; };
#pragma unroll
    for (int j = 0; j < PA<KS>::NP; ++j) {
      a[L - 1].p[j] = act_fin2<TANH>(act_exp2<TANH>(pairOf(pv, j)));
      zd[L - 1].p[j] = pairOf(ptn, j);
    }
    // output layer (VALU)
    float u = 0.f, ud = 0.f;
    {
      f32x2 u2 = {0.f, 0.f}, ud2 = {0.f, 0.f};
#pragma unroll
      for (int j = 0; j < PA<KS>::NP; ++j) {
        const bool full = 2 * j + 1 < KS;
        const f32x2 wv = {WO[4 * (2 * j) + lc.g], full ? WO[4 * (2 * j + 1) + lc.g] : 0.f};
        const f32x2 av = a[L - 1].p[j];
        u2 += wv * av;
        ud2 += wv * (act_d1_2<TANH>(av) * zd[L - 1].p[j]);
      }
      u = u2[0] + u2[1];
      ud = ud2[0] + ud2[1];
    }
    // sum over the four lane groups: row swaps (v_permlane16_swap / v_permlane32_swap, tools/micro/rowsum4_check.hip) instead of
    // two ds_bpermute round trips per value -- this stretch of the tile has no matrix work to hide an LDS latency behind;
    // same pairing as xor 16 then xor 32, so the same bits
    u = rowsum4(u);  ud = rowsum4(ud);
    u += bo;

    // ---------------------------------------------------------------- weak-form epilogue
    if (fl(FL_MODE1)) {                                      // forward only: model value and directional derivative
      if (valid && lc.g == 0) {
        if (fl(FL_OUTU)) A.out_u[row] = u;
        if (fl(FL_OUTUD)) A.out_ud[row * A.ostride] = ud;
      }
      continue;
    }
    float ubar = 0.f, udbar = 0.f;
    bool epi_barrier = false;                                // this tile's epilogue ran a workgroup barrier (uniform)
    if (interior && fl(FL_MODE2)) {                          // seeds were assembled per unique point
      if (valid) {
        ubar = fl(FL_SEEDU) ? A.seed_u[row] : 0.f;
        udbar = fl(FL_SEEDUD) ? A.seed_ud[row * A.ostride] : 1.f;   // no array: tangent seed 1 (the direction G carries the seeds)
      }
    } else if (interior) {
      // per-row tables (non-uniform supports, VarNetUtility.py:506-523) override the periodic ones
      const float dnt = !fl(FL_TD) ? 0.f : (fl(FL_DNTROW) ? (valid ? A.dNtrow[row] : 0.f) : tab_dnt);
      const float wq = tab_w;
      float t = ud - dnt * u;
      if (fl(FL_SRC)) t -= (valid ? A.src[row] : 0.f) * (fl(FL_NROW) ? (valid ? A.Nrow[row] : 0.f) : tab_N);
      t *= wq;
      if (!valid) t = 0.f;
      const int qs = sc(q);
      const int seg = qs < CW ? qs : CW;
      // A test function of up to 16 points (1D+t, two-point Gauss: q = 16) lies inside one wave: the butterfly below leaves
      // its sum R_k in every lane of the group (a + b == b + a bit for bit, so all lanes agree) -- no LDS, no workgroup barrier.
      const bool qtree_t = fl(FL_QTREE);
      const bool rk_in_wave = qtree_t && qs <= CW;
      if (qtree_t) {
        // butterfly over the seg <= 16 lanes of a test function's points, inside a 16-lane row: DPP moves (no LDS round
        // trip on the critical path of the epilogue).  After the two quad steps all lanes of a quad hold the same value, so
        // mirroring within 8 and within 16 lanes pairs the same sums as xor 4 / xor 8 would (bit-identical results).
        if (seg > 1) t += dpp_f32<0xB1>(t);        // quad_perm [1,0,3,2]
        if (seg > 2) t += dpp_f32<0x4E>(t);        // quad_perm [2,3,0,1]
        if (seg > 4) t += dpp_f32<0x141>(t);       // row_half_mirror
        if (seg > 8) t += dpp_f32<0x140>(t);       // row_mirror
        if (!rk_in_wave && lc.g == 0 && lc.c == 0) sInt[pt >> 4] = t;       // seg == CW here: q > CW
      } else if (lc.g == 0) {
        sInt[pt] = t;                                                 // q does not divide the tile: serial sum
      }
      if (!rk_in_wave) { __syncthreads(); epi_barrier = true; }
      // every lane sums the partials of its own test function (same order in all lanes, so all
      // agree bit for bit): no second barrier and no serial section
      float R = 0.f;
      if (rk_in_wave) {
        R = t;
      } else if (qtree_t) {
        const int per = qs >> 4;                                      // partials per test function, q / seg: seg == CW here (q > CW)
        if (per == 4) {
          // integNum 64 (2D+t, two-point Gauss): the four partials with one 16-byte read instead of four dependent round
          // trips right behind the barrier, where every wave of the workgroup waits for them; same order of additions
          const f32x4 s4 = *reinterpret_cast<const f32x4a*>(&sInt[tf_l * 4]);
          R = ((s4[0] + s4[1]) + s4[2]) + s4[3];
        } else {
          for (int j = 0; j < per; ++j) R += sInt[tf_l * per + j];    // :661
        }
      } else {
        for (int p = 0; p < qs; ++p) R += sInt[tf_l * qs + p];
      }
      const long k = tile * TT + tf_l;                                // = r0 / q + tf_l
      float s = 0.f;
      if (pt < TPTS && k < A.n_k) {
        const float dj = fl(FL_DETJV) ? A.detJv[k] : A.detJ;
        if (lc.g == 0 && pq_l == 0) {                                 // one lane per test function
          const float lv = dj * R * R;
          loss_var += lv;
          if (fl(FL_LOSSVEC)) A.lossVec[k] = lv;
        }
        s = 2.f * A.w2 * dj * R * wq;
      }
      udbar = s;
      ubar = -dnt * s;
    } else {
      if (valid) {
        const float e = u - A.label[row];
        const bool isbc = row < A.bDof;
        if (lc.g == 0) {
          const float e2 = A.biDimVal * e * e;
          if (isbc) loss_bc += e2; else loss_ic += e2;
        }
        ubar = (isbc ? cb : ci) * e;
      }
    }

    // ---------------------------------------------------------------- backward
    PA<KS> zb, zdb;
#pragma unroll
    for (int j = 0; j < PA<KS>::NP; ++j) {
      const bool full = 2 * j + 1 < KS;
      const f32x2 wv = {WO[4 * (2 * j) + lc.g], full ? WO[4 * (2 * j + 1) + lc.g] : 0.f};
      const f32x2 av = opaque2(a[L - 1].p[j]);
      const f32x2 sp = act_d1_2<TANH>(av);
      const f32x2 ab = wv * f32x2{ubar, ubar}, adb = wv * f32x2{udbar, udbar};
      const f32x2 zq = adb * sp;
      zdb.p[j] = zq;
      zb.p[j] = ab * sp + zq * act_d2r_2<TANH>(av) * zd[L - 1].p[j];
      // Output-layer weight gradient, no LDS, no MFMA, no barrier: d w_o[f] = sum_p (a[f][p] ubar[p] + adot[f][p] udbar[p]).
      // Both seeds are per-point scalars, so the products are combined per element in registers and summed over the 16
      // lanes of a row (= the wave's 16 points of feature 4 ks + g) with DPP moves; lane c == ks of each row keeps the sum
      // of k-step ks.  This stretch of the tile (epilogue -> first publish round) has no matrix work to hide an LDS round
      // trip behind, and the images stay untouched until the first publish.
      const f32x2 c2 = av * f32x2{ubar, ubar} + (sp * zd[L - 1].p[j]) * f32x2{udbar, udbar};
      const float s0 = rowsum16(c2[0]);
      woacc += (lc.c == 2 * j) ? s0 : 0.f;
      if (2 * j + 1 < KS) {
        const float s1 = rowsum16(c2[1]);
        woacc += (lc.c == 2 * j + 1) ? s1 : 0.f;
      }
    }
    boacc += rowsum16(ubar);                 // d loss / d b_o = sum_p ubar_p (every lane of the wave holds the wave's sum)
    // The lane-major images of the hidden layers overlap other waves' columns of the per-wave (input-layer) transposition
    // at the end of the previous tile: a tile whose epilogue had its own workgroup barrier is already past it.
    if constexpr (HID13) { if (!epi_barrier) __syncthreads(); }
#pragma unroll
    for (int l = L; l >= 2; --l) {
      if (l == 2 && L > 2) {                                 // bring layer-1 activations back
        float xr[KS0], gr[KS0];
#pragma unroll
        for (int s = 0; s < KS0; ++s) { xr[s] = opaque(xin[s]); gr[s] = opaque(gin[s]); }
        f32x4 rv[GE::MT], rt[GE::MT];
        layer1_raw(xr, gr, rv, rt);
#pragma unroll
        for (int j = 0; j < PA<KS>::NP; ++j) {
          a[0].p[j] = act_fin2<TANH>(act_exp2<TANH>(pairOf(rv, j)));
          zd[0].p[j] = pairOf(rt, j);
        }
      }
      if constexpr (HID13) {
        if (l - 2 < LY::NSTK) {
          f32x4 acc2[2] = {stash[(l - 2) * ST_L], stash[(l - 2) * ST_L + 64]};
          h13_wgrad_layer<TANH, !LY::BF>(a[l - 2], zd[l - 2], zb, zdb, TA, lc, wave, lane, t_base_bytes, acc2);
          stash[(l - 2) * ST_L] = acc2[0];
          stash[(l - 2) * ST_L + 64] = acc2[1];
        } else {
          h13_wgrad_layer<TANH, !LY::BF>(a[l - 2], zd[l - 2], zb, zdb, TA, lc, wave, lane, t_base_bytes, wacch[l - 2]);
        }
      }
      else if constexpr (NHACC == 2) {
        if (l - 2 < LY::NSTK) {               // accumulators of this layer live in the LDS stash between tiles
          f32x4 acc2[2] = {stash[(l - 2) * ST_L], stash[(l - 2) * ST_L + 64]};
          wgrad_layer<KS, KS, false, TANH, LY::MERGE>(a[l - 2], zd[l - 2], zb, zdb, TA, TB, lc, wave, acc2, ones_h[l - 2]);
          stash[(l - 2) * ST_L] = acc2[0];
          stash[(l - 2) * ST_L + 64] = acc2[1];
        } else {
          wgrad_layer<KS, KS, false, TANH, LY::MERGE>(a[l - 2], zd[l - 2], zb, zdb, TA, TB, lc, wave, wacch[l - 2], ones_h[l - 2]);
        }
      }
      else wgrad_layer<KS, KS, false, TANH, LY::MERGE>(a[l - 2], zd[l - 2], zb, zdb, TA, TB, lc, wave, wacch[l - 2], ones_h[l - 2]);
      if constexpr (fullpos(KS)) {
        if (!ones_h[l - 2]) thin_bias<KS>(zb, TA, TB, lc, wave, lane, bsum_h[l - 2]);
      }
      f32x4 accv[GE::MT], acct[GE::MT];
#pragma unroll
      for (int m = 0; m < GE::MT; ++m) { accv[m] = f32x4{0.f, 0.f, 0.f, 0.f}; acct[m] = f32x4{0.f, 0.f, 0.f, 0.f}; }
      if constexpr (LY::BF) {
        // bf16 pieces through the transposed reads of the same images: K fragment over the OUT-features 4(8qf+j)+g of layer l,
        // row tile over the IN-positions 16 mt + c (all four on the matrix pipe).  K halves (second fragment): the edge half E0 is
        // the transposed read of out row tile 3, whose rows 4g + 0, 1, 2 are the h-, m- and l-pieces of out-feature 48 + g (out-fold),
        // row 4g + 3 zero; for the folded IN tile it is the corner seen transposed -- one row, slots 4, 5, 6 = h, m, l, the in-fold
        // rows zero there -- so E_h, E_m, E_l give its six products once.  Same invariants as in the forward sweep.
        const char* tl = win_base(trb, l);
#pragma unroll
        for (int qf = 0; qf < 2; ++qf) {
          u32x4 Bz[3], Bzd[3];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int k0 = 8 * qf + 2 * e;
            if (k0 >= KS) {
#pragma unroll
              for (int p = 0; p < 3; ++p) { Bz[p][e] = 0u; Bzd[p][e] = 0u; }
              continue;
            }
            const bool full = k0 + 1 < KS;
            u32 h, md, lo;
            split2(zb[k0], full ? zb[k0 + 1] : 0.f, h, md, lo);
            Bz[0][e] = h; Bz[1][e] = md; Bz[2][e] = lo;
            split2(zdb[k0], full ? zdb[k0 + 1] : 0.f, h, md, lo);
            Bzd[0][e] = h; Bzd[1][e] = md; Bzd[2][e] = lo;
          }
          if (qf == 1) {                             // out-features 32..47 + the out-fold rows of 48, 49 as K halves (five_khalf)
            u32x4 Kz[3], Kzd[3];
            khalf_pack(Bz, Kz);
            khalf_pack(Bzd, Kzd);
            const u32x4 (*const Ks[2])[3] = {&Kz, &Kzd};
#pragma unroll
            for (int mt = 0; mt < GE::MT; ++mt) {
              f32x4* const as[2] = {&accv[mt], &acct[mt]};
              const unsigned long long T0 = ffrag_tr_half(tl, 0, 2, mt), E0 = ffrag_tr_half(tl, 0, 3, mt);
              if (mt == 3) {                         // in-features 48, 49: the mirror fold (in-slots 5, 6 of piece 0)
                three_khalf<2>(halves(T0, T0), halves(T0, E0), halves(E0, E0), Ks, as);
                continue;
              }
              const unsigned long long T1 = ffrag_tr_half(tl, 1, 2, mt), T2 = ffrag_tr_half(tl, 2, 2, mt);
              five_khalf<2>(halves(T0, T0), halves(T1, T1), halves(T2, 0ull), halves(T0, E0), halves(E0, E0), Ks, as);
            }
            continue;
          }
#pragma unroll
          for (int mt = 0; mt < GE::MT; ++mt) {
            const u32x4 (*const Bs[2])[3] = {&Bz, &Bzd};
            f32x4* const as[2] = {&accv[mt], &acct[mt]};
            if (mt == 3) {                           // in-features 48, 49: the mirror fold (in-slots 5, 6 of piece 0)
              three_folded<2>(ffrag_tr1(tl, 0, qf, mt), Bs, as);
              continue;
            }
            u32x4 At[3];
            ffrag_tr(tl, qf, mt, At);
            six<2>(At, Bs, as);
          }
        }
        fold_rows(accv[3]);
        fold_rows(acct[3]);
      } else {
      const float* Wl = WH + (l - 2) * LY::HPWS;
      int k_out = (net.H[l] + 3) >> 2, m_in = (net.H[l - 1] + 15) >> 4;
      float wf[GE::MTM], we[GE::NVE], ev[GE::NVE], et[GE::NVE];
#pragma unroll
      for (int m = 0; m < GE::MTM; ++m) wf[m] = Wl[lc.offB0 + 16 * m * WS + vpos(0, 0)];
#pragma unroll
      for (int v = 0; v < GE::NVE; ++v) {
        we[v] = GE::EDGE ? Wl[(4 * (KS - 1) + v) * WS + 4 * lc.g + vpos(0, 0)] : 0.f;
        ev[v] = 0.f;
        et[v] = 0.f;
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        float wn[GE::MTM], wen[GE::NVE];
#pragma unroll
        for (int m = 0; m < GE::MTM; ++m) wn[m] = (ks + 1 < KS) ? Wl[lc.offB0 + 16 * m * WS + vpos(ks + 1, 0)] : 0.f;
#pragma unroll
        for (int v = 0; v < GE::NVE; ++v)
          wen[v] = (GE::EDGE && ks + 1 < KS) ? Wl[(4 * (KS - 1) + v) * WS + 4 * lc.g + vpos(ks + 1, 0)] : 0.f;
        __builtin_amdgcn_sched_barrier(0);
        if (GE::live_k(ks, k_out)) {
#pragma unroll
          for (int m = 0; m < GE::MTM; ++m) {
            if (!GE::live_m(m, m_in)) continue;
            accv[m] = mfma16(wf[m], zb[ks], accv[m]);
            acct[m] = mfma16(wf[m], zdb[ks], acct[m]);
          }
        }
        if (GE::EDGE) {
#pragma unroll
          for (int v = 0; v < GE::NVE; ++v) { ev[v] += we[v] * zb[ks]; et[v] += we[v] * zdb[ks]; }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < GE::MTM; ++m) wf[m] = wn[m];
#pragma unroll
        for (int v = 0; v < GE::NVE; ++v) we[v] = wen[v];
      }
      if (GE::EDGE) {
        accv[GE::MT - 1][0] = edge_reduce_scatter<GE::NVE>(ev, lc.g);
        acct[GE::MT - 1][0] = edge_reduce_scatter<GE::NVE>(et, lc.g);
      }
      }
      // zbar of layer l-1, two k-steps per packed instruction (accumulator rows ks, ks+1 are a register pair)
#pragma unroll
      for (int j = 0; j < PA<KS>::NP; ++j) {
        const int ks = 2 * j;
        if (ks + 1 < KS) {
          const f32x2 av = opaque2(a[l - 2].p[j]);
          const f32x2 sp = act_d1_2<TANH>(av);
          const f32x2 ab = {accv[ks >> 2][ks & 3], accv[ks >> 2][(ks & 3) + 1]};
          const f32x2 adb = {acct[ks >> 2][ks & 3], acct[ks >> 2][(ks & 3) + 1]};
          const f32x2 zq = adb * sp;
          zdb.p[j] = zq;
          zb.p[j] = ab * sp + zq * act_d2r_2<TANH>(av) * zd[l - 2].p[j];
        } else {
          const float av = opaque(a[l - 2][ks]);
          const float sp = act_d1<TANH>(av);
          const float ab = accv[ks >> 2][ks & 3], adb = acct[ks >> 2][ks & 3];
          zdb.set(ks, adb * sp);
          zb.set(ks, ab * sp + adb * sp * act_d2r<TANH>(av) * zd[l - 2][ks]);
        }
      }
    }
    if (fl(FL_THIN_IN)) thin_wgrad_in<KS>(xin, gin, zb, zdb, TA, TB, lc, wave, lane, wacc1[0]);
    else wgrad_layer<KS0, KS, true, TANH, LY::MERGE>(xin, gin, zb, zdb, TA, TB, lc, wave, wacc1, true);
  }

  // ------------------------------------------------------------------ epilogue
  __syncthreads();
  for (int i = tid; i < (LY::G_LOW ? LY::G_SZ : LY::T_SZ); i += NTHREADS) lds[LY::G_OFF + i] = 0.f;
  __syncthreads();
  // Accumulators -> LDS gradient image, every sum in a fixed order (bitwise reproducible).
  // Thin layers first: all eight waves hold partial sums of the same elements; each parks its registers in its own slot
  // ([wave][input | output layer][register][lane]) and the store phase below adds the slots in wave order.
  float* SL = lds + LY::SLOT_OFF;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    SL[((wave * 2 + 0) * 4 + i) * 64 + lane] = thin_in ? wacc1[0][i] : 0.f;
    SL[((wave * 2 + 1) * 4 + i) * 64 + lane] = (i == 0) ? woacc : boacc;
  }
  if constexpr (HID13) {
    // 50-wide hidden layers: a tile wave's first slot and the two border jobs own their image elements
    // exclusively (one parallel phase); the shared tile (m,2) gets its two halves in two phases.
    auto flush_hidden = [&](int slot_lo, int slot_hi) {
#pragma unroll
      for (int l = 2; l <= L; ++l) {
        f32x4 acc2[2];
        if (l - 2 < LY::NSTK) { acc2[0] = stash[(l - 2) * ST_L]; acc2[1] = stash[(l - 2) * ST_L + 64]; }
        else { acc2[0] = wacch[l - 2][0]; acc2[1] = wacch[l - 2][1]; }
        h13_flush<LY::HP>(acc2, Gacc + LY::G1_SZ + (l - 2) * LY::GH_SZ, lc, wave, lane, slot_lo, slot_hi);
      }
    };
    const bool border = H13::role(wave) != 0;
    flush_hidden(0, border ? 2 : 1);
    __syncthreads();
    if (!border && wave < NW / 2) flush_hidden(1, 2);
    __syncthreads();
    if (!border && wave >= NW / 2) flush_hidden(1, 2);
    if (!thin_in) {                                  // d_in > 3: generic cooperative tiles of the input layer, one round per point split
      using W1 = WG<KS0, KS>;
      const int s1 = (W1::NT >= NW) ? 0 : wave / W1::NT;
      for (int r = 0; r < ((W1::NT >= NW) ? 1 : W1::NS); ++r) {
        __syncthreads();
        if (s1 == r) wgrad_flush<KS0, KS, LY::HP>(wacc1, Gacc, lc, wave);
      }
    }
    __syncthreads();
  } else {
    // generic tiles: waves with the same point-split index own distinct tiles, so round r serves all waves
    // of split r at once (one round when a layer has >= 8 tiles)
    using W1 = WG<KS0, KS>;
    const int s1 = (W1::NT >= NW) ? 0 : wave / W1::NT;
    const int sh = (WHG::NT >= NW) ? 0 : wave / WHG::NT;
    constexpr int R1 = (W1::NT >= NW) ? 1 : W1::NS;
    constexpr int RH = (L > 1) ? ((WHG::NT >= NW) ? 1 : WHG::NS) : 0;
    // bias gradients that did not ride in a constant-one row (KS == 16 behind a 64-wide layer) are per-wave partial sums
    // added in wave order: those rare shapes keep one round per wave
    bool serial_bias = false;
    if constexpr (fullpos(KS)) {
#pragma unroll
      for (int l = 2; l <= L; ++l) serial_bias = serial_bias || !ones_h[l - 2];
    }
    const int r1 = thin_in ? 0 : R1;
    const int nr = serial_bias ? NW : (r1 > RH ? r1 : RH);
    for (int r = 0; r < nr; ++r) {
      if (!thin_in && s1 == r && r < R1) wgrad_flush<KS0, KS, LY::HP>(wacc1, Gacc, lc, wave);
      if (sh == r && r < RH) {
#pragma unroll
        for (int l = 2; l <= L; ++l) {
          if constexpr (NHACC == 2) {
            if (l - 2 < LY::NSTK) {
              const f32x4 acc2[2] = {stash[(l - 2) * ST_L], stash[(l - 2) * ST_L + 64]};
              wgrad_flush<KS, KS, LY::HP>(acc2, Gacc + LY::G1_SZ + (l - 2) * LY::GH_SZ, lc, wave, ones_h[l - 2]);
              continue;
            }
          }
          wgrad_flush<KS, KS, LY::HP>(wacch[l - 2], Gacc + LY::G1_SZ + (l - 2) * LY::GH_SZ, lc, wave, ones_h[l - 2]);
        }
      }
      if constexpr (fullpos(KS)) {
        if (serial_bias && wave == r) {
          // hidden: lane = position of the output feature; output layer: sum over the wave's 16 points
#pragma unroll
          for (int l = 2; l <= L; ++l)
            if (!ones_h[l - 2] && vfeat(lane) < LY::HP)
              Gacc[LY::G1_SZ + (l - 2) * LY::GH_SZ + LY::HP * LY::HP + vfeat(lane)] += bsum_h[l - 2];
        }
      }
      __syncthreads();
    }
    if (nr == 0) __syncthreads();                    // the slots must be visible to the store phase
  }
  float* out = A.partial + (long)blockIdx.x * P;
#pragma unroll
  for (int l = 1; l <= L + 1; ++l) {
    const int Hin = net.H[l - 1], Hout = net.H[l];
    const int gs = (l == L + 1) ? 1 : LY::HP;
    const int brow = (l == 1) ? 4 * KS0 : LY::HP;
    const float* Gl = Gacc + ((l == 1) ? 0 : (l == L + 1) ? LY::GO_OFF : LY::G1_SZ + (l - 2) * LY::GH_SZ);
    // 64 consecutive threads write one row of the [Hin+1, Hout] block (coalesced, no integer division)
    const int cc = tid & 63;
    if (cc < Hout) {
      for (int r = tid >> 6; r <= Hin; r += NTHREADS / 64) {
        float v = Gl[(r < Hin ? r : brow) * gs + cc];
        if (l == 1 && thin_in) {
          // thin_wgrad_in: register i = input row (3 = bias row), lane = column position of feature cc
          const float* sp = SL + (r < Hin ? r : 3) * 64 + vpos(cc >> 2, cc & 3);
#pragma unroll
          for (int w = 0; w < NW; ++w) v += sp[(w * 2 + 0) * 4 * 64];
        } else if (l == L + 1) {
          // output layer: slot register 0 = woacc (lane 16 g + c holds feature 4 c + g), register 1 = boacc (any lane)
          const float* sp = SL + (r < Hin ? 4 * 64 + 16 * (r & 3) + (r >> 2) : 5 * 64);
#pragma unroll
          for (int w = 0; w < NW; ++w) v += sp[(w * 2) * 4 * 64];
        }
        out[net.woff[l] + r * Hout + cc] = v;
      }
    }
  }
  float v0 = loss_var, v1 = loss_bc, v2 = loss_ic;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    v0 += __shfl_down(v0, o, 64);
    v1 += __shfl_down(v1, o, 64);
    v2 += __shfl_down(v2, o, 64);
  }
  __syncthreads();
  if (lane == 0) { sInt[wave * 3 + 0] = v0; sInt[wave * 3 + 1] = v1; sInt[wave * 3 + 2] = v2; }
  __syncthreads();
  if (tid < 3) {
    float s = 0.f;
    for (int w = 0; w < NW; ++w) s += sInt[w * 3 + tid];
    A.losspart[blockIdx.x * 3 + tid] = s;
  }
}

int pick_ks(int hmax) {
  if (hmax <= 20) return 5;
  if (hmax <= 32) return 8;
  if (hmax <= 50) return 13;      // NVE == 2: the edge k-step carries features 48, 49 only
  if (hmax <= 64) return 16;      // <= 63: the bias gradient rides in the row of (absent) feature 63; a 64-wide layer's
                                  // successor gets it from thin_bias
  return 0;
}

}  // namespace

int vn_fused16_ks(const VnNet& net) { return pick_ks(net.hmax); }

size_t vn_fused16_lds_bytes(const VnNet& net) {
  return visit_all(net, (size_t)0, [](auto I) { return (size_t)Lay<decltype(I)::L, decltype(I)::KS>::TOTAL * sizeof(float); });
}

size_t vn_fused16_stash_bytes(const VnNet& net) {
  return visit_all(net, (size_t)0, [](auto I) {
    using LY = Lay<decltype(I)::L, decltype(I)::KS>;
    return (size_t)LY::NSTG * LY::ST_LAYER * sizeof(float);
  });
}

bool vn_fused16_net_supported(const VnNet& net) {
  if (net.d_in > 4 * KS0) return false;
  const size_t b = vn_fused16_lds_bytes(net);
  return b != 0 && b <= 160 * 1024;
}

bool vn_fused16_supported(const VnNet& net, int integ_num) {
  if (integ_num < 1 || integ_num > TILE) return false;   // whole test functions must fit a tile
  return vn_fused16_net_supported(net);
}

hipError_t vn_fused16_launch(const VnFusedArgs& h, int grid, hipStream_t s) {
  VnFusedArgsD a;
  a.net = h.net; a.theta = h.theta; a.X = h.X; a.G = h.G; a.src = h.src; a.nT = h.nT; a.n_k = h.n_k;
  a.integ_num = h.integ_num; a.feN = h.feN; a.fedNt = h.fedNt; a.feW = h.feW; a.Nrow = h.Nrow; a.dNtrow = h.dNtrow; a.detJv = h.detJv;
  a.detJ = h.detJ; a.time_dependent = h.time_dependent; a.lossVec = h.lossVec; a.Xb = h.Xb;
  a.label = h.label; a.nB = h.nB; a.bDof = h.bDof; a.biDimVal = h.biDimVal; a.w0 = h.w0; a.w1 = h.w1;
  a.w2 = h.w2; a.partial = h.partial; a.losspart = h.losspart; a.stash = h.stash; a.stamps = h.stamps;
  a.mode = h.mode; a.dir = h.mode ? h.dir : -1; a.ostride = h.ostride; a.out_u = h.out_u; a.out_ud = h.out_ud;
  a.seed_u = h.seed_u; a.seed_ud = h.seed_ud;
  if (!h.stash && vn_fused16_stash_bytes(h.net) > 0) return hipErrorInvalidValue;
  return visit_all(h.net, hipErrorInvalidValue, [&](auto I) {
    using T = decltype(I);
    constexpr auto kernel = vn_fused16_kernel<T::L, T::KS, T::TANH>;
    constexpr size_t bytes = (size_t)Lay<T::L, T::KS>::TOTAL * sizeof(float);
    const hipError_t e = allow_lds_once<kernel>(bytes);            // the grid is the caller's
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NTHREADS), bytes, s, a);
    return hipGetLastError();
  });
}
