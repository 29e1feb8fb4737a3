// C-ABI host layer of libvarnet_hip.so (see include/varnet_hip.h for the contract and the
// reference call sites each entry point replaces).
#include "vn_internal.h"
#include "vn_ansatz.h"
#include "vn_dedup.h"
#include "vn_edge.h"
#include "vn_lbfgs.h"
#include "vn_obj64.h"
#include "vn_pgrad16.h"
#include "vn_taylor16.h"
#include "vn_terms.h"
#include "vn_learnt.h"
#include "vn_weights.h"
#include "vn_split16.h"
#include "vn_reparam.h"
#include "vn_balance.h"
#include "vn_adapt.h"
#include "vn_bicadapt.h"

hipError_t vn_calibrate_f64(int ncu, hipStream_t s, double ghz, double out[3]);      // vn_calib.hip (fp64 MFMA loop)

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl is dlopen'ed by vn_comm_*, never linked

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) return fail(VN_EHIP, "%s: %s", #expr, hipGetErrorString(e_));   \
  } while (0)

// (a failed call leaves earlier launches of the same step in flight: drain them before the caller unwinds)
#define LAYCHK(call)                                                          \
  do {                                                                        \
    char lerr_[384] = "";                                                      \
    (void)hipGetLastError();                                                  \
    if (call) {                                                               \
      (void)hipStreamSynchronize(h->stream);                                  \
      return fail(VN_EHIP, "layer-by-layer route: %s", lerr_);                \
    }                                                                         \
  } while (0)

// One polynomial term of a batch's PDE
struct Term {
  bool on = false;
  const float* stream = nullptr;   // [n_k*integ_num] per-row coefficient of the term, caller-owned
  double c[3] = {0.0, 0.0, 0.0};
};

// The streams of a hard-constraint ansatz u = A + B n on one row set (vn_ansatz.hip), caller-owned; B == nullptr: none registered.
// Rows: a = grad_x A . G_r, b = grad_x B . G_r, [rows]; the unique points of a map: a = grad_x A, b = grad_x B, [U, dim].
struct Ansatz {
  const float* A = nullptr;
  const float* B = nullptr;
  const float* a = nullptr;
  const float* b = nullptr;
};

// The self-adaptive weights of one batch (vn_set_tf_adapt): parameters, the double-buffered device state and its snapshot.
// f: 13 pieces of `stride` floats -- half 0 and half 1 as (lambda | omega | m1 | m2), the initial lambda, the snapshot's four;
// d: scalars of half 0, half 1 and the snapshot (VN_ADAPT_SCAL each), then the kernels' partials.
struct Adapt {
  int rule = VN_ADAPT_NONE, power = 2, normalize = 1;
  long every = 1;
  double par[10] = {};
  long n_k = 0, stride = 0;
  float* f = nullptr;
  double* d = nullptr;
  int cur = 0;                 // the committed half
  bool pending = false;        // the other half holds the update of a gradient evaluation that no optimizer step has committed
};

struct Batch {
  const float* Input = nullptr;
  const float* gcoef = nullptr;
  const float* source = nullptr;
  const float* sb_phi = nullptr;   // [sb_J, n_k*integ_num] basis streams of the source (vn_set_source_basis), caller-owned; nullptr: none
  int sb_J = 0;
  const float* fb_G = nullptr;     // [fb_J, n_k*integ_num, dim] basis streams of gcoef (vn_set_field_basis), caller-owned; nullptr: none
  int fb_J = 0;
  const float* detJv = nullptr;
  const float* Nrow = nullptr;
  const float* dNtrow = nullptr;
  long n_k = 0;
  double detJ = 0.0;
  bool set = false;
  // optional per-batch copy of the BC/IC rows (the reference's shuffle permutes them per feed: vn_set_batch_bic)
  const float* biInput = nullptr;
  const float* biLabel = nullptr;
  const float* bb_B = nullptr;     // [bb_J, nB] basis streams of that copy's labels (vn_set_bic_basis), caller-owned; nullptr: none
  int bb_J = 0;
  // de-duplicated formulation (vn_set_dedup)
  const float* Xu = nullptr;
  const int* uid = nullptr;   // (Xu is only ever set on the 8-wave routes: vn_set_dedup refuses the others)
  const int* rowptr = nullptr;
  const int* rowidx = nullptr;
  long U = 0;
  float* gcsr = nullptr;      // owned: gcoef in CSR order, [n_k*integ_num, dim] (static per batch; built by vn_set_dedup)
  long gcsr_cap = 0;
  bool gper = false;          // gcoef repeats with period integ_num along the rows (constant coefficients): no CSR copy needed
  // the polynomial terms (vn_terms.hip); as initialised here: not registered
  // reaction rate * (c1 u + c2 u^2 + c3 u^3) on the source side (vn_set_reaction); stream = rate, or nullptr: rate == 1
  Term react;
  // flux -div(w F(u)), F(u) = f1 u + f2 u^2 + f3 u^3, integrated by parts onto the test function (vn_set_nlflux);
  // stream = phi = sum_d w_d dN/dx_d per row
  Term nlflux;
  // diffusivity D(u) = d0 + d1 u + d2 u^2 of div(kappa D(u) grad u) (vn_set_nldiff); gcoef is then kappa dN/dx alone;
  // stream = psi = sum_d v_d dN/dx_d + N div v per row, or nullptr: no advection
  Term nldiff = {false, nullptr, {1.0, 0.0, 0.0}};
  // per-test-function loss weights (vn_weights.hip): static (vn_set_tf_weights) or causal (vn_set_causal); as initialised: none
  VnWeightsReg wt;
  int* wt_own = nullptr;      // owned: the causal registration's slab ids and CSR, one allocation (wt.slab / wt.sptr / wt.sidx)
  // self-adaptive weights (vn_set_tf_adapt, vn_adapt.hip), owned; while registered, wt.omega is its committed omega buffer
  Adapt* ad = nullptr;
  // hard-constraint ansatz (vn_ansatz.hip): the interior rows' streams (vn_set_ansatz) and those of the map's unique points
  // (vn_set_ansatz_points); as initialised here: none
  Ansatz az, azp;
};

inline bool has_terms(const Batch& b) { return b.react.on || b.nlflux.on || b.nldiff.on; }
inline bool has_weights(const Batch& b) { return vn_weights_on(b.wt); }
inline bool has_ansatz(const Batch& b) { return b.az.B != nullptr; }

// How an engine computes its gradient, decided once by pick_route (vn_create).
enum class Route {
  layered,    // layer by layer (vn_layered.hip): networks outside the kernels' range, or VN_KERNEL_LAYERED
  generic,    // generic forward / backward kernels (vn_generic.hip)
  fused4,     // 4-wave fused kernel (vn_fused.hip): the cross-check build only
  fused8,     // 8-wave fused kernel (vn_fused16.hip)
  twopass,    // 8-wave fused kernel twice around the row-wise seed kernel (integ_num > 128)
};

// vn_debug_point_route & 3: which kernels evaluate points (vn_forward*, vn_residual*, the de-duplicated unique points)
enum class PointRoute {
  automatic,  // 0 (and 3): the matrix-pipe kernels where the network has them
  per_thread, // 1: vn_residual / vn_*_f64 on the per-thread kernels (the tests' cross-check)
  f32_mfma,   // 2: the f32-MFMA point kernels where the bf16-piece kernels (vn_split16.hip) would run (cross-check build only)
};

constexpr int PROF_CAP = 4096;

#ifdef VN_WITH_FUSED32
constexpr bool kWithFused32 = true;
#else
constexpr bool kWithFused32 = false;
#endif
#ifdef VN_XCHECK_F32_POINT
constexpr bool kWithF32Point = true;     // cross-check build: vn_pgrad16 / vn_taylor16 also instantiated for the nets vn_split16 serves
#else
constexpr bool kWithF32Point = false;
#endif

// ---- learnt vectors: small vectors the Adam step moves next to the parameters ----------------
// One record per vector; what differs between the vectors is a row of kLearnt.  Everything that handles them (learnt_* below
// vn_engine) runs over the records in LearntId order.
enum LearntId { LV_COEF, LV_SRC, LV_FLD, LV_BIC, LV_FBC, LV_N };
constexpr int LV_CAP = VN_SRC_JMAX;              // the largest capacity of any kind (host staging arrays)

struct Learnt {
  bool on = false;
  int J = 0;                                      // entries in use (<= the kind's cap)
  unsigned long long mask = 0;                    // bit j: entry j is learnt
  double lr = 0.0;
  float* state = nullptr;                         // [6 * cap] (value | m | v) at stride cap, then their copy of vn_state_snapshot
  float* bounds = nullptr;                        // [2 * cap] (lo | hi) at stride cap
  double* grad = nullptr;                         // [cap] gradient of the last gradient evaluation
  float* part = nullptr;                          // [maxblk, J] partials of the reduction
  int blocks = 0;                                 // partials the current gradient evaluation wrote (0: the batch has nothing to reduce)
  // the prior of vn_set_learnt_prior (static: vn_state_snapshot has nothing to copy); all null / 0 without one
  double weight = 0.0;                            // alpha of the quadratic prior
  double* R = nullptr;                            // [J, J] its matrix; nullptr: the identity
  double* mean = nullptr;                         // [cap] its mean
  float* l1 = nullptr;                            // [cap] shrinkage weights; nullptr: none
  double* pen = nullptr;                          // [2] (Q, sum lambda |a|) of vn_get_learnt_prior
  struct Work { float* p = nullptr; long cap = 0; } work[3];   // the feature's own work buffers, by its *Work slot: allocated on
};                                                             // first use (lv_ensure), freed with the vector (learnt_free)
enum CoefWork { CW_ACC };                   // [3, U] accR_j, accF_j, gs_j of the de-duplicated step
enum SrcWork { SW_MIX };                    // [nT] s0 + sum_j a_j phi_j of the batch being evaluated
enum FldWork { FW_MIX, FW_CSR, FW_PACK };   // [nT, dim] g0 + sum_j b_j G_j of the batch being evaluated; the same in CSR order (de-duplicated
                                            // step), rebuilt every evaluation; [nT, 4] (u, grad u) of the batch's own rows (row-wise gradient)
enum BicWork { BW_MIX };                    // [nBreg] label0 + sum_j a_j B_j of the BC/IC set the batch being evaluated reads
enum FbcWork { XW_LABEL, XW_COEF };         // [nF] label0 + sum_{j < Jl} a_j S_j and [nF] coef0 + sum_{j >= Jl} a_j S_j of the flux rows

struct LearntKind {
  int cap;                    // capacity, and the stride of (value | m | v)
  int lanes;                  // lane-group width of the fp64 fold (VnLearntApplyArgs)
  const char* setter;         // the messages' nouns
  const char* noun;
  const char* what;
  const char* grads;
};
constexpr LearntKind kLearnt[LV_N] = {
  {VN_COEF_N, 16, "vn_set_coef_learn", "coefficient", "coefficients", "the nine coefficient gradients"},
  {VN_SRC_JMAX, 64, "vn_set_source_learn", "amplitude", "source amplitudes", "the amplitude gradients"},
  {VN_FLD_JMAX, 64, "vn_set_field_learn", "amplitude", "field amplitudes", "the amplitude gradients"},
  {VN_BIC_JMAX, 64, "vn_set_bic_learn", "amplitude", "boundary and initial amplitudes", "the amplitude gradients"},
  {VN_FBC_JMAX, 64, "vn_set_fluxbc_learn", "amplitude", "flux and Robin amplitudes", "the amplitude gradients"},
};

int learnt_weights_refusal(const LearntKind& k, int batch) {
  return fail(VN_EUNSUPPORTED, "learnt %s (%s) next to per-test-function loss weights (vn_set_tf_weights / vn_set_causal, batch %d): "
                               "the weights are applied after the seeds the %s reduction reads", k.what, k.setter, batch, k.noun);
}

// ---- edge row sets: rows the network is evaluated on beside a batch (vn_edge.h) ---------------
// One record per set, by VnEdgeId; what differs between the sets is a row of kEdge (below vn_engine) and the few fields the
// engine keeps beside the records.  Everything that handles them (edge_* below) runs over the records in VnEdgeId order.
enum EdgeBuf { EB_U, EB_UD, EB_UBAR, EB_UDBAR, EB_LOSS, EB_PARTIAL, EB_N };

struct EdgeSet {
  const float* X = nullptr;                       // caller-owned rows [rows, d_in]
  const float* G = nullptr;                       // caller-owned tangent directions [rows, dim]; nullptr: values only
  long rows = 0;                                  // rows the network sees
  long count = 0;                                 // rows, pairs or observations the mean divides by; 0: none registered
  int grid = 0;                                   // workgroups of the rows' reverse pass
  float* buf[EB_N] = {};                          // engine-owned: u, ud, ubar, udbar [rows], loss [seed blocks], partial [grid, P]
  long cap[EB_N] = {};
};

}  // namespace

#ifndef VN_WITH_FUSED32
// Product build: the 4-wave geometry (vn_fused.hip) is not linked -- it serves no automatic route (every network it takes is
// one of the 8-wave kernel's).  It lives in the tests' cross-check library (make xcheck: -DVN_WITH_FUSED32 + vn_fused.o).
bool vn_fused_supported(const VnNet&, int) { return false; }
hipError_t vn_fused_launch(const VnFusedArgs&, int, hipStream_t) { return hipErrorInvalidValue; }
#endif


struct vn_engine {
  vn_config cfg{};
  VnNet net{};
  hipStream_t stream = nullptr;
  int ncu = 256;

  float *theta = nullptr, *m = nullptr, *v = nullptr;
  double* theta64 = nullptr;
  float* gradbuf_int = nullptr;
  float* gradbuf = nullptr;
  float* lossbuf = nullptr;       // [4] for vn_eval_loss
  float* partial = nullptr;       // [partial_rows, P]; partial_rows = bwd_grid until an ansatz step appends its BC/IC rows' partials
  long partial_rows = 0;
  int bwd_grid = 0, fwd_grid = 0;

  float *feN = nullptr, *fedNt = nullptr, *feW = nullptr;
  bool has_fe = false, has_feW = false;

  std::vector<Batch> batches;
  const float *biInput = nullptr, *biLabel = nullptr;
  long nB = 0, bDof = 0;
  long nBreg = 0;                    // rows of vn_set_bic as the caller counts them (a steady engine keeps nB = bDof of them): the
                                     // length of a label stream and of every basis stream of vn_set_bic_basis
  const float* bicB = nullptr;       // [bicJ, nBreg] basis streams of the shared set's labels (vn_set_bic_basis), caller-owned
  int bicJ = 0;
  double biDimVal = 1.0;
  double w[3] = {1.0, 1.0, 1.0};

  float *u = nullptr, *ud = nullptr, *ubar = nullptr, *udbar = nullptr;
  long work_rows = 0;
  float *ub = nullptr, *ubar_b = nullptr;
  long work_b = 0;
  float* losspart = nullptr;
  long losspart_cap = 0;

  int64_t step = 0;
  Route route = Route::generic;
  bool full_grid = false;            // VN_FULL_GRID=1 (diagnostic): #CU workgroups whatever the tile count (fixed-cost measurements)
  VnOptArgs fuse;                    // optimizer step to fold into the next gradient reduction (kind -1: none)
  VnLayered* layered = nullptr;      // Route::layered
  float* tp_losspart = nullptr; long tp_losspart_cap = 0;
  float* fused_losspart = nullptr;   // [ncu*3]
  float* f16_stash = nullptr; long f16_stash_cap = 0;   // 8-wave kernel's weight-gradient stash (vn_fused16_stash_bytes per workgroup)
  unsigned long long* stamps = nullptr;   // 8 counters, diagnostic builds
  // de-duplicated formulation work buffers
  float *dd_uv = nullptr, *dd_su = nullptr, *dd_sg = nullptr, *dd_partial = nullptr, *dd_losspart = nullptr;
  long dd_uv_cap = 0, dd_su_cap = 0, dd_sg_cap = 0, dd_partial_cap = 0, dd_cap_lp = 0;
  bool feN_zero = false;      // the table of vn_set_fe_table has an entry N_p == 0 (the flux term's fold divides by N_p)
  float* rx_seff = nullptr; long rx_seff_cap = 0;   // the terms in the de-duplicated step: source + their shares per row (vn_terms.hip)
  float* nd_A = nullptr; long nd_A_cap = 0;         // quasilinear diffusion on the row-wise routes: sum_d u_{x_d} gcoef_d per row (vn_terms.hip)
  // loss weights (vn_weights.hip), allocated at the first registration: the loss field of a step whose caller passes none, omega_k
  // of the causal mode, and its slab statistics (doubles, sized in floats: lsum [S * chunks], then oslab [S])
  float* wt_lvec = nullptr; long wt_lvec_cap = 0;
  float* wt_omega = nullptr; long wt_omega_cap = 0;
  float* wt_stat = nullptr; long wt_stat_cap = 0;
  bool ad_quiet = false;       // vn_term_grads' probes: gradient evaluations that leave every adaptive state (vn_set_tf_adapt) alone
  // weights on the BC/IC rows (vn_set_bic_weights, vn_set_bic_adapt; vn_bicadapt.hip), owned, by part (0 bc, 1 ic): nullptr: the
  // part is unweighted.  A static registration is a state that never moves (rule VN_ADAPT_NONE, m(x) = x).  bw_field: the
  // unweighted loss field of both parts, the ic part's at vn_adapt_stride(bDof); allocated with the first registration
  Adapt* bw[2] = {nullptr, nullptr};
  float* bw_field = nullptr; long bw_field_cap = 0;
  // the edge row sets by VnEdgeId (es[id].count == 0: none registered), then what each kind keeps beside its record, caller-owned:
  // boundary-flux rows (vn_set_flux_bc), nF = count rows with their normals in G
  EdgeSet es[VN_EDGE_N];
  const float *fcoef = nullptr, *flabel = nullptr;
  double fbiDimVal = 1.0;
  const float* fbcS = nullptr;       // [fbcJl + fbcJc, nF] basis streams of the flux rows (vn_set_fluxbc_basis), caller-owned: fbcJl of
  int fbcJl = 0, fbcJc = 0;          // the flux datum (label), then fbcJc of the Robin coefficient (coef)
  // periodic pairs (vn_set_periodic): rows i and i + nP pair, nP = count, 2 nP rows; the directions in G while pgamma > 0
  double pgamma = 1.0, pbiDimVal = 1.0;
  // observations (vn_set_observations): n = rows points in nO = count segments
  const float *oQ = nullptr, *oval = nullptr, *owgt = nullptr;
  const int* orowptr = nullptr;
  double olambda = 0.0;
  double* omisfit = nullptr;                      // device slot: the unweighted misfit O of the last evaluation
  // hard-constraint ansatz (vn_set_ansatz_rows): the streams of the BC/IC rows and of the edge sets by VnEdgeId, caller-owned
  Ansatz az_bic, az_edge[VN_EDGE_N];
  // the vectors learnt next to the parameters, by LearntId: the nine coefficients of inverse mode (vn_set_coef_learn),
  // which live on the device while they are learnt, and the engine-wide amplitudes of the batches' source bases
  // (vn_set_source_learn) and gcoef bases (vn_set_field_learn), of the BC/IC label bases (vn_set_bic_learn) and of the flux rows'
  // bases (vn_set_fluxbc_learn), all of vn_learnt.hip; each carries its feature's own work buffers
  Learnt lv[LV_N];
  // learnt weight scales (vn_set_reparam, vn_reparam.hip): while rp.mode != 0, theta is theta_eff = f(s) (.) V and the optimizer
  // steps (V, s); every buffer below is allocated by the registration and freed when it is cleared
  struct Reparam {
    int mode = 0, gran = 0, S = 0;
    double n = 1.0, lr = 0.0;
    float* V = nullptr;              // [P]
    float* sc = nullptr;             // [4 S]: s | first-moment slot | second-moment slot | fl32(f(s)) as last formed
    float* snap = nullptr;           // [P + 4 S]: vn_state_snapshot's copy of V and sc
    float* gout = nullptr;           // [P + S]: g_V | g_s of vn_reparam_grad
    int* group = nullptr;            // [P] entry -> scale index, -1: in no group
    std::vector<float> s_init;       // what vn_params_init factorises with
    VnReparamArgs lay;               // mode, layer table and state pointers, filled once
  } rp;
  // per-term gradients (vn_term_grads, vn_term_stats; vn_balance.hip), allocated at the first call: the sums G_k, the statistics
  // kernels' partials, and the result slot -- stats [4][3] | gram [4][4] | value [4], read back in one copy
  float* tg_T = nullptr;       // [VN_TERM_N][P]
  double* tg_part = nullptr;   // [VN_BAL_MAX_BLOCKS][VN_BAL_ROW]
  double* tg_out = nullptr;    // [VN_BAL_OUT + VN_TERM_N]
  float* snap = nullptr;       // vn_state_snapshot: device copy of (theta | m | v), 3 P floats
  int64_t snap_step = -1;      // step counter at the snapshot (-1: none)
  PointRoute point_route = PointRoute::automatic;   // vn_debug_point_route(route & 3)
  bool eval_rowwise = false;   // vn_debug_point_route(route | 8): vn_eval_loss on the row-wise forward although the batch carries a de-duplication map
  bool no_gtable = false;      // vn_debug_point_route(route | 4): vn_set_dedup keeps the CSR-ordered copy of gcoef although it is periodic

  // VN_OPT_LBFGS (vn_lbfgs_step): device buffers allocated at the first call; what the host knows of the optimizer's state
  VnLbfgsBufs lb{};
  bool lb_alloc = false;
  bool lb_valid = false;       // (f_k, g_k) in lb.g_k belong to theta and to the objective as registered
  bool lb_reset = true;        // the ring is dropped before the next direction
  int32_t lb_batch = -1;
  double lb_f[4] = {0, 0, 0, 0};   // loss, BC, IC, var at theta_k
  double lb_w[3] = {0, 0, 0};      // loss weights (f_k, g_k) were evaluated with
  float* lb_lossh = nullptr;   // [4] pinned host floats: a trial's loss scalars
  bool lb_loss64 = false;      // vn_lbfgs_loss64: f_k and every trial's loss from the loss-only form of vn_objective_f64

  VnObj64Work o64{};           // vn_objective_f64: work buffers, allocated at the first call

  // tower gradient SUM over RCCL (vn_comm_init); nullptr = single process or host-side collective
  ncclComm_t comm = nullptr;
  int comm_world = 1, comm_rank = 0;
  // ncclCommInitRank has no timeout: a caller may run vn_comm_init on a helper thread and give up on it (vn_comm_abandon).
  // `comm` is committed / withdrawn under this mutex only, so the thread that trains never sees a communicator appear late.
  std::mutex comm_mu;
  bool comm_abandoned = false;
  ncclComm_t comm_orphan = nullptr;     // a communicator that came up after (or was up at) abandonment: never used, never destroyed

  // profiling of the dominant kernel
  bool prof_on = false;
  int prof_n = 0;
  std::vector<hipEvent_t> ev0, ev1;
  std::vector<hipEvent_t> cev0, cev1;   // around the all-reduce
  int cprof_n = 0;
  std::string prof_name = "vn_generic_bwd_kernel";
};

namespace {

int build_net(const vn_config& c, VnNet& net) {
  if (c.n_layers < 1 || c.n_layers > VN_MAX_LAYERS)
    return fail(VN_EINVAL, "n_layers=%d outside [1,%d]", c.n_layers, VN_MAX_LAYERS);
  if (c.d_in < 1 || c.d_in > VN_MAX_DIN) return fail(VN_EINVAL, "d_in=%d outside [1,%d]", c.d_in, VN_MAX_DIN);
  if (c.dim < 1 || c.dim > c.d_in) return fail(VN_EINVAL, "dim=%d must be in [1,d_in]", c.dim);
  if (c.integ_num < 1) return fail(VN_EINVAL, "integ_num must be positive");
  if (c.activation != VN_ACT_SIGMOID && c.activation != VN_ACT_TANH && c.activation != VN_ACT_PER_LAYER)
    return fail(VN_EUNSUPPORTED, "activation must be sigmoid or tanh (VarNet.py:97)");
  if (c.optimizer != VN_OPT_ADAM && c.optimizer != VN_OPT_RMSPROP && c.optimizer != VN_OPT_LBFGS)
    return fail(VN_EINVAL, "unknown optimizer requested!");
  if (c.optimizer != VN_OPT_LBFGS && c.lr < 0.0) return fail(VN_EINVAL, "learning rate must be positive!");  // TFModel.py:130
  if (c.optimizer == VN_OPT_ADAM) {
    // taken literally, never defaulted: a zero-initialised config (eps = 0: 0/0 in the update of a zero-gradient
    // parameter) is an error, not a NaN three steps later
    if (!(c.beta1 >= 0.0 && c.beta1 < 1.0) || !(c.beta2 >= 0.0 && c.beta2 < 1.0))
      return fail(VN_EINVAL, "Adam beta1 = %g, beta2 = %g must lie in [0, 1) (TF-1 defaults 0.9, 0.999; the struct is not defaulted)",
                  c.beta1, c.beta2);
    if (!(c.eps > 0.0))
      return fail(VN_EINVAL, "Adam epsilon = %g must be positive (TF-1 default 1e-8; the struct is not defaulted)", c.eps);
  }
  memset(&net, 0, sizeof net);
  net.d_in = c.d_in;
  net.dim = c.dim;
  net.L = c.n_layers;
  net.H[0] = c.d_in;
  int off = 0, hmax = 0;
  for (int l = 1; l <= net.L + 1; ++l) {
    const int h = (l <= net.L) ? c.widths[l - 1] : 1;
    if (h < 1 || h > VN_MAX_WIDTH) return fail(VN_EINVAL, "layer width %d outside [1,%d]", h, VN_MAX_WIDTH);
    net.H[l] = h;
    net.woff[l] = off;
    off += net.H[l - 1] * h;
    net.boff[l] = off;
    off += h;
    if (l <= net.L && h > hmax) hmax = h;
  }
  net.P = off;
  net.hmax = hmax;
  // per-layer list (TFModel.py:113-119): a list whose entries agree is the uniform case
  bool mixed = false;
  for (int l = 1; l <= net.L; ++l) {
    const int a = (c.activation == VN_ACT_PER_LAYER) ? c.layer_act[l - 1] : c.activation;
    if (a != VN_ACT_SIGMOID && a != VN_ACT_TANH) return fail(VN_EUNSUPPORTED, "activation must be sigmoid or tanh (VarNet.py:97)");
    net.actl[l] = a;
    if (a != net.actl[1]) mixed = true;
  }
  net.act = mixed ? VN_ACT_PER_LAYER : net.actl[1];
  return VN_OK;
}

// Networks outside the kernels' range (VN_KMAX_*), and nets whose generic-kernel tile does not fit LDS while no fused
// instantiation exists, go layer by layer (vn_layered.hip); VN_KERNEL_LAYERED forces that route.  One extension of the range:
// 7 and 8 hidden layers up to 50 wide are instantiated in the 8-wave fused kernel (deep, narrow nets); the generic kernels do
// not cover them, so every path of such an engine runs on the fused kernel.
int pick_route(const vn_config& c, const VnNet& net, Route* route) {
  const int k = c.kernel, q = c.integ_num;
  const bool generic_range = vn_net_in_kernel_range(net);
  const bool deep_fused = !generic_range && net.L <= 8 && net.hmax <= VN_KMAX_WIDTH && net.d_in <= VN_KMAX_DIN &&
                          net.act != VN_ACT_PER_LAYER && vn_fused16_net_supported(net) &&
                          (k == VN_KERNEL_AUTO || k == VN_KERNEL_FUSED16);
  const bool in_range = generic_range || deep_fused;
  if (!in_range && k != VN_KERNEL_AUTO && k != VN_KERNEL_LAYERED)
    return fail(VN_EUNSUPPORTED, "network (%d layers, widest %d, %d inputs%s) is outside the range of the requested kernel family "
                "(<= %d layers, width <= %d, <= %d inputs, one activation): use VN_KERNEL_AUTO or VN_KERNEL_LAYERED",
                net.L, net.hmax, net.d_in, net.act == VN_ACT_PER_LAYER ? ", mixed activations" : "", VN_KMAX_LAYERS,
                VN_KMAX_WIDTH, VN_KMAX_DIN);
  *route = Route::layered;
  if (k == VN_KERNEL_LAYERED || !in_range) return VN_OK;
  const bool fused_ok = k != VN_KERNEL_GENERIC && k != VN_KERNEL_FUSED && vn_fused16_net_supported(net);
  if (!fused_ok && vn_generic_bwd_lds_bytes(net) > 160 * 1024) {
    if (k == VN_KERNEL_AUTO) return VN_OK;
    return fail(VN_EUNSUPPORTED, "network needs %zu B of LDS per tile on the generic kernels (> 160 KiB): reduce depth/width",
                vn_generic_bwd_lds_bytes(net));
  }
  if (k == VN_KERNEL_FUSED && !vn_fused_supported(net, q))
    return fail(VN_EUNSUPPORTED, kWithFused32 ? "fused kernel unsupported for this network / integ_num"
                                              : "VN_KERNEL_FUSED (the 4-wave geometry) is not part of the product library: it lives in the "
                                                "tests' cross-check build, libvarnet_hip_xcheck.so (make -C varnet_amd/csrc xcheck)");
  const bool tp_ok = q > 128 && vn_fused16_net_supported(net);
  if (k == VN_KERNEL_FUSED16 && !vn_fused16_supported(net, q) && !tp_ok)
    return fail(VN_EUNSUPPORTED, "fused16 kernel unsupported for this network / integ_num");
  // AUTO: the 8-wave geometry where instantiated (faster: two waves per SIMD overlap VALU/LDS work with MFMA), else the 4-wave
  // geometry, else two-pass, else the generic kernels
  const bool eight = k == VN_KERNEL_FUSED16 || k == VN_KERNEL_AUTO;
  if (eight && vn_fused16_supported(net, q)) *route = Route::fused8;
  else if (k != VN_KERNEL_GENERIC && vn_fused_supported(net, q)) *route = Route::fused4;
  else if (eight && tp_ok) *route = Route::twopass;
  else *route = Route::generic;
  return VN_OK;
}

int ensure(float** p, long* cap, long need) {
  if (need <= *cap) return VN_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  HIPCHK(hipMalloc((void**)p, (size_t)need * sizeof(float)));
  *cap = need;
  return VN_OK;
}

// work buffer `slot` of learnt vector `id`: the pointer, and room for `need` floats
inline float* lv_work(const vn_engine* h, int id, int slot) { return h->lv[id].work[slot].p; }
int lv_ensure(vn_engine* h, int id, int slot, long need) { return ensure(&h->lv[id].work[slot].p, &h->lv[id].work[slot].cap, need); }

// What the mixes at the start of an evaluation end in, once the caller has found the rows' basis to be the engine's: work buffer `slot`
// of vector `id` = base + sum_{j < J} amp[first + j] stream_j over n entries (vn_learnt.hip)
int learnt_mix(vn_engine* h, int id, int slot, const float* base, const float* stream, int first, int J, long n) {
  if (n <= 0) return VN_OK;
  if (int rc = lv_ensure(h, id, slot, n)) return rc;
  VnMixArgs a{};
  a.base = base; a.stream = stream; a.amp = h->lv[id].state + first; a.J = J; a.n = n; a.out = lv_work(h, id, slot);
  HIPCHK(vn_learnt_mix_launch(a, h->stream));
  return VN_OK;
}

uint64_t splitmix64(uint64_t& s) {
  s += 0x9E3779B97F4A7C15ull;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int refresh_theta64(vn_engine* h) {
  // fp32 parameters widened on the host side of the stream: small, off the hot path
  std::vector<float> t(h->net.P);
  HIPCHK(hipMemcpyAsync(t.data(), h->theta, t.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::vector<double> d(t.begin(), t.end());
  if (!h->theta64) HIPCHK(hipMalloc((void**)&h->theta64, d.size() * sizeof(double)));
  HIPCHK(hipMemcpyAsync(h->theta64, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VN_OK;
}

int check_batch(vn_engine* h, int32_t batch) {
  if (batch < 0 || batch >= (int)h->batches.size() || !h->batches[batch].set)
    return fail(VN_ESTATE, "batch %d has no interior data (call vn_set_interior first)", batch);
  if (!h->has_fe && !(h->batches[batch].Nrow && h->batches[batch].dNtrow))
    return fail(VN_ESTATE, "FE tables missing (call vn_set_fe_table first)");
  return VN_OK;
}

inline const float* bi_x(const vn_engine* h, const Batch& b) { return b.biInput ? b.biInput : h->biInput; }
// the labels as registered, and the basis streams of the same set (the batch's own copy, else the shared one)
inline const float* bi_y0(const vn_engine* h, const Batch& b) { return b.biLabel ? b.biLabel : h->biLabel; }
inline const float* bic_basis(const vn_engine* h, const Batch& b) { return b.biLabel ? b.bb_B : h->bicB; }
inline int bic_basis_J(const vn_engine* h, const Batch& b) { return b.biLabel ? b.bb_J : h->bicJ; }
// (while boundary / initial amplitudes are learnt, a batch whose set has a basis reads the mixed labels bic_mix formed at the start
// of the evaluation: every launch site takes its labels from here)
inline bool bic_learnt(const vn_engine* h, const Batch& b) { return h->lv[LV_BIC].on && bic_basis(h, b); }
inline const float* bi_y(const vn_engine* h, const Batch& b) { return bic_learnt(h, b) ? lv_work(h, LV_BIC, BW_MIX) : bi_y0(h, b); }
// (while amplitudes are learnt, a batch with a basis reads the mixed stream source_mix formed at the start of the evaluation)
inline bool src_learnt(const vn_engine* h, const Batch& b) { return h->lv[LV_SRC].on && b.sb_phi; }
inline const float* batch_src(const vn_engine* h, const Batch& b) {
  return !h->cfg.has_source ? nullptr : src_learnt(h, b) ? lv_work(h, LV_SRC, SW_MIX) : b.source;
}
// (... and the mixed direction field_mix formed there in place of the batch's gcoef)
inline bool fld_learnt(const vn_engine* h, const Batch& b) { return h->lv[LV_FLD].on && b.fb_G; }
inline const float* batch_gcoef(const vn_engine* h, const Batch& b) { return fld_learnt(h, b) ? lv_work(h, LV_FLD, FW_MIX) : b.gcoef; }
inline const float* fe_w(const vn_engine* h) { return (h->cfg.has_integw && h->has_feW) ? h->feW : nullptr; }

inline bool on_8wave(const vn_engine* h) { return h->route == Route::fused8 || h->route == Route::twopass; }

// VN_OPT_LBFGS: the objective or the iterate changed behind the optimizer's back -- (f_k, g_k) are stale, the ring is dropped
inline void lbfgs_invalidate(vn_engine* h) { h->lb_valid = false; h->lb_reset = true; }
inline void lbfgs_invalidate(vn_engine* h, int32_t batch) { if (batch == h->lb_batch) lbfgs_invalidate(h); }
inline bool is_lbfgs(const vn_engine* h) { return h->cfg.optimizer == VN_OPT_LBFGS; }
#define NOT_LBFGS(name)                                                                                              \
  if (is_lbfgs(h)) return fail(VN_ESTATE, name " is a first-order optimizer step: an L-BFGS engine (VN_OPT_LBFGS) advances by vn_lbfgs_step only")

// ---- point kernels of the 8-wave family (vn_debug_point_route) ----------------------------
// hidden widths 33..64: the products as six bf16-piece MFMAs, fp32-class (vn_split16.hip), unless route 2 asks for f32-MFMA
inline bool use_split16(const vn_engine* h) { return h->point_route != PointRoute::f32_mfma && vn_split16_supported(h->net); }

// (u, grad u) at n points, the outputs of vn_pgrad16_launch; with neither g nor pack, the value-only sweep (F_pt per point)
hipError_t point_pass(const vn_engine* h, const float* X, long n, float* u, float* g, float* pack) {
  if (!use_split16(h)) return vn_pgrad16_launch(h->net, h->theta, X, n, u, g, pack, h->ncu, 0, h->stream);
  if (!g && !pack) return vn_split16_forward(h->net, h->theta, X, n, u, h->ncu, h->stream);
  return vn_split16_pgrad(h->net, h->theta, X, n, u, g, pack, h->ncu, h->stream);
}

// Strong residual in f32.  Networks of the 8-wave family: second-order forward mode on the matrix pipe (vn_split16.hip or
// vn_taylor16.hip); the per-point kernel keeps the generic / 4-wave requests (and is what the new kernels are cross-checked against)
hipError_t residual_f32(const vn_engine* h, const float* X, const float* diff, const float* vel, const float* src, const float* ddx,
                        long n, float* u, float* res) {
  const int td = h->cfg.time_dependent;
  if (on_8wave(h) && h->point_route != PointRoute::per_thread && vn_taylor16_supported(h->net, td)) {
    if (use_split16(h)) return vn_split16_residual(h->net, h->theta, X, diff, vel, src, ddx, td, n, u, res, h->ncu, h->stream);
    return vn_taylor16_residual(h->net, h->theta, X, diff, vel, src, ddx, td, n, u, res, h->ncu, h->stream);
  }
  return vn_pointwise_residual_f32(h->net, h->theta, X, diff, vel, src, ddx, td, n, u, res, h->stream);
}

// fp64 points (vn_forward_f64, vn_residual_f64): networks of the 8-wave family whose fp64 images fit the LDS on the fp64 matrix
// pipe (vn_taylor16d.hip), else per thread
inline bool use_taylor16d(const vn_engine* h) {
  return on_8wave(h) && h->point_route != PointRoute::per_thread && vn_taylor16d_supported(h->net);
}

// ---- vn_profile_*: HIP events around the region of a step that prof_name is charged with ---
// (prof_n moves in prof_stop only, so both ends of a region see the same slot)
int prof_start(vn_engine* h) {
  if (!h->prof_on || h->prof_n >= PROF_CAP) return VN_OK;
  if (!h->ev0[h->prof_n]) { HIPCHK(hipEventCreate(&h->ev0[h->prof_n])); HIPCHK(hipEventCreate(&h->ev1[h->prof_n])); }
  HIPCHK(hipEventRecord(h->ev0[h->prof_n], h->stream));
  return VN_OK;
}

int prof_stop(vn_engine* h) {
  if (!h->prof_on || h->prof_n >= PROF_CAP) return VN_OK;
  HIPCHK(hipEventRecord(h->ev1[h->prof_n], h->stream));
  h->prof_n++;
  return VN_OK;
}

// A checker kernel's count of violations in one device int, zeroed before and read back after it (synchronises: registration only)
template <class Launch>
int count_on_device(vn_engine* h, Launch launch, int* count) {
  int* err_dev = nullptr;
  HIPCHK(hipMalloc((void**)&err_dev, sizeof(int)));
  hipError_t e = hipMemsetAsync(err_dev, 0, sizeof(int), h->stream);
  if (e == hipSuccess) e = launch(err_dev);
  *count = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(count, err_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(err_dev);
  if (e != hipSuccess) return fail(VN_EHIP, "vn_set_dedup: %s", hipGetErrorString(e));
  return VN_OK;
}

// ---- kernel arguments shared by every launch site; callers set rows, mode, outputs, seeds and partial buffers ----
// Fused kernels: with a batch, also its BC/IC rows, bDof, biDimVal and the loss weights; without one (the forward-only mode on
// arbitrary rows) those stay zero.
VnFusedArgs fused_args(const vn_engine* h, const Batch* b) {
  VnFusedArgs f{};
  f.net = h->net; f.theta = h->theta; f.integ_num = h->cfg.integ_num;
  f.feN = h->feN; f.fedNt = h->fedNt; f.time_dependent = h->cfg.time_dependent;
  if (b) {
    f.Xb = bi_x(h, *b); f.label = bi_y(h, *b); f.nB = h->nB; f.bDof = h->bDof; f.biDimVal = (float)h->biDimVal;
    f.w0 = (float)h->w[0]; f.w1 = (float)h->w[1]; f.w2 = (float)h->w[2];
  }
  return f;
}

// Row-wise seed kernel: the batch's interior rows (values in h->u, h->ud) and the BC/IC rows (values in h->ub)
VnSeedArgs seed_args(const vn_engine* h, const Batch& b) {
  VnSeedArgs a{};
  a.u = h->u; a.ud = h->ud; a.source = batch_src(h, b);
  a.feN = h->feN; a.fedNt = h->fedNt; a.feW = fe_w(h);
  a.Nrow = b.Nrow; a.dNtrow = b.dNtrow; a.detJv = b.detJv; a.detJ = (float)b.detJ;
  a.n_k = b.n_k; a.integ_num = h->cfg.integ_num; a.time_dependent = h->cfg.time_dependent;
  a.ub = h->ub; a.label = bi_y(h, b); a.nB = h->nB; a.bDof = h->bDof; a.biDimVal = (float)h->biDimVal;
  a.w0 = (float)h->w[0]; a.w1 = (float)h->w[1]; a.w2 = (float)h->w[2];
  if (b.react.on) { a.react = 1; a.rate = b.react.stream; a.c1 = (float)b.react.c[0]; a.c2 = (float)b.react.c[1]; a.c3 = (float)b.react.c[2]; }
  if (b.react.on && h->lv[LV_COEF].on) a.coef = h->lv[LV_COEF].state;
  return a;
}

// De-duplicated assembly (seed and gather kernels) of a batch with a de-duplication map, (u, grad u) of its points in h->dd_uv
VnDedupArgs dedup_args(const vn_engine* h, const Batch& b) {
  VnDedupArgs a{};
  a.upack = h->dd_uv; a.uid = b.uid; a.rowptr = b.rowptr; a.rowidx = b.rowidx;
  // (learnt field amplitudes: gcoef moves every step, so no periodic table, and the CSR copy is the one field_mix rebuilt)
  const bool fld = fld_learnt(h, b);
  a.gcoef = batch_gcoef(h, b); a.gcoef_csr = fld ? lv_work(h, LV_FLD, FW_CSR) : b.gcsr; a.source = batch_src(h, b);
  a.feN = h->feN; a.fedNt = h->fedNt; a.feW = fe_w(h);
  a.detJv = b.detJv; a.detJ = (float)b.detJ; a.n_k = b.n_k; a.U = b.U; a.q = h->cfg.integ_num; a.dim = h->cfg.dim;
  a.time_dependent = h->cfg.time_dependent; a.w2 = (float)h->w[2]; a.gper = b.gper && !fld ? 1 : 0;
  return a;
}

// ---- the polynomial terms of a batch (vn_terms.hip): what the messages call each, and the four stages that know their order ----
struct TermKind {
  Term Batch::*slot;
  const char* name;         // "the <name> is not built for ..."
  const char* coefs;        // "<coefs> coefficients"
  const char* integrand;    // "no <integrand> to integrate"
  bool by_Np;               // its share of the de-duplicated source divides by N_p
};
const TermKind kReact{&Batch::react, "reaction term", "reaction", "reaction term", false};
const TermKind kNlflux{&Batch::nlflux, "flux term", "flux", "flux term", true};
const TermKind kNldiff{&Batch::nldiff, "diffusivity D(u)", "diffusivity", "diffusion term", true};
const TermKind* const kTerms[] = {&kReact, &kNlflux, &kNldiff};

// A term that divides by N_p cannot join a de-duplication map while the table of vn_set_fe_table has a zero entry: an error code at
// registration (`how`: what the call cannot do for batch `batch`) and, since the table may change afterwards, in the steps
int check_Np(const vn_engine* h, const TermKind& k, int batch = -1, const char* how = nullptr) {
  if (!k.by_Np || !h->feN_zero) return VN_OK;
  if (how) return fail(VN_EUNSUPPORTED, "the %s of batch %d %s: vn_set_fe_table has an entry N_p == 0", k.name, batch, how);
  return fail(VN_EUNSUPPORTED, "the %s of a de-duplicated batch needs test-function values N_p != 0 at every quadrature "
                               "point (vn_set_fe_table has a zero entry); clear the map (vn_set_dedup with Xu = NULL) to run row-wise", k.name);
}

// Inverse mode: where a registered term of b reads its three coefficients (nullptr: learning off, the batch's own by value)
const float* term_cp(const vn_engine* h, const Batch& b, const Term& t) {
  if (!h->lv[LV_COEF].on) return nullptr;
  return h->lv[LV_COEF].state + 3 * (&t == &b.react ? 0 : &t == &b.nlflux ? 1 : 2);
}

// Row-wise routes: values in h->u, integrand / seeds in h->ud, h->ubar, h->udbar, A_r of the D(u) pair saved in h->nd_A
VnTermRowArgs term_row_args(const vn_engine* h, const Batch& b, const Term& t) {
  VnTermRowArgs a{};
  a.u = h->u; a.stream = t.stream;
  for (int i = 0; i < 3; ++i) a.c[i] = (float)t.c[i];
  a.cp = term_cp(h, b, t);
  a.nT = b.n_k * h->cfg.integ_num;
  a.ud = h->ud; a.A = h->nd_A; a.udbar = h->udbar; a.ubar = h->ubar;
  return a;
}

// Before vn_seed_launch: D(u) turns ud = A into D(u) A - u psi before anything else edits it, then -F(u) phi joins it
int terms_fold_rows(vn_engine* h, const Batch& b) {
  if (b.nldiff.on) {
    if (int rc = ensure(&h->nd_A, &h->nd_A_cap, b.n_k * h->cfg.integ_num)) return rc;
    HIPCHK(vn_nldiff_fold_launch(term_row_args(h, b, b.nldiff), h->stream));
  }
  if (b.nlflux.on) HIPCHK(vn_nlflux_fold_launch(term_row_args(h, b, b.nlflux), h->stream));
  return VN_OK;
}

// After a vn_seed_launch that produced seeds: D(u) rescales the tangent seed last, the flux term's value seed reads it unscaled
int terms_seed_rows(vn_engine* h, const Batch& b) {
  if (src_learnt(h, b)) {                          // source identification: the amplitude sums read udbar before D(u) rescales it
    VnSrcGradArgs g{};
    g.udbar = h->udbar; g.Nrow = b.Nrow; g.feN = h->feN; g.phi = b.sb_phi; g.J = b.sb_J;
    g.nT = b.n_k * h->cfg.integ_num; g.q = h->cfg.integ_num; g.mask = h->lv[LV_SRC].mask; g.part = h->lv[LV_SRC].part;
    HIPCHK(vn_srcgrad_rows_launch(g, &h->lv[LV_SRC].blocks, h->stream));
  }
  if (h->lv[LV_COEF].on && has_terms(b)) {   // inverse mode: the coefficient sums read udbar before D(u) rescales it
    VnCoefRowsArgs c{};
    c.u = h->u; c.udbar = h->udbar; c.nT = b.n_k * h->cfg.integ_num; c.q = h->cfg.integ_num;
    c.react = b.react.on ? 1 : 0; c.rate = b.react.stream; c.Nrow = b.Nrow; c.feN = h->feN;
    c.phi = b.nlflux.on ? b.nlflux.stream : nullptr; c.A = b.nldiff.on ? h->nd_A : nullptr;
    c.mask = h->lv[LV_COEF].mask; c.part = h->lv[LV_COEF].part;
    HIPCHK(vn_coefgrad_rows_launch(c, &h->lv[LV_COEF].blocks, h->stream));
  }
  if (b.nlflux.on) HIPCHK(vn_nlflux_seed_launch(term_row_args(h, b, b.nlflux), h->stream));
  if (b.nldiff.on) HIPCHK(vn_nldiff_seed_launch(term_row_args(h, b, b.nldiff), h->stream));
  if (fld_learnt(h, b)) {                          // field identification: the amplitude sums read udbar as D(u) left it, and the
    const long nT = b.n_k * h->cfg.integ_num;      // second tangent grad u_r of a point pass over the batch's own rows
    if (int rc = lv_ensure(h, LV_FLD, FW_PACK, 4 * nT)) return rc;
    float* pack = lv_work(h, LV_FLD, FW_PACK);
    HIPCHK(point_pass(h, b.Input, nT, nullptr, nullptr, pack));
    VnFldGradArgs g{};
    g.udbar = h->udbar; g.pack = pack; g.G = b.fb_G; g.J = b.fb_J; g.dim = h->cfg.dim;
    g.nT = nT; g.q = h->cfg.integ_num; g.mask = h->lv[LV_FLD].mask; g.part = h->lv[LV_FLD].part;
    HIPCHK(vn_fldgrad_rows_launch(g, &h->lv[LV_FLD].blocks, h->stream));
  }
  return VN_OK;
}

// De-duplicated step: the values of the batch's points in h->dd_uv; source so far, test-function seeds and point seeds as in d
VnTermDedupArgs term_dedup_args(const vn_engine* h, const Batch& b, const Term& t, const VnDedupArgs& d) {
  VnTermDedupArgs a{};
  a.upack = h->dd_uv; a.uid = b.uid; a.rowptr = b.rowptr; a.rowidx = b.rowidx;
  a.base = d.source; a.stream = t.stream;
  for (int i = 0; i < 3; ++i) a.c[i] = (float)t.c[i];
  a.cp = term_cp(h, b, t);
  a.feN = h->feN; a.feW = fe_w(h); a.stf = d.stf;
  a.nT = b.n_k * h->cfg.integ_num; a.U = b.U; a.q = h->cfg.integ_num;
  a.s_eff = h->rx_seff; a.seed_u = d.seed_u;
  return a;
}

// ... of D(u), which alone reads gcoef and the points' tangent seeds
VnTermDedupArgs nldiff_dedup_args(const vn_engine* h, const Batch& b, const VnDedupArgs& d) {
  VnTermDedupArgs a = term_dedup_args(h, b, b.nldiff, d);
  a.gcoef = batch_gcoef(h, b); a.dim = h->cfg.dim; a.gper = b.gper && !fld_learnt(h, b) ? 1 : 0; a.seed_g = d.seed_g;
  return a;
}

// Before vn_dedup_seed_launch, which takes d.source: source + rate p(u) per row takes the place of the source, F(u) phi / N_p comes
// on top of it, ((1 - D(u)) A + u psi) / N_p on top of both -- each in h->rx_seff, on what the previous one left there
int terms_source_dedup(vn_engine* h, const Batch& b, VnDedupArgs& d) {
  if (!has_terms(b)) return VN_OK;
  for (const TermKind* k : kTerms)
    if ((b.*(k->slot)).on)
      if (int rc = check_Np(h, *k)) return rc;
  if (int rc = ensure(&h->rx_seff, &h->rx_seff_cap, b.n_k * h->cfg.integ_num)) return rc;
  if (b.react.on) { HIPCHK(vn_react_source_launch(term_dedup_args(h, b, b.react, d), h->stream)); d.source = h->rx_seff; }
  if (b.nlflux.on) { HIPCHK(vn_nlflux_source_launch(term_dedup_args(h, b, b.nlflux, d), h->stream)); d.source = h->rx_seff; }
  if (b.nldiff.on) { HIPCHK(vn_nldiff_source_launch(nldiff_dedup_args(h, b, d), h->stream)); d.source = h->rx_seff; }
  return VN_OK;
}

// After vn_dedup_gather_launch: each term's value seed, added to the gathered one; D(u) last (D'(u) grad u . seed_g needs the
// unscaled seed_g)
int terms_gather_dedup(vn_engine* h, const Batch& b, const VnDedupArgs& d) {
  if (h->lv[LV_COEF].on && has_terms(b)) {   // inverse mode: each kernel also stores its per-point sum for vn_coefgrad_points_kernel
    if (int rc = lv_ensure(h, LV_COEF, CW_ACC, 3 * b.U)) return rc;
    float* acc = lv_work(h, LV_COEF, CW_ACC);
    VnTermDedupArgs r = term_dedup_args(h, b, b.react, d), f = term_dedup_args(h, b, b.nlflux, d), n = nldiff_dedup_args(h, b, d);
    r.acc_out = acc; f.acc_out = acc + b.U; n.acc_out = acc + 2 * b.U;
    if (b.react.on) HIPCHK(vn_react_gather_launch(r, h->stream));
    if (b.nlflux.on) HIPCHK(vn_nlflux_gather_launch(f, h->stream));
    if (b.nldiff.on) HIPCHK(vn_nldiff_point_launch(n, h->stream));
    VnCoefPointsArgs c{};
    c.upack = h->dd_uv; c.U = b.U; c.mask = h->lv[LV_COEF].mask; c.part = h->lv[LV_COEF].part;
    c.accR = b.react.on ? r.acc_out : nullptr; c.accF = b.nlflux.on ? f.acc_out : nullptr; c.gs = b.nldiff.on ? n.acc_out : nullptr;
    HIPCHK(vn_coefgrad_points_launch(c, &h->lv[LV_COEF].blocks, h->stream));
    return VN_OK;
  }
  if (b.react.on) HIPCHK(vn_react_gather_launch(term_dedup_args(h, b, b.react, d), h->stream));
  if (b.nlflux.on) HIPCHK(vn_nlflux_gather_launch(term_dedup_args(h, b, b.nlflux, d), h->stream));
  if (b.nldiff.on) HIPCHK(vn_nldiff_point_launch(nldiff_dedup_args(h, b, d), h->stream));
  return VN_OK;
}

// ---- per-test-function loss weights (vn_weights.hip) ----
constexpr long kWtStat = 2L * VN_WEIGHTS_MAX_SLABS * (VN_WEIGHTS_MAX_CHUNKS + 1);   // floats that hold lsum and oslab at their largest

inline VnWeightsWork weights_work(const vn_engine* h) {
  VnWeightsWork wk;
  wk.lsum = reinterpret_cast<double*>(h->wt_stat);
  wk.oslab = wk.lsum + (long)VN_WEIGHTS_MAX_SLABS * VN_WEIGHTS_MAX_CHUNKS;
  return wk;
}

// Where a seed kernel writes the batch's loss field: the caller's array, else the engine's own when the weights need one
inline float* weights_lossvec(const vn_engine* h, const Batch& b, float* lossVec) {
  return lossVec || !has_weights(b) ? lossVec : h->wt_lvec;
}

// ---- self-adaptive weights (vn_adapt.hip): the state of a batch, double-buffered ----
inline VnAdaptState adapt_half(const Adapt& ad, int piece0, int scal) {
  VnAdaptState s;
  float* f = ad.f + (long)piece0 * ad.stride;
  s.lambda = f; s.omega = f + ad.stride;
  if (ad.rule == VN_ADAPT_SA) { s.m1 = f + 2 * ad.stride; s.m2 = f + 3 * ad.stride; }
  s.scal = ad.d + (long)scal * VN_ADAPT_SCAL;
  return s;
}
inline VnAdaptState adapt_state(const Adapt& ad, int half) { return adapt_half(ad, 4 * half, half); }
inline VnAdaptState adapt_snap(const Adapt& ad) { return adapt_half(ad, 9, 2); }
inline float* adapt_lambda0(const Adapt& ad) { return ad.f + 8 * ad.stride; }
constexpr long kAdaptPieces = 13;
constexpr long kAdaptDoubles = 3L * VN_ADAPT_SCAL + 6L * VN_ADAPT_MAX_BLOCKS;

VnAdaptArgs adapt_args(const Adapt& ad, int rule, int from, int to) {
  VnAdaptArgs a;
  a.rule = rule; a.power = ad.power; a.normalize = ad.normalize; a.n_k = ad.n_k;
  if (ad.rule == VN_ADAPT_RBA) { a.gamma = (float)ad.par[0]; a.eta = (float)ad.par[1]; }
  else { a.lr = ad.par[0]; a.cap = (float)ad.par[1]; a.beta1 = ad.par[2]; a.beta2 = ad.par[3]; a.eps = ad.par[4]; }
  a.cur = adapt_state(ad, from); a.next = adapt_state(ad, to);
  a.part = ad.d + 3L * VN_ADAPT_SCAL;
  return a;
}

// The index of the step a gradient evaluation belongs to: steps completed before it (the folded step has counted itself already)
inline int64_t adapt_step_index(const vn_engine* h) { return h->step - (h->fuse.kind >= 0 ? 1 : 0); }

// omega, Z and the statistics of the committed half rebuilt from its lambda (in place); nothing is pending afterwards
int adapt_rebuild(vn_engine* h, Adapt& ad) {
  HIPCHK(vn_adapt_update_launch(adapt_args(ad, VN_ADAPT_NONE, ad.cur, ad.cur), h->stream));
  ad.pending = false;
  return VN_OK;
}

// Back to the registered initial state: lambda = its initial values, slots and tau zero
int adapt_reset(vn_engine* h, Adapt& ad) {
  const VnAdaptState s = adapt_state(ad, ad.cur);
  const size_t nb = (size_t)ad.n_k * sizeof(float);
  HIPCHK(hipMemcpyAsync(s.lambda, adapt_lambda0(ad), nb, hipMemcpyDeviceToDevice, h->stream));
  if (s.m1) HIPCHK(hipMemsetAsync(s.m1, 0, 2 * (size_t)ad.stride * sizeof(float), h->stream));
  HIPCHK(hipMemsetAsync(s.scal, 0, VN_ADAPT_SCAL * sizeof(double), h->stream));
  return adapt_rebuild(h, ad);
}

// Every state registered on the engine, in the order vn_state_export lays them out: each batch's (vn_set_tf_adapt) in batch
// order, then the bc part's, then the ic part's (vn_set_bic_weights, vn_set_bic_adapt).  A further holder is appended here.
// f(Adapt&) returns an error code; the first that is not VN_OK ends the walk and is returned.
template <class F>
int adapt_each(const vn_engine* h, F f) {
  for (const Batch& b : h->batches)
    if (b.ad)
      if (int rc = f(*b.ad)) return rc;
  for (Adapt* ad : h->bw)
    if (ad)
      if (int rc = f(*ad)) return rc;
  return VN_OK;
}

// Batch::wt.omega of every adaptive batch is its state's committed omega: called wherever a state is installed or `cur` may move
void adapt_point_omega(vn_engine* h) {
  for (Batch& b : h->batches)
    if (b.ad) b.wt.omega = adapt_state(*b.ad, b.ad->cur).omega;
}

// The optimizer step's share: every pending state becomes the committed one -- the halves swap, nothing is copied
void adapt_commit(vn_engine* h) {
  adapt_each(h, [](Adapt& ad) -> int {
    if (ad.pending) { ad.cur ^= 1; ad.pending = false; }
    return VN_OK;
  });
  adapt_point_omega(h);
}
void adapt_drop_pending(vn_engine* h) {
  adapt_each(h, [](Adapt& ad) -> int { ad.pending = false; return VN_OK; });
}

// The committed half into the snapshot (back = false) or the snapshot into the committed half; then nothing is pending
int adapt_snap_copy(vn_engine* h, Adapt& ad, bool back) {
  const VnAdaptState s = adapt_state(ad, ad.cur), t = adapt_snap(ad);
  const VnAdaptState &dst = back ? s : t, &src = back ? t : s;
  HIPCHK(hipMemcpyAsync(dst.lambda, src.lambda, 4 * (size_t)ad.stride * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dst.scal, src.scal, VN_ADAPT_SCAL * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  if (back) ad.pending = false;
  return VN_OK;
}

// A state in vn_state_export's bytes: the scalars, then lambda, omega[, m1, m2] of n_k floats each.  adapt_bytes: its size;
// adapt_host_copy: the committed half to the cursor p (vn_state_export) or from it (load: vn_state_import; then nothing is
// pending), and p moves past the state
inline int64_t adapt_bytes(const Adapt& ad) {
  return (int64_t)(VN_ADAPT_SCAL * sizeof(double)) + (int64_t)(ad.rule == VN_ADAPT_SA ? 4 : 2) * ad.n_k * (int64_t)sizeof(float);
}
int adapt_host_copy(vn_engine* h, Adapt& ad, char*& p, bool load) {
  const VnAdaptState s = adapt_state(ad, ad.cur);
  auto copy = [&](void* dev, size_t nb) {
    char* host = p;
    p += nb;
    return load ? hipMemcpyAsync(dev, host, nb, hipMemcpyHostToDevice, h->stream) : hipMemcpyAsync(host, dev, nb, hipMemcpyDeviceToHost, h->stream);
  };
  HIPCHK(copy(s.scal, VN_ADAPT_SCAL * sizeof(double)));
  for (float* piece : {s.lambda, s.omega, s.m1, s.m2})
    if (piece) HIPCHK(copy(piece, (size_t)ad.n_k * sizeof(float)));
  if (load) ad.pending = false;
  return VN_OK;
}

// After the seed kernel and every term's seed kernel: [causal: the weights from lossVec], stf scaled (de-duplicated step),
// the var loss partials of the seed kernel's blocks (tfb test functions each) replaced, the rows' seeds scaled (row-wise routes)
int weights_stage(vn_engine* h, const Batch& b, const float* lossVec, int tfb, float* stf, float* part, bool rows) {
  if (!has_weights(b)) return VN_OK;
  // self-adaptive weights: a gradient evaluation (the only caller with seeds to scale) also forms the pending state from its
  // own loss field; it reads the committed half and writes the other, so the weights applied below are the committed ones
  if (b.ad && (rows || stf) && !h->ad_quiet && adapt_step_index(h) % b.ad->every == 0) {
    VnAdaptArgs a = adapt_args(*b.ad, b.ad->rule, b.ad->cur, b.ad->cur ^ 1);
    a.lossVec = lossVec;
    HIPCHK(vn_adapt_update_launch(a, h->stream));
    b.ad->pending = true;
  }
  const bool causal = b.wt.S > 0;
  HIPCHK(vn_weights_apply_f32(b.wt, weights_work(h), lossVec, b.n_k, tfb, causal ? h->wt_omega : nullptr, stf, part, h->stream));
  if (rows)
    HIPCHK(vn_weights_rows_f32(causal ? h->wt_omega : b.wt.omega, b.n_k, h->cfg.integ_num, h->ubar, h->udbar, h->stream));
  return VN_OK;
}

void adapt_free(Adapt*& ad) {
  if (!ad) return;
  if (ad->f) (void)hipFree(ad->f);
  if (ad->d) (void)hipFree(ad->d);
  delete ad;
  ad = nullptr;
}

void clear_weights(Batch& b) {
  if (b.wt_own) (void)hipFree(b.wt_own);
  b.wt_own = nullptr;
  adapt_free(b.ad);
  b.wt = VnWeightsReg();
}

// ---- hard-constraint ansatz u = A + B n (vn_ansatz.hip): the stages, in the order that file's header fixes ----
// Fold of one row set right after its forward: (v, vd) = (n, nd) -> (u, ud); vd nullptr: a values-only set
int ansatz_fold(vn_engine* h, const Ansatz& z, float* v, float* vd, long n) {
  VnAnsatzRowArgs r{};
  r.A = z.A; r.B = z.B; r.a = vd ? z.a : nullptr; r.b = vd ? z.b : nullptr; r.n = n; r.v = v; r.vd = vd;
  HIPCHK(vn_ansatz_fold_launch(r, h->stream));
  return VN_OK;
}

// Adjoint of one row set, last before its reverse pass: (v, vd) = (ubar, udbar) -> the seeds of (n, nd)
int ansatz_adjoint(vn_engine* h, const Ansatz& z, float* v, float* vd, long n) {
  VnAnsatzRowArgs r{};
  r.B = z.B; r.b = vd ? z.b : nullptr; r.n = n; r.v = v; r.vd = vd;
  HIPCHK(vn_ansatz_adjoint_launch(r, h->stream));
  return VN_OK;
}

// The unique points of b's map: the record h->dd_uv after point_pass (fold), the gathered seeds (adjoint)
VnAnsatzPointArgs ansatz_point_args(const vn_engine* h, const Batch& b) {
  VnAnsatzPointArgs p{};
  p.A = b.azp.A; p.B = b.azp.B; p.gA = b.azp.a; p.gB = b.azp.b; p.U = b.U; p.dim = h->cfg.dim;
  p.pack = h->dd_uv; p.seed_u = h->dd_su; p.seed_g = h->dd_sg;
  return p;
}

// The routes that carry the stage: the generic kernels serve the BC/IC rows of every ansatz step and the edge sets
int ansatz_check_route(const vn_engine* h) {
  if (h->route == Route::fused4)
    return fail(VN_EUNSUPPORTED, "a hard-constraint ansatz is not built for VN_KERNEL_FUSED (the 4-wave cross-check geometry): its "
                                 "single launch forms the BC/IC seeds itself; the generic and the 8-wave families carry it");
  if (h->route != Route::layered && vn_net_in_kernel_range(h->net)) return VN_OK;
  return fail(VN_EUNSUPPORTED, "a hard-constraint ansatz needs a network of the hand-written kernels (<= %d hidden layers, width <= %d, "
              "<= %d inputs, one activation); this one (%d layers, widest %d, %d inputs%s) runs on the layer-by-layer route "
              "or the deep fused kernel only", VN_KMAX_LAYERS, VN_KMAX_WIDTH, VN_KMAX_DIN, h->net.L, h->net.hmax,
              h->net.d_in, h->net.act == VN_ACT_PER_LAYER ? ", mixed activations" : "");
}

// Non-finite entries of the streams of a registration, counted on the device (synchronises: registration only)
int ansatz_check_finite(vn_engine* h, const char* who, const Ansatz& z, long n, long nd) {
  int bad = 0;
  auto check = [&](int* err_dev) {
    hipError_t e = vn_ansatz_check_launch(z.A, n, err_dev, h->stream);
    if (e == hipSuccess) e = vn_ansatz_check_launch(z.B, n, err_dev, h->stream);
    if (e == hipSuccess) e = vn_ansatz_check_launch(z.a, nd, err_dev, h->stream);
    if (e == hipSuccess) e = vn_ansatz_check_launch(z.b, nd, err_dev, h->stream);
    return e;
  };
  if (int rc = count_on_device(h, check, &bad)) return rc;
  if (bad) return fail(VN_EINVAL, "%s: %d non-finite entr%s in the ansatz streams", who, bad, bad == 1 ? "y" : "ies");
  return VN_OK;
}

const char* const kAnsatzSet[] = {"the BC/IC rows (VN_ANSATZ_BIC)", "the boundary-flux rows (VN_ANSATZ_FLUX)",
                                  "the periodic pairs (VN_ANSATZ_PERIODIC)", "the observations (VN_ANSATZ_OBS)"};

// Before every evaluation of batch b: all of its row sets carry the map, or none does.  Without any registration: one pass over
// five pointers, nothing else.
int ansatz_check_eval(const vn_engine* h, const Batch& b, int batch) {
  const bool on = has_ansatz(b);
  const Ansatz* sets[1 + VN_EDGE_N] = {&h->az_bic, &h->az_edge[0], &h->az_edge[1], &h->az_edge[2]};
  const long rows[1 + VN_EDGE_N] = {h->nB, h->es[0].count, h->es[1].count, h->es[2].count};
  for (int i = 0; i < 1 + VN_EDGE_N; ++i) {
    const bool reg = rows[i] > 0, has = sets[i]->B != nullptr;
    if (on && reg && !has)
      return fail(VN_ESTATE, "batch %d has a hard-constraint ansatz (vn_set_ansatz) but %s have no ansatz streams (vn_set_ansatz_rows): "
                             "they would be evaluated on the bare network output", batch, kAnsatzSet[i]);
    if (!on && has)
      return fail(VN_ESTATE, "%s have ansatz streams (vn_set_ansatz_rows) but batch %d has no ansatz (vn_set_ansatz): its interior rows "
                             "would be evaluated on the bare network output", kAnsatzSet[i], batch);
  }
  if (!on) return VN_OK;
  if (b.Xu && !b.azp.B)
    return fail(VN_ESTATE, "batch %d has a de-duplication map and a hard-constraint ansatz but no ansatz streams at the map's unique "
                           "points (vn_set_ansatz_points)", batch);
  if (b.biInput && h->az_bic.B)
    return fail(VN_EUNSUPPORTED, "batch %d has its own copy of the BC/IC rows (vn_set_batch_bic) next to BC/IC ansatz streams "
                                 "(vn_set_ansatz_rows), which belong to the rows of vn_set_bic", batch);
  return VN_OK;
}

// The BC/IC rows of an ansatz step on the 8-wave sequences.  The seeded reverse launch forms their seeds from n - label, which
// cannot express B (A + B n - label), so they leave it (f.nB = 0) for the generic kernels in the order run_generic shows: forward,
// fold, the row-wise seed kernel with an empty interior set, ubar_b *= B_b, reverse pass -- gradient partials to `partial`
// ([*nparts, P] on return), loss partials to `lp` ([*nlp, 3]).
// h->partial with room for `rows` partials (an ansatz step of the two-pass sequence appends its BC/IC rows' to the launch's own)
int grow_partial(vn_engine* h, long rows) {
  if (rows <= h->partial_rows) return VN_OK;
  float* p = nullptr;
  HIPCHK(hipMalloc((void**)&p, (size_t)rows * h->net.P * sizeof(float)));
  (void)hipFree(h->partial);                         // (waits for the launches in flight)
  h->partial = p; h->partial_rows = rows;
  return VN_OK;
}

inline int ansatz_bic_lossparts(const vn_engine* h) { return h->nB > 0 ? (int)((h->nB + 255) / 256) : 0; }
inline int ansatz_bic_parts(const vn_engine* h) {               // workgroups of the rows' reverse pass, as edge_alloc sizes a set's
  const long tiles = (h->nB + 31) / 32;
  return (int)(tiles < h->ncu ? tiles : h->ncu);
}

int ansatz_bic_rows(vn_engine* h, const Batch& b, float* partial, float* lp, int* nparts, int* nlp) {
  *nparts = 0; *nlp = 0;
  if (h->nB <= 0) return VN_OK;
  VnRows r{}, none{};
  r.X = bi_x(h, b); r.G = nullptr; r.u = h->ub; r.ud = nullptr; r.n = h->nB;
  HIPCHK(vn_generic_forward(h->net, h->theta, r, none, h->fwd_grid, h->stream));
  if (int rc = ansatz_fold(h, h->az_bic, h->ub, nullptr, h->nB)) return rc;
  VnSeedArgs s = seed_args(h, b);
  s.n_k = 0; s.source = nullptr; s.feW = nullptr; s.react = 0;   // interior set empty: the BC/IC terms alone
  s.ubar_b = h->ubar_b; s.part = lp;
  const int bgrid = ansatz_bic_lossparts(h);
  HIPCHK(vn_seed_launch(s, bgrid, h->stream));
  if (int rc = ansatz_adjoint(h, h->az_bic, h->ubar_b, nullptr, h->nB)) return rc;
  r.u = nullptr; r.ubar = h->ubar_b; r.udbar = nullptr;
  const int grid = ansatz_bic_parts(h);
  HIPCHK(vn_generic_backward(h->net, h->theta, r, none, partial, grid, h->stream));
  *nparts = grid; *nlp = bgrid;
  return VN_OK;
}

// ---- weights on the BC/IC rows (vn_set_bic_weights, vn_set_bic_adapt; vn_bicadapt.hip) ----
// While a part is registered, the rows leave the step's main launch (nB = 0 there), whose seeds know no omega, and run as a pass
// of their own, as under an ansatz: a forward of the rows, the rows' seed kernel, the generic reverse pass.
inline bool bicw_on(const vn_engine* h) { return h->bw[0] || h->bw[1]; }
inline long bicw_count(const vn_engine* h, int part) { return part == 0 ? h->bDof : h->nB - h->bDof; }
inline float* bicw_field(const vn_engine* h, int part) { return h->bw_field + (part ? vn_adapt_stride(h->bDof) : 0); }
inline int bicw_lossparts(const vn_engine* h) { return bicw_on(h) ? vn_bic_rows_blocks(h->nB) : 0; }
inline int bicw_parts(const vn_engine* h) { return bicw_on(h) ? ansatz_bic_parts(h) : 0; }

const LearntKind* learnt_any(const vn_engine* h);
int fused_forward(vn_engine* h, const float* X, const float* G, long n, float* out_u, float* out_ud);

// What cannot stand next to a registration, checked by the registration and again before every evaluation (so that it holds in
// both orders of registration)
int bicw_check(const vn_engine* h, const char* who) {
  if (h->az_bic.B)
    return fail(VN_EUNSUPPORTED, "%s next to BC/IC ansatz streams (vn_set_ansatz_rows): under a hard-constraint ansatz the rows' error is "
                                 "zero by construction, there is nothing to weight", who);
  if (const LearntKind* k = learnt_any(h))
    return fail(VN_EUNSUPPORTED, "%s next to learnt %s (%s): the %s sums next to the rows' own pass are not built (and learnt boundary "
                                 "data would move the labels the weights follow)", who, k->what, k->setter, k->noun);
  if (h->comm)
    return fail(VN_EUNSUPPORTED, "%s under a communicator: a rank's max, mean and Z would follow its own shard's steps, so the ranks "
                                 "together would train another objective than one rank", who);
  for (size_t i = 0; i < h->batches.size(); ++i)
    if (h->batches[i].biInput)
      return fail(VN_EUNSUPPORTED, "%s next to batch %zu's own copy of the BC/IC rows (vn_set_batch_bic): the weights belong to the rows "
                                   "of vn_set_bic, one state per row", who, i);
  return VN_OK;
}

// The rows' seed kernel on the values in h->ub: loss field, loss partials to lp, with_seeds the weighted seeds to h->ubar_b; and
// in a gradient evaluation that is no probe, the pending state of every adaptive part from its own loss field (the committed half is
// read, the other written: the weights applied are the committed ones)
int bicw_seed(vn_engine* h, const Batch& b, float* lp, bool with_seeds) {
  VnBicRowsArgs a;
  a.ub = h->ub; a.label = bi_y(h, b); a.nB = h->nB; a.bDof = h->bDof;
  a.biDimVal = (float)h->biDimVal; a.w0 = (float)h->w[0]; a.w1 = (float)h->w[1];
  for (int s = 0; s < 2; ++s) {
    a.omega[s] = h->bw[s] ? adapt_state(*h->bw[s], h->bw[s]->cur).omega : nullptr;
    a.field[s] = bicw_count(h, s) > 0 ? bicw_field(h, s) : nullptr;
  }
  a.ubar_b = with_seeds ? h->ubar_b : nullptr; a.part = lp;
  HIPCHK(vn_bic_rows_launch(a, h->stream));
  if (!with_seeds || h->ad_quiet) return VN_OK;
  for (int s = 0; s < 2; ++s) {
    Adapt* ad = h->bw[s];
    if (!ad || ad->rule == VN_ADAPT_NONE || adapt_step_index(h) % ad->every != 0) continue;
    VnAdaptArgs u = adapt_args(*ad, ad->rule, ad->cur, ad->cur ^ 1);
    u.lossVec = bicw_field(h, s);
    HIPCHK(vn_adapt_update_launch(u, h->stream));
    ad->pending = true;
  }
  return VN_OK;
}

// The rows' pass of a gradient evaluation on the 8-wave sequences: gradient partials to `partial` ([*nparts, P] on return), loss
// partials to `lp` ([*nlp, 3])
int bicw_rows(vn_engine* h, const Batch& b, float* partial, float* lp, int* nparts, int* nlp) {
  *nparts = 0; *nlp = 0;
  if (h->nB <= 0) return VN_OK;
  VnRows r{}, none{};
  r.X = bi_x(h, b); r.G = nullptr; r.u = h->ub; r.ud = nullptr; r.n = h->nB;
  if (on_8wave(h)) {                                 // the 8-wave kernel's forward-only mode: the faster of the two (DESIGN.md section
    if (int rc = fused_forward(h, r.X, nullptr, r.n, r.u, nullptr)) return rc;   // 35); it borrows h->partial's first rows, which
  } else {                                                                       // the step's own launch writes afterwards
    HIPCHK(vn_generic_forward(h->net, h->theta, r, none, h->fwd_grid, h->stream));
  }
  if (int rc = bicw_seed(h, b, lp, true)) return rc;
  r.u = nullptr; r.ubar = h->ubar_b; r.udbar = nullptr;
  const int grid = bicw_parts(h);
  HIPCHK(vn_generic_backward(h->net, h->theta, r, none, partial, grid, h->stream));
  *nparts = grid; *nlp = bicw_lossparts(h);
  return VN_OK;
}

// Every launch of the 8-wave fused kernel: its global-memory stash (per workgroup; none for most instantiations) is sized here
int fused8_launch(vn_engine* h, VnFusedArgs& f, int grid) {
  const long per = (long)(vn_fused16_stash_bytes(h->net) / sizeof(float));
  if (per > 0) {
    if (int rc = ensure(&h->f16_stash, &h->f16_stash_cap, per * grid)) return rc;
    f.stash = h->f16_stash;
  }
  HIPCHK(vn_fused16_launch(f, grid, h->stream));
  return VN_OK;
}

// Model value (and directional derivative along G, if given) at n rows with the 8-wave fused kernel in its
// forward-only mode: 2 F_pt per row at the fused kernel's efficiency instead of the generic forward kernel.
int fused_forward(vn_engine* h, const float* X, const float* G, long n, float* out_u, float* out_ud) {
  if (n <= 0) return VN_OK;
  VnFusedArgs f = fused_args(h, nullptr);
  f.X = X; f.G = G; f.nT = n;
  f.partial = h->partial; f.losspart = h->fused_losspart;
  f.mode = 1; f.dir = G ? -1 : 0; f.ostride = 1; f.out_u = out_u; f.out_ud = G ? out_ud : nullptr;
  if (!f.losspart || !f.partial) return fail(VN_ESTATE, "fused forward without its work buffers");   // the kernel stores to both
  const long tiles = (n + 127) / 128;
  const int grid = (int)(tiles < h->ncu ? tiles : h->ncu);
  if (int rc = fused8_launch(h, f, grid)) return rc;
  return VN_OK;
}

// Boundary / initial amplitudes: the amplitude sums over the BC/IC rows, whose values are in h->ub (vn_learnt.hip)
int bic_reduce(vn_engine* h, const Batch& b) {
  if (!bic_learnt(h, b) || h->nB <= 0) return VN_OK;
  VnBicGradArgs g{};
  g.ub = h->ub; g.label = bi_y(h, b); g.B = bic_basis(h, b); g.J = bic_basis_J(h, b);
  g.nB = h->nBreg; g.bDof = h->bDof; g.steady = h->cfg.time_dependent ? 0 : 1;
  g.biDimVal = (float)h->biDimVal; g.w0 = (float)h->w[0]; g.w1 = (float)h->w[1];
  g.mask = h->lv[LV_BIC].mask; g.part = h->lv[LV_BIC].part;
  HIPCHK(vn_bicgrad_launch(g, &h->lv[LV_BIC].blocks, h->stream));
  return VN_OK;
}

// ... on the routes whose reverse pass carries the BC/IC tiles and leaves no values of those rows behind (the single launch, the
// two-pass sequence, the de-duplicated step): one forward of the rows first.  Enqueued ahead of the step's own launches: it
// borrows the work buffers the step's reduction reads, and that reduction may fold the parameters' update in.
int bic_forward_reduce(vn_engine* h, const Batch& b) {
  if (!bic_learnt(h, b) || h->nB <= 0) return VN_OK;
  if (int rc = fused_forward(h, bi_x(h, b), nullptr, h->nB, h->ub, nullptr)) return rc;
  return bic_reduce(h, b);
}

// Flux and Robin amplitudes: while they are learnt and the flux rows have a basis, the part that has streams reads the values
// fluxbc_mix formed at the start of the evaluation; else the caller's arrays.  The two read sites (flux_seed, vn_objective_f64)
// take their coefficient and label from here.
inline bool fbc_learnt(const vn_engine* h) { return h->lv[LV_FBC].on && h->fbcS; }
inline const float* flux_coef(const vn_engine* h) { return fbc_learnt(h) && h->fbcJc > 0 ? lv_work(h, LV_FBC, XW_COEF) : h->fcoef; }
inline const float* flux_label(const vn_engine* h) { return fbc_learnt(h) && h->fbcJl > 0 ? lv_work(h, LV_FBC, XW_LABEL) : h->flabel; }

// ... first thing in an evaluation: the basis must be the engine's, then the label and the coefficient are formed, one mix per
// part that has streams (vn_learnt.hip)
int fluxbc_mix(vn_engine* h) {
  if (!fbc_learnt(h)) return VN_OK;
  const Learnt& v = h->lv[LV_FBC];
  const long nF = h->es[VN_EDGE_FLUX].count;
  if (h->fbcJl + h->fbcJc != v.J)
    return fail(VN_EINVAL, "the flux rows have a basis of %d + %d streams, the learnt amplitudes (vn_set_fluxbc_learn) are %d", h->fbcJl,
                h->fbcJc, v.J);
  if (h->fbcJl > 0)
    if (int rc = learnt_mix(h, LV_FBC, XW_LABEL, h->flabel, h->fbcS, 0, h->fbcJl, nF)) return rc;
  if (h->fbcJc > 0)
    if (int rc = learnt_mix(h, LV_FBC, XW_COEF, h->fcoef, h->fbcS + (long)h->fbcJl * nF, h->fbcJl, h->fbcJc, nF)) return rc;
  return VN_OK;
}

// ... and after the flux set's edge pass of a gradient evaluation: the amplitude sums over its values and seeds
int fluxbc_reduce(vn_engine* h) {
  if (!fbc_learnt(h)) return VN_OK;
  const EdgeSet& e = h->es[VN_EDGE_FLUX];
  VnFbcGradArgs g{};
  g.u = e.buf[EB_U]; g.udbar = e.buf[EB_UDBAR]; g.S = h->fbcS; g.J = h->fbcJl + h->fbcJc; g.Jl = h->fbcJl; g.nF = e.count;
  g.mask = h->lv[LV_FBC].mask; g.part = h->lv[LV_FBC].part;
  HIPCHK(vn_fbcgrad_launch(g, &h->lv[LV_FBC].blocks, h->stream));
  return VN_OK;
}

// ---- edge row sets (vn_edge.h) ------------------------------------------------------------------
// The seed kernel of each kind: from the values in e.buf[EB_U] and the tangent stream ud (nullptr: values only) the loss
// partials in e.buf[EB_LOSS] and, where asked for, the seeds ubar and udbar (nullptr: loss only / values only).
hipError_t flux_seed(const vn_engine* h, const EdgeSet& e, const float* ud, float* ubar, float* udbar) {
  VnFluxSeedArgs a{};
  a.u = e.buf[EB_U]; a.ud = ud; a.coef = flux_coef(h); a.label = flux_label(h); a.nF = e.count;
  a.biDimVal = (float)h->fbiDimVal; a.w0 = (float)h->w[0];
  a.ubar = ubar; a.udbar = udbar; a.part = e.buf[EB_LOSS];
  return vn_flux_seed_launch(a, h->stream);
}

hipError_t periodic_seed(const vn_engine* h, const EdgeSet& e, const float* ud, float* ubar, float* udbar) {
  VnPeriodicSeedArgs a{};
  a.u = e.buf[EB_U]; a.ud = ud; a.nP = e.count; a.gamma = (float)h->pgamma;
  a.biDimVal = (float)h->pbiDimVal; a.w0 = (float)h->w[0];
  a.ubar = ubar; a.udbar = udbar; a.part = e.buf[EB_LOSS];
  return vn_periodic_seed_launch(a, h->stream);
}

hipError_t obs_seed(const vn_engine* h, const EdgeSet& e, const float* ud, float* ubar, float* udbar) {
  VnObsSeedArgs a{};
  a.u = e.buf[EB_U]; a.ud = ud; a.q = h->oQ; a.rowptr = h->orowptr; a.value = h->oval; a.wgt = h->owgt;
  a.nO = e.count; a.lambda = (float)h->olambda;
  a.ubar = ubar; a.udbar = udbar; a.part = e.buf[EB_LOSS];
  return vn_obs_seed_launch(a, h->stream);
}

struct EdgeKind {
  const char* noun;           // the subject of the refusal message
  hipError_t (*seed)(const vn_engine*, const EdgeSet&, const float* ud, float* ubar, float* udbar);
};
constexpr EdgeKind kEdge[VN_EDGE_N] = {
  {"boundary-flux rows", flux_seed},
  {"periodic boundary pairs", periodic_seed},
  {"observations", obs_seed},
};

// One set, on every route: value and derivative G . grad_x u of each of its rows (the generic forward kernel with the set's
// directions as tangents; none registered: the value stream only), the kind's residuals with their loss partials and seeds,
// and with_grad the generic reverse pass into the set's own partials -- launches of the set's own, so a step without it is
// untouched.  Everything reads theta before the step's reduction (which may fold the update in); *sum is what that reduction
// adds.  Nothing registered: nothing is enqueued.
int edge_pass(vn_engine* h, int id, bool with_grad, VnEdgeSum* sum) {
  *sum = VnEdgeSum();
  const EdgeSet& e = h->es[id];
  if (e.count <= 0) return VN_OK;
  const bool deriv = e.G != nullptr;
  VnRows r{}, none{};
  r.X = e.X; r.G = e.G; r.u = e.buf[EB_U]; r.ud = deriv ? e.buf[EB_UD] : nullptr; r.n = e.rows;
  HIPCHK(vn_generic_forward(h->net, h->theta, r, none, h->fwd_grid, h->stream));
  const Ansatz& z = h->az_edge[id];                  // hard-constraint ansatz: the seed kernel sees u = A + B n and its derivative
  if (z.B)
    if (int rc = ansatz_fold(h, z, r.u, r.ud, e.rows)) return rc;
  float* ubar = with_grad ? e.buf[EB_UBAR] : nullptr;
  float* udbar = with_grad && deriv ? e.buf[EB_UDBAR] : nullptr;
  HIPCHK(kEdge[id].seed(h, e, r.ud, ubar, udbar));
  if (with_grad && z.B)
    if (int rc = ansatz_adjoint(h, z, ubar, udbar, e.rows)) return rc;
  if (with_grad) {
    r.u = nullptr; r.ud = nullptr; r.ubar = ubar; r.udbar = udbar;
    HIPCHK(vn_generic_backward(h->net, h->theta, r, none, e.buf[EB_PARTIAL], e.grid, h->stream));
    sum->partial = e.buf[EB_PARTIAL]; sum->nparts = e.grid;
  }
  sum->loss = e.buf[EB_LOSS]; sum->nlp = vn_edge_seed_blocks(e.count); sum->count = e.count;
  return VN_OK;
}

// The edge passes of a step in VnEdgeId order: what its reduction adds.
int edge_passes(vn_engine* h, bool with_grad, VnEdgeSums* fx) {
  for (int id = 0; id < VN_EDGE_N; ++id) {
    if (int rc = edge_pass(h, id, with_grad, &fx->set[id])) return rc;
    if (id == VN_EDGE_FLUX && with_grad)
      if (int rc = fluxbc_reduce(h)) return rc;      // flux and Robin amplitudes: u and udbar of the flux rows are in the set's buffers
  }
  if (h->es[VN_EDGE_OBS].count > 0) { fx->lambda = (float)h->olambda; fx->misfit = h->omisfit; }
  return VN_OK;
}

// Registration, step 1: a call replaces the previous registration, also when it fails.
void edge_drop(vn_engine* h, int id) {
  EdgeSet& e = h->es[id];
  e.X = e.G = nullptr;
  lbfgs_invalidate(h);
  e.count = e.rows = 0;
  h->az_edge[id] = Ansatz();                         // the rows' ansatz streams go with them (vn_set_ansatz_rows)
}

// Step 2, after the call's own argument checks: the edge passes run on the generic kernels, whatever route the interior term takes.
int edge_check_route(const vn_engine* h, int id) {
  if (h->route != Route::layered && vn_net_in_kernel_range(h->net)) return VN_OK;
  return fail(VN_EUNSUPPORTED, "%s need a network of the hand-written kernels (<= %d hidden layers, width <= %d, "
              "<= %d inputs, one activation); this one (%d layers, widest %d, %d inputs%s) runs on the layer-by-layer route "
              "or the deep fused kernel only", kEdge[id].noun, VN_KMAX_LAYERS, VN_KMAX_WIDTH, VN_KMAX_DIN, h->net.L, h->net.hmax,
              h->net.d_in, h->net.act == VN_ACT_PER_LAYER ? ", mixed activations" : "");
}

// Step 3: the reverse grid and the work buffers of `rows` rows and `count` seed threads (deriv: a direction is in play -- else no
// tangent stream, no derivative seed).  The set stays unregistered until the caller sets X, G and count.
int edge_alloc(vn_engine* h, int id, long rows, long count, bool deriv) {
  EdgeSet& e = h->es[id];
  const long tiles = (rows + 31) / 32;
  e.rows = rows;
  e.grid = (int)(tiles < h->ncu ? tiles : h->ncu);
  const long need[EB_N] = {rows, deriv ? rows : 0, rows, deriv ? rows : 0, vn_edge_seed_blocks(count), (long)e.grid * h->net.P};
  for (int b : {EB_U, EB_UBAR, EB_UD, EB_UDBAR, EB_LOSS, EB_PARTIAL})
    if (int rc = ensure(&e.buf[b], &e.cap[b], need[b])) return rc;
  return VN_OK;
}

// Loss components and loss field of a batch that carries a de-duplication map (vn_set_dedup), without the row-wise forward: (u, grad u)
// once per unique point (2 F_pt per POINT where the forward-only mode of the fused kernel costs 2 F_pt per ROW), the assembly kernel of
// the training step in its loss-only form (R_k, lossVec, variational partials), the BC/IC rows through the forward-only mode and the
// row-wise seed kernel with an empty interior set.  What every monitor of a run on the de-duplicated formulation calls (splitLoss,
// VarNet.py:1365): 2.9 -> 0.45 ms on BASELINE config 3.
int eval_dedup(vn_engine* h, const Batch& b, float* lossVec, float* lossdst, const VnEdgeSums& fx) {
  const int sblk = (int)((b.n_k + VN_DEDUP_TFB - 1) / VN_DEDUP_TFB);
  const int bgrid = (int)(((h->nB > 0 ? h->nB : 1) + 255) / 256);
  if (int rc = ensure(&h->losspart, &h->losspart_cap, (long)(sblk + bgrid) * 3)) return rc;
  HIPCHK(point_pass(h, b.Xu, b.U, nullptr, nullptr, h->dd_uv));
  if (has_ansatz(b)) HIPCHK(vn_ansatz_points_fold_launch(ansatz_point_args(h, b), h->stream));
  VnDedupArgs a = dedup_args(h, b);
  a.lossVec = weights_lossvec(h, b, lossVec); a.part = h->losspart;          // loss only: no seeds
  if (int rc = terms_source_dedup(h, b, a)) return rc;
  HIPCHK(vn_dedup_seed_launch(a, sblk, h->stream));
  if (int rc = weights_stage(h, b, a.lossVec, VN_DEDUP_TFB, nullptr, a.part, false)) return rc;
  if (int rc = fused_forward(h, bi_x(h, b), nullptr, h->nB, h->ub, nullptr)) return rc;
  if (has_ansatz(b))
    if (int rc = ansatz_fold(h, h->az_bic, h->ub, nullptr, h->nB)) return rc;
  VnSeedArgs s = seed_args(h, b);
  // interior set empty: the BC/IC terms alone (Nrow, dNtrow and detJv are nullptr on a batch with a de-duplication map)
  s.n_k = 0; s.source = nullptr; s.feW = nullptr;
  s.part = h->losspart + (long)sblk * 3;
  if (bicw_on(h)) {                                  // weighted rows: their own seed kernel in its loss-only form (bgrid blocks as well)
    if (int rc = bicw_seed(h, b, s.part, false)) return rc;
  } else {
    HIPCHK(vn_seed_launch(s, bgrid, h->stream));
  }
  if (lossdst)
    HIPCHK(vn_reduce_launch(nullptr, 0, 0, h->losspart, sblk + bgrid, h->bDof, h->nB, s.w0, s.w1, s.w2, lossdst, h->stream,
                            VnOptArgs(), fx));
  return VN_OK;
}

// forward + weak-form epilogue; with_seeds = also produce backward seeds.  fx: the flux rows' and the periodic pairs' loss, folded
// into lossdst.
int run_forward_and_seed(vn_engine* h, const Batch& b, bool with_seeds, float* lossVec, float* lossdst,
                         const VnEdgeSums& fx = VnEdgeSums()) {
  if (!with_seeds && b.Xu && h->has_fe && !h->eval_rowwise) return eval_dedup(h, b, lossVec, lossdst, fx);
  VnRows s0{}, s1{};
  s0.X = b.Input; s0.G = batch_gcoef(h, b); s0.u = h->u; s0.ud = h->ud; s0.n = b.n_k * h->cfg.integ_num;
  s1.X = bi_x(h, b); s1.G = nullptr; s1.u = h->ub; s1.ud = nullptr; s1.n = h->nB;
  if (h->route == Route::layered) {
    LAYCHK(vn_layered_forward(h->layered, h->theta, s0, h->stream, lerr_, sizeof lerr_, with_seeds ? 0 : -1));
    LAYCHK(vn_layered_forward(h->layered, h->theta, s1, h->stream, lerr_, sizeof lerr_, with_seeds ? 1 : -1));
  } else if ((on_8wave(h) && h->has_fe && !with_seeds) || !vn_net_in_kernel_range(h->net)) {
    // splitLoss / trainWeight / the monitors: the fused kernel's forward-only mode for both row sets (and every forward of a
    // 7-8 hidden layer net, which the generic kernels do not cover)
    if (int rc = fused_forward(h, s0.X, s0.G, s0.n, s0.u, s0.ud)) return rc;
    if (int rc = fused_forward(h, s1.X, nullptr, s1.n, s1.u, nullptr)) return rc;
  } else {
    HIPCHK(vn_generic_forward(h->net, h->theta, s0, s1, h->fwd_grid, h->stream));
  }
  if (has_ansatz(b)) {                               // hard-constraint ansatz: (n, nd) -> (u, ud) before anything reads them
    if (int rc = ansatz_fold(h, b.az, h->u, h->ud, s0.n)) return rc;
    if (int rc = ansatz_fold(h, h->az_bic, h->ub, nullptr, h->nB)) return rc;
  }

  const long nthreads = b.n_k > h->nB ? b.n_k : h->nB;
  const int grid = (int)(((nthreads > 0 ? nthreads : 1) + 255) / 256);      // an empty set still zeroes its partials
  const int blp = bicw_lossparts(h);                 // weighted BC/IC rows: their own seed kernel, its partials behind the others
  if (int rc = ensure(&h->losspart, &h->losspart_cap, (long)(grid + blp) * 3)) return rc;
  VnSeedArgs a = seed_args(h, b);
  if (with_seeds) { a.ubar = h->ubar; a.udbar = h->udbar; a.ubar_b = h->ubar_b; }
  a.lossVec = weights_lossvec(h, b, lossVec); a.part = h->losspart;
  if (blp) { a.ub = nullptr; a.label = nullptr; a.nB = 0; a.bDof = 0; a.ubar_b = nullptr; }
  if (int rc = terms_fold_rows(h, b)) return rc;
  HIPCHK(vn_seed_launch(a, grid, h->stream));
  if (blp)
    if (int rc = bicw_seed(h, b, h->losspart + (long)grid * 3, with_seeds)) return rc;
  if (with_seeds) {
    if (int rc = bic_reduce(h, b)) return rc;      // boundary / initial amplitudes: u_b is in h->ub
    if (int rc = terms_seed_rows(h, b)) return rc;
  }
  if (int rc = weights_stage(h, b, a.lossVec, 256, nullptr, a.part, with_seeds)) return rc;
  if (with_seeds && has_ansatz(b)) {                 // ... and last, the seeds of (u, ud) -> those of (n, nd)
    if (int rc = ansatz_adjoint(h, b.az, h->ubar, h->udbar, s0.n)) return rc;
    if (int rc = ansatz_adjoint(h, h->az_bic, h->ubar_b, nullptr, h->nB)) return rc;
  }
  if (lossdst) {
    HIPCHK(vn_reduce_launch(nullptr, 0, 0, h->losspart, grid + blp, h->bDof, h->nB, a.w0, a.w1, a.w2, lossdst, h->stream,
                            VnOptArgs(), fx));
  }
  return VN_OK;
}

int run_layered(vn_engine* h, const Batch& b, float* gradbuf, const VnEdgeSums& fx) {
  if (int rc = run_forward_and_seed(h, b, true, nullptr, nullptr)) return rc;
  VnRows s0{}, s1{};
  s0.X = b.Input; s0.G = batch_gcoef(h, b); s0.ubar = h->ubar; s0.udbar = h->udbar; s0.n = b.n_k * h->cfg.integ_num;
  s1.X = bi_x(h, b); s1.G = nullptr; s1.ubar = h->ubar_b; s1.udbar = nullptr; s1.n = h->nB;
  // one gradient vector (no per-workgroup partials): the GEMMs accumulate into it chunk by chunk
  HIPCHK(hipMemsetAsync(h->partial, 0, (size_t)h->net.P * sizeof(float), h->stream));
  if (int rc = prof_start(h)) return rc;
  LAYCHK(vn_layered_backward(h->layered, h->theta, s0, h->partial, h->stream, lerr_, sizeof lerr_, 0));
  LAYCHK(vn_layered_backward(h->layered, h->theta, s1, h->partial, h->stream, lerr_, sizeof lerr_, 1));
  if (int rc = prof_stop(h)) return rc;
  const long nth = b.n_k > h->nB ? b.n_k : h->nB;
  const int lg = (int)(((nth > 0 ? nth : 1) + 255) / 256);
  HIPCHK(vn_reduce_launch(h->partial, 1, h->net.P, h->losspart, lg, h->bDof, h->nB, (float)h->w[0], (float)h->w[1],
                          (float)h->w[2], gradbuf, h->stream, h->fuse, fx));
  return VN_OK;
}

int run_generic(vn_engine* h, const Batch& b, float* gradbuf, const VnEdgeSums& fx) {
  if (int rc = run_forward_and_seed(h, b, true, nullptr, nullptr)) return rc;
  VnRows s0{}, s1{};
  s0.X = b.Input; s0.G = batch_gcoef(h, b); s0.ubar = h->ubar; s0.udbar = h->udbar; s0.n = b.n_k * h->cfg.integ_num;
  s1.X = bi_x(h, b); s1.G = nullptr; s1.ubar = h->ubar_b; s1.udbar = nullptr; s1.n = h->nB;
  if (int rc = prof_start(h)) return rc;
  HIPCHK(vn_generic_backward(h->net, h->theta, s0, s1, h->partial, h->bwd_grid, h->stream));
  if (int rc = prof_stop(h)) return rc;
  const long nthreads = b.n_k > h->nB ? b.n_k : h->nB;
  // (weighted BC/IC rows: run_forward_and_seed put their seed kernel's partials behind the others, their weighted seeds in ubar_b)
  const int lgrid = bicw_on(h) ? (int)(((nthreads > 0 ? nthreads : 1) + 255) / 256) + bicw_lossparts(h) : (int)((nthreads + 255) / 256);
  HIPCHK(vn_reduce_launch(h->partial, h->bwd_grid, h->net.P, h->losspart, lgrid, h->bDof, h->nB, (float)h->w[0],
                          (float)h->w[1], (float)h->w[2], gradbuf, h->stream, h->fuse, fx));
  return VN_OK;
}

// One launch of the fused kernel (8-wave, or 4-wave in the cross-check build) for the whole step: forward, weak-form epilogue
// and reverse pass of every tile, BC/IC tiles included
int run_fused(vn_engine* h, const Batch& b, float* gradbuf, const VnEdgeSums& fx) {
  VnFusedArgs a = fused_args(h, &b);
  a.X = b.Input; a.G = batch_gcoef(h, b); a.src = batch_src(h, b);
  a.nT = b.n_k * h->cfg.integ_num; a.n_k = b.n_k; a.feW = fe_w(h);
  a.Nrow = b.Nrow; a.dNtrow = b.dNtrow; a.detJv = b.detJv; a.detJ = (float)b.detJ;
  a.partial = h->partial; a.losspart = h->fused_losspart; a.stamps = h->stamps;
  const bool bw = bicw_on(h);                        // weighted BC/IC rows leave the launch (bicw_rows)
  if (bw) a.nB = 0;
  // one persistent workgroup per CU, but never more workgroups than tiles (small mini-batches: idle workgroups would still
  // image the weights, flush and store an all-zero partial that the reduction then has to read)
  const long tt = 128 / a.integ_num > 0 ? 128 / a.integ_num : 1;
  const long tiles = (a.n_k + tt - 1) / tt + (a.nB + 127) / 128;
  const int grid = h->full_grid ? h->ncu : (int)(tiles < 1 ? 1 : tiles < h->ncu ? tiles : h->ncu);
  if (int rc = bic_forward_reduce(h, b)) return rc;
  int bparts = 0, blp = 0;
  if (bw) {                                          // their partials behind the launch's own; the loss partials need the room too
    if (int rc = ensure(&h->tp_losspart, &h->tp_losspart_cap, (long)(grid + bicw_lossparts(h)) * 3)) return rc;
    if (int rc = grow_partial(h, grid + bicw_parts(h))) return rc;
    a.partial = h->partial; a.losspart = h->tp_losspart;
    if (int rc = bicw_rows(h, b, h->partial + (long)grid * h->net.P, a.losspart + (long)grid * 3, &bparts, &blp)) return rc;
  }
  if (int rc = prof_start(h)) return rc;
  if (h->route == Route::fused8) {
    if (int rc = fused8_launch(h, a, grid)) return rc;
  } else {
    HIPCHK(vn_fused_launch(a, grid, h->stream));
  }
  if (int rc = prof_stop(h)) return rc;
  HIPCHK(vn_reduce_launch(h->partial, grid + bparts, h->net.P, a.losspart, grid + blp, h->bDof, h->nB, a.w0, a.w1, a.w2,
                          gradbuf, h->stream, h->fuse, fx));
  return VN_OK;
}

// Test functions that do not fit one 128-point tile (integNum 216: 3-point Gauss in 2D+t) cannot have their
// R_k formed inside a tile.  Two launches of the 8-wave fused kernel around the row-wise seed kernel:
//   1. forward only  -> u, directional derivative per row          (2 F_pt)
//   2. vn_seed_kernel -> R_k, lossVec, variational loss partials, per-row seeds
//   3. reverse pass with those seeds (recomputes the forward); BC/IC tiles ride along   (6 F_pt)
// 8 F_pt per point instead of 6, against 8 F_pt at 0.07 of peak on the generic kernels.
// Also the step of a batch with a reaction term on the single-launch route, at any integ_num (vn_set_reaction): the term lives
// in the seed kernel; neither mode of the fused kernel looks at integ_num.  A flux term (vn_set_nlflux) and a diffusivity D(u)
// (vn_set_nldiff) take the same sequence, with their elementwise kernels around the seed kernel (terms_fold_rows, terms_seed_rows).
// So does a batch with per-test-function loss weights (vn_set_tf_weights, vn_set_causal): they are applied after the seed kernel.
int run_twopass(vn_engine* h, const Batch& b, float* gradbuf, const VnEdgeSums& fx) {
  const int grid = h->ncu, P = h->net.P;
  const int sgrid = (int)((b.n_k + 255) / 256);
  const bool az = has_ansatz(b);                     // hard-constraint ansatz: the BC/IC rows leave step 3 (ansatz_bic_rows)
  const bool bw = bicw_on(h);                        // weighted BC/IC rows: likewise (bicw_rows)
  if (int rc = ensure(&h->tp_losspart, &h->tp_losspart_cap, (long)(grid + sgrid + (az || bw ? ansatz_bic_lossparts(h) : 0)) * 3)) return rc;
  if (az || bw)
    if (int rc = grow_partial(h, grid + ansatz_bic_parts(h))) return rc;
  if (int rc = bic_forward_reduce(h, b)) return rc;
  float* lp = h->tp_losspart;
  VnFusedArgs f = fused_args(h, &b);
  f.X = b.Input; f.G = batch_gcoef(h, b); f.nT = b.n_k * h->cfg.integ_num; f.nB = 0;     // BC/IC: step 3
  f.partial = h->partial; f.losspart = lp;
  f.dir = -1; f.ostride = 1;
  f.mode = 1; f.out_u = h->u; f.out_ud = h->ud;
  if (int rc = fused8_launch(h, f, grid)) return rc;
  if (az)
    if (int rc = ansatz_fold(h, b.az, h->u, h->ud, f.nT)) return rc;

  VnSeedArgs a = seed_args(h, b);
  a.ubar = h->ubar; a.udbar = h->udbar;
  a.ub = nullptr; a.label = nullptr; a.nB = 0; a.bDof = 0; a.biDimVal = 0.f;   // BC/IC: step 3
  a.part = lp + (long)grid * 3;
  a.lossVec = weights_lossvec(h, b, nullptr);
  if (int rc = terms_fold_rows(h, b)) return rc;
  HIPCHK(vn_seed_launch(a, sgrid, h->stream));
  if (int rc = terms_seed_rows(h, b)) return rc;
  if (int rc = weights_stage(h, b, a.lossVec, 256, nullptr, a.part, true)) return rc;
  int bparts = 0, blp = 0;
  if (az) {
    if (int rc = ansatz_adjoint(h, b.az, h->ubar, h->udbar, f.nT)) return rc;
    if (int rc = ansatz_bic_rows(h, b, h->partial + (long)grid * P, lp + (long)(grid + sgrid) * 3, &bparts, &blp)) return rc;
  }
  if (bw)
    if (int rc = bicw_rows(h, b, h->partial + (long)grid * P, lp + (long)(grid + sgrid) * 3, &bparts, &blp)) return rc;

  f.mode = 2; f.out_u = nullptr; f.out_ud = nullptr; f.seed_u = h->ubar; f.seed_ud = h->udbar; f.nB = az || bw ? 0 : h->nB;
  if (int rc = prof_start(h)) return rc;
  if (int rc = fused8_launch(h, f, grid)) return rc;
  if (int rc = prof_stop(h)) return rc;
  HIPCHK(vn_reduce_launch(h->partial, grid + bparts, P, lp, grid + sgrid + blp, h->bDof, h->nB, f.w0, f.w1, f.w2, gradbuf, h->stream,
                          h->fuse, fx));
  return VN_OK;
}

// One gradient evaluation in the de-duplicated formulation (vn_dedup.hip header), 8 F_pt per unique point:
//   1. (u, du/dx_d) at the unique points: value forward + value-adjoint sweep to the inputs     (2 F_pt, vn_pgrad16.hip)
//   2. weak-form assembly over (test function, quadrature point) rows -> R_k, loss, per-row seeds
//   3. seed gather per unique point: su = d loss / d u, sg[d] = d loss / d u_{x_d}
//   4. ONE reverse launch of the fused kernel (recomputes the forward): the directional derivative is linear in its
//      direction, sum_d sg_d * d(u_{x_d})/d theta = d(sg . grad u)/d theta with sg held fixed, so the per-point direction
//      G = sg with tangent seed 1 and value seed su gives the whole gradient; BC/IC tiles ride along       (6 F_pt)
int run_dedup(vn_engine* h, const Batch& b, float* gradbuf, const VnEdgeSums& fx) {
  const int grid = h->ncu, P = h->net.P;
  const int sblk = (int)((b.n_k + VN_DEDUP_TFB - 1) / VN_DEDUP_TFB);
  const bool az = has_ansatz(b);                     // hard-constraint ansatz: the BC/IC rows leave step 4 (ansatz_bic_rows)
  const bool bw = bicw_on(h);                        // weighted BC/IC rows: likewise (bicw_rows)
  if (az || bw) {
    if (int rc = ensure(&h->dd_losspart, &h->dd_cap_lp, (long)(grid + sblk + ansatz_bic_lossparts(h)) * 3)) return rc;
    if (int rc = ensure(&h->dd_partial, &h->dd_partial_cap, (long)(grid + ansatz_bic_parts(h)) * P)) return rc;
  }
  float* lp = h->dd_losspart;                       // [grid + sblk][3] (+ the BC/IC rows' of an ansatz step)
  if (int rc = bic_forward_reduce(h, b)) return rc;
  // vn_profile_*: HIP events around the formulation's whole kernel sequence (steps 1-4; the reduction stays outside as
  // in the row-wise step)
  if (int rc = prof_start(h)) return rc;
  HIPCHK(point_pass(h, b.Xu, b.U, nullptr, nullptr, h->dd_uv));
  if (az) HIPCHK(vn_ansatz_points_fold_launch(ansatz_point_args(h, b), h->stream));
  VnDedupArgs a = dedup_args(h, b);
  a.stf = h->u; a.part = lp + (long)grid * 3;
  a.seed_u = h->dd_su; a.seed_g = h->dd_sg;
  a.lossVec = weights_lossvec(h, b, nullptr);
  if (int rc = terms_source_dedup(h, b, a)) return rc;
  HIPCHK(vn_dedup_seed_launch(a, sblk, h->stream));
  if (int rc = weights_stage(h, b, a.lossVec, VN_DEDUP_TFB, a.stf, a.part, false)) return rc;   // stf[k] *= omega_k before the gather
  HIPCHK(vn_dedup_gather_launch(a, h->stream));
  if (int rc = terms_gather_dedup(h, b, a)) return rc;
  int bparts = 0, blp = 0;
  if (az) {                                        // last before the reverse launch: the seeds of (u, grad u) -> those of (n, grad n)
    HIPCHK(vn_ansatz_points_adjoint_launch(ansatz_point_args(h, b), h->stream));
    if (int rc = ansatz_bic_rows(h, b, h->dd_partial + (long)grid * P, lp + (long)(grid + sblk) * 3, &bparts, &blp)) return rc;
  }
  if (bw)
    if (int rc = bicw_rows(h, b, h->dd_partial + (long)grid * P, lp + (long)(grid + sblk) * 3, &bparts, &blp)) return rc;
  if (src_learnt(h, b)) {                          // source identification: a row's seed is stf[k] x its quadrature weight
    VnSrcGradArgs g{};
    g.stf = a.stf; g.feW = fe_w(h); g.feN = h->feN; g.phi = b.sb_phi; g.J = b.sb_J;
    g.nT = b.n_k * h->cfg.integ_num; g.q = h->cfg.integ_num; g.mask = h->lv[LV_SRC].mask; g.part = h->lv[LV_SRC].part;
    HIPCHK(vn_srcgrad_rows_launch(g, &h->lv[LV_SRC].blocks, h->stream));
  }
  if (fld_learnt(h, b)) {                          // field identification: ... times D(u_j), with grad u of the row's point
    VnFldGradArgs g{};
    g.stf = a.stf; g.feW = fe_w(h); g.pack = h->dd_uv; g.uid = b.uid; g.G = b.fb_G; g.J = b.fb_J; g.dim = h->cfg.dim;
    g.nldiff = b.nldiff.on ? 1 : 0; g.cp = b.nldiff.on ? term_cp(h, b, b.nldiff) : nullptr;
    for (int i = 0; i < 3; ++i) g.c[i] = (float)b.nldiff.c[i];
    g.nT = b.n_k * h->cfg.integ_num; g.q = h->cfg.integ_num; g.mask = h->lv[LV_FLD].mask; g.part = h->lv[LV_FLD].part;
    HIPCHK(vn_fldgrad_rows_launch(g, &h->lv[LV_FLD].blocks, h->stream));
  }
  VnFusedArgs f = fused_args(h, &b);
  f.X = b.Xu; f.G = h->dd_sg; f.nT = b.U;
  f.partial = h->dd_partial; f.losspart = lp;
  f.mode = 2; f.dir = -1; f.ostride = 1;
  f.seed_u = h->dd_su; f.seed_ud = nullptr;          // tangent seed 1
  if (az || bw) f.nB = 0;
  if (int rc = fused8_launch(h, f, grid)) return rc;
  if (int rc = prof_stop(h)) return rc;
  HIPCHK(vn_reduce_launch(h->dd_partial, grid + bparts, P, lp, grid + sblk + blp, h->bDof, h->nB, f.w0, f.w1, f.w2, gradbuf, h->stream,
                          h->fuse, fx));
  return VN_OK;
}

// After the last kernel of a gradient evaluation that reads vector `id` (or what was mixed from it): with `fold` the partials are
// folded into its gradient (zeros when the batch wrote none: one zeroed partial row stands in), and with `update` the masked
// entries take their Adam step at step counter t and are clamped
int learnt_finish(vn_engine* h, int id, bool fold, bool update, double t) {
  const LearntKind& k = kLearnt[id];
  Learnt& v = h->lv[id];
  if (fold && v.blocks <= 0) {
    HIPCHK(hipMemsetAsync(v.part, 0, (size_t)v.J * sizeof(float), h->stream));
    v.blocks = 1;
  }
  VnLearntApplyArgs a{};
  if (fold) { a.part = v.part; a.blocks = v.blocks; }
  a.J = v.J; a.lanes = k.lanes; a.grad = v.grad;
  a.val = v.state; a.m = v.state + k.cap; a.v = v.state + 2 * k.cap;
  a.lo = v.bounds; a.hi = v.bounds + k.cap;
  a.mask = v.mask;
  a.R = v.R; a.mean = v.mean; a.weight = v.weight; a.l1 = v.l1;
  a.update = update ? 1 : 0;
  if (update) {
    const vn_config& c = h->cfg;
    a.lr_t = (float)(v.lr * std::sqrt(1.0 - std::pow(c.beta2, t)) / (1.0 - std::pow(c.beta1, t)));
    a.b1 = (float)c.beta1; a.b2 = (float)c.beta2; a.eps = (float)c.eps;
  }
  HIPCHK(vn_learnt_apply_launch(a, h->stream));
  return VN_OK;
}

// the prior of a vector, dropped (the caller has drained the stream)
void learnt_prior_drop(Learnt& v) {
  for (void* p : {(void*)v.R, (void*)v.mean, (void*)v.l1, (void*)v.pen})
    if (p) (void)hipFree(p);
  v.R = nullptr; v.mean = nullptr; v.l1 = nullptr; v.pen = nullptr;
  v.weight = 0.0;
}

// (the feature's own work buffers and the prior go with its vector)
void learnt_free(vn_engine* h, int id) {
  Learnt& v = h->lv[id];
  learnt_prior_drop(v);
  for (void* p : {(void*)v.state, (void*)v.bounds, (void*)v.grad, (void*)v.part})
    if (p) (void)hipFree(p);
  for (const Learnt::Work& w : v.work)
    if (w.p) (void)hipFree(w.p);
  v = Learnt{};
}

// vn_state_snapshot (`back`: vn_state_rollback): (value | m | v) of every learnt vector to (from) the copy behind them
int learnt_copy(vn_engine* h, bool back) {
  for (int id = 0; id < LV_N; ++id) {
    const Learnt& v = h->lv[id];
    if (!v.on) continue;
    const size_t n = 3 * (size_t)kLearnt[id].cap;
    HIPCHK(hipMemcpyAsync(v.state + (back ? 0 : n), v.state + (back ? n : 0), n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  }
  return VN_OK;
}

// the first vector that is learnt, in LearntId order (the one whose refusal of weighted batches is reported), or nullptr
const LearntKind* learnt_any(const vn_engine* h) {
  for (int id = 0; id < LV_N; ++id)
    if (h->lv[id].on) return &kLearnt[id];
  return nullptr;
}

// Source identification, first thing in an evaluation of batch b: the batch's basis must be the engine's, then s_mix is formed
int source_mix(vn_engine* h, const Batch& b, int batch) {
  if (!src_learnt(h, b)) return VN_OK;
  if (b.sb_J != h->lv[LV_SRC].J)
    return fail(VN_EINVAL, "batch %d has a source basis of %d streams, the learnt amplitudes (vn_set_source_learn) are %d", batch, b.sb_J, h->lv[LV_SRC].J);
  if (h->route == Route::fused4 && !b.Xu)
    return fail(VN_EUNSUPPORTED, "learnt source amplitudes are not built for VN_KERNEL_FUSED (the 4-wave cross-check geometry): its "
                                 "single launch leaves no row seeds to reduce; every other kernel family carries them");
  return learnt_mix(h, LV_SRC, SW_MIX, b.source, b.sb_phi, 0, b.sb_J, b.n_k * h->cfg.integ_num);
}

// Field identification, first thing in an evaluation of batch b (the routes without a point pass for the rows' grad u were refused by
// vn_set_field_learn): the batch's basis must be the engine's, then gcoef is formed -- the mix over the nT * dim entries of a
// stream -- and, on a de-duplication map, its CSR-ordered copy
int field_mix(vn_engine* h, const Batch& b, int batch) {
  if (!fld_learnt(h, b)) return VN_OK;
  if (b.fb_J != h->lv[LV_FLD].J)
    return fail(VN_EINVAL, "batch %d has a field basis of %d streams, the learnt amplitudes (vn_set_field_learn) are %d", batch, b.fb_J, h->lv[LV_FLD].J);
  const long n = b.n_k * h->cfg.integ_num * h->cfg.dim;
  if (int rc = learnt_mix(h, LV_FLD, FW_MIX, b.gcoef, b.fb_G, 0, b.fb_J, n)) return rc;
  if (n > 0 && b.Xu) {
    if (int rc = lv_ensure(h, LV_FLD, FW_CSR, n)) return rc;
    HIPCHK(vn_dedup_permute_launch(lv_work(h, LV_FLD, FW_MIX), b.rowidx, lv_work(h, LV_FLD, FW_CSR), b.n_k * h->cfg.integ_num, h->cfg.dim,
                                   h->stream));
  }
  return VN_OK;
}

// Boundary / initial amplitudes, first thing in an evaluation of batch b: the basis of the BC/IC set the batch reads must be the
// engine's, then the labels are formed -- all nBreg of them, so a stream keeps its stride; a steady engine reads the first bDof
int bic_mix(vn_engine* h, const Batch& b, int batch) {
  if (!bic_learnt(h, b)) return VN_OK;
  if (bic_basis_J(h, b) != h->lv[LV_BIC].J)
    return fail(VN_EINVAL, "the BC/IC rows of batch %d have a basis of %d streams, the learnt amplitudes (vn_set_bic_learn) are %d", batch,
                bic_basis_J(h, b), h->lv[LV_BIC].J);
  return learnt_mix(h, LV_BIC, BW_MIX, bi_y0(h, b), bic_basis(h, b), 0, h->lv[LV_BIC].J, h->nBreg);
}

// ---- RCCL, loaded at run time -------------------------------------------------------------
// librccl.so.1 is resolved by SONAME, so a process that already carries RCCL (PyTorch-ROCm does) shares that
// copy; VN_RCCL_LIB names another file.  Nothing here is touched unless vn_comm_* is called, so the library
// loads (and every other entry point works) on a machine without RCCL.
struct Rccl {
  void* dl = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommCount) CommCount = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclGetVersion) GetVersion = nullptr;
};
Rccl g_rccl;

int load_rccl() {
  if (g_rccl.dl) return VN_OK;
  // $VN_RCCL_LIB names THE library to use (no fall-through to another copy: a host that points at a specific build
  // must not silently get a different one); otherwise the SONAME a PyTorch-ROCm process already carries, then /opt/rocm
  const char* user = getenv("VN_RCCL_LIB");
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* dl = nullptr;
  if (user && *user) {
    dl = dlopen(user, RTLD_NOW | RTLD_LOCAL);
    if (!dl) return fail(VN_EUNSUPPORTED, "RCCL: VN_RCCL_LIB=%s cannot be loaded (%s)", user, dlerror());
  } else {
    for (const char* n : names) {
      dl = dlopen(n, RTLD_NOW | RTLD_LOCAL);
      if (dl) break;
    }
  }
  if (!dl) return fail(VN_EUNSUPPORTED, "RCCL not found (%s): set VN_RCCL_LIB", dlerror());
  Rccl r;
  r.dl = dl;
#define VN_SYM(field, name)                                                          \
  r.field = (decltype(r.field))dlsym(dl, name);                                      \
  if (!r.field) { dlclose(dl); return fail(VN_EUNSUPPORTED, "RCCL symbol %s missing", name); }
  VN_SYM(GetUniqueId, "ncclGetUniqueId")
  VN_SYM(CommInitRank, "ncclCommInitRank")
  VN_SYM(CommDestroy, "ncclCommDestroy")
  VN_SYM(CommCount, "ncclCommCount")
  VN_SYM(AllReduce, "ncclAllReduce")
  VN_SYM(GetErrorString, "ncclGetErrorString")
  VN_SYM(GetVersion, "ncclGetVersion")
#undef VN_SYM
  g_rccl = r;
  return VN_OK;
}

// (the collective library probes peers / IPC handles with HIP calls that may fail benignly; their stale last-error
// must not be reported by the launch check of the next kernel of this library)
#define RCCLCHK(expr)                                                                        \
  do {                                                                                       \
    ncclResult_t r_ = (expr);                                                                \
    (void)hipGetLastError();                                                                 \
    if (r_ != ncclSuccess) return fail(VN_ECOMM, "%s: %s", #expr, g_rccl.GetErrorString(r_)); \
  } while (0)

// ---- learnt weight scales (vn_set_reparam) ------------------------------------------------
void reparam_free(vn_engine* h) {
  void* ptrs[] = {h->rp.V, h->rp.sc, h->rp.snap, h->rp.gout, h->rp.group};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  h->rp = vn_engine::Reparam{};
}

// number of scales of (mode, granularity) on `net`, and the layer table of vn_reparam.hip with the entry -> group map
int reparam_layout(const VnNet& net, int mode, int gran, VnReparamArgs& a, std::vector<int>& group) {
  a = VnReparamArgs{};
  a.mode = mode;
  a.tied = mode == VN_REPARAM_SLOPE && gran == VN_REPARAM_PER_LAYER;
  a.nl = net.L + 1;
  a.P = net.P;
  group.assign(net.P, -1);
  int S = 0;
  for (int l = 1; l <= net.L + 1; ++l) {
    const int k = l - 1, fi = net.H[l - 1], fo = net.H[l];
    a.fi[k] = fi; a.fo[k] = fo; a.woff[k] = net.woff[l]; a.boff[k] = net.boff[l];
    const bool in = mode == VN_REPARAM_RWF || l <= net.L;       // slope: hidden layers only
    a.soff[k] = in ? S : -1;
    if (!in) continue;
    for (int i = 0; i < fi; ++i)
      for (int j = 0; j < fo; ++j) group[net.woff[l] + i * fo + j] = S + (a.tied ? 0 : j);
    if (mode == VN_REPARAM_SLOPE)                                // rwf: biases are in no group
      for (int j = 0; j < fo; ++j) group[net.boff[l] + j] = S + (a.tied ? 0 : j);
    S += a.tied ? 1 : fo;
  }
  a.S = S;
  return S;
}

inline bool reparam_on(const vn_engine* h) { return h->rp.mode != VN_REPARAM_NONE; }

// V = theta / f(s) (theta as it stands), then theta_eff = f(s) V: the rebuilt vector is the single source of truth
int reparam_factorise(vn_engine* h) {
  HIPCHK(vn_reparam_factorise_launch(h->rp.lay, h->rp.group, h->stream));
  HIPCHK(vn_reparam_rebuild_launch(h->rp.lay, h->rp.group, h->stream));
  return VN_OK;
}

}  // namespace

extern "C" {

const char* vn_last_error(void) { return g_err.c_str(); }
int vn_abi_version(void) { return VN_ABI_VERSION; }   // 7: vn_comm_abandon; 6: vn_forward_grad; 5: vn_comm_version; 4: vn_comm_available, validated Adam hyper-parameters (3: vn_config.widths[16], VN_KERNEL_LAYERED)

int vn_create(const vn_config* cfg, vn_engine** out) {
  if (!cfg || !out) return fail(VN_EINVAL, "null argument");
  *out = nullptr;
  VnNet net;
  if (int rc = build_net(*cfg, net)) return rc;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(VN_EHIP, "no HIP device available (%s): the VarNet engine has no CPU fallback",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (cfg->device < 0 || cfg->device >= ndev) return fail(VN_EINVAL, "requested processor %d is unavailable!", cfg->device);
  HIPCHK(hipSetDevice(cfg->device));
  Route route;
  if (int rc = pick_route(*cfg, net, &route)) return rc;
  vn_engine* h = new vn_engine();
  h->cfg = *cfg;              // taken literally (lr = 0 is a legal, if useless, TF learning rate: TFModel.py:130)
  h->net = net;
  h->route = route;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) h->ncu = prop.multiProcessorCount;
  const size_t P = net.P;
  if (route == Route::layered) {
    h->fwd_grid = h->bwd_grid = 1;            // one gradient vector, no per-workgroup partials
  } else {
    const size_t fwd_lds = vn_generic_fwd_lds_bytes(net), bwd_lds = vn_generic_bwd_lds_bytes(net);
    int fpc = (int)((160 * 1024) / fwd_lds); if (fpc > 4) fpc = 4; if (fpc < 1) fpc = 1;
    int bpc = (int)((160 * 1024) / bwd_lds); if (bpc > 2) bpc = 2; if (bpc < 1) bpc = 1;
    h->fwd_grid = h->ncu * fpc;
    h->bwd_grid = h->ncu * bpc;
  }
  h->ev0.resize(PROF_CAP, nullptr);
  h->ev1.resize(PROF_CAP, nullptr);
  h->cev0.resize(PROF_CAP, nullptr);
  h->cev1.resize(PROF_CAP, nullptr);
  hipError_t a = hipSuccess;
  if (a == hipSuccess) a = hipMalloc((void**)&h->theta, P * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&h->m, P * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&h->v, P * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&h->gradbuf_int, (P + 4) * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&h->lossbuf, 4 * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&h->partial, (size_t)h->bwd_grid * P * sizeof(float));
  if (a == hipSuccess) h->partial_rows = h->bwd_grid;
  if (a == hipSuccess) a = hipMalloc((void**)&h->feN, cfg->integ_num * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&h->fedNt, cfg->integ_num * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&h->feW, cfg->integ_num * sizeof(float));
  if (a == hipSuccess) a = hipMemset(h->theta, 0, P * sizeof(float));
  if (a == hipSuccess) a = hipMemset(h->m, 0, P * sizeof(float));
  if (a == hipSuccess) a = hipMemset(h->v, 0, P * sizeof(float));
  if (a == hipSuccess) a = hipMemset(h->gradbuf_int, 0, (P + 4) * sizeof(float));
  if (a != hipSuccess) {
    vn_destroy(h);
    return fail(VN_ENOMEM, "device allocation failed: %s", hipGetErrorString(a));
  }
  h->gradbuf = h->gradbuf_int;
  { const char* fg = getenv("VN_FULL_GRID"); h->full_grid = fg && *fg && *fg != '0'; }
  if (route == Route::layered) {
    char lerr[384] = "";
    if (vn_layered_create(&h->layered, net, lerr, sizeof lerr)) {
      vn_destroy(h);
      return fail(VN_EUNSUPPORTED, "layer-by-layer route unavailable: %s", lerr);
    }
    h->prof_name = "vn_layered_backward";
  } else if (route != Route::generic) {
    // (the forward-only mode of the 8-wave kernel writes its per-workgroup loss partials here too: vn_forward and
    // vn_eval_loss of a two-pass engine must not find it NULL)
    if (hipMalloc((void**)&h->fused_losspart, (size_t)h->ncu * 3 * sizeof(float)) != hipSuccess) {
      vn_destroy(h);
      return fail(VN_ENOMEM, "device allocation failed");
    }
    h->prof_name = "vn_fused_kernel";
    if (on_8wave(h)) {       // the instantiation that runs, as rocprofv3 prints it (template arguments)
      char nm[96];
      snprintf(nm, sizeof nm, "vn_fused16_kernel<%d, %d, %s>", net.L, vn_fused16_ks(net), net.act == VN_ACT_TANH ? "true" : "false");
      h->prof_name = nm;
    }
    if (hipMalloc((void**)&h->stamps, 8 * sizeof(unsigned long long)) == hipSuccess)
      (void)hipMemset(h->stamps, 0, 8 * sizeof(unsigned long long));
  }
  *out = h;
  return VN_OK;
}

int vn_destroy(vn_engine* h) {
  if (!h) return VN_OK;
  (void)hipSetDevice(h->cfg.device);
  if (h->layered) { (void)hipStreamSynchronize(h->stream); vn_layered_destroy(h->layered); h->layered = nullptr; }
  if (h->comm && g_rccl.CommDestroy) { (void)hipStreamSynchronize(h->stream); (void)g_rccl.CommDestroy(h->comm); h->comm = nullptr; }
  void* ptrs[] = {h->theta, h->m, h->v, h->snap, h->theta64, h->gradbuf_int, h->lossbuf, h->partial, h->feN, h->fedNt,
                  h->feW, h->u, h->ud, h->ubar, h->udbar, h->ub, h->ubar_b, h->losspart, h->fused_losspart, h->stamps, h->dd_uv, h->dd_su, h->dd_sg, h->dd_partial,
                  h->dd_losspart, h->rx_seff, h->nd_A, h->wt_lvec, h->wt_omega, h->wt_stat, h->tp_losspart, h->f16_stash, h->omisfit,
                  h->lb.ring, h->lb.theta_k, h->lb.g_k, h->lb.d, h->lb.part, h->lb.G, h->lb.coef, h->lb.meta};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (EdgeSet& e : h->es)
    for (float* p : e.buf)
      if (p) (void)hipFree(p);
  if (h->lb.out) (void)hipHostFree(h->lb.out);
  vn_obj64_free(h->o64);
  for (int id = 0; id < LV_N; ++id) learnt_free(h, id);
  reparam_free(h);
  if (h->tg_T) (void)hipFree(h->tg_T);
  if (h->tg_part) (void)hipFree(h->tg_part);
  if (h->tg_out) (void)hipFree(h->tg_out);
  for (Batch& b : h->batches) {
    if (b.gcsr) (void)hipFree(b.gcsr);
    clear_weights(b);
  }
  for (Adapt*& ad : h->bw) adapt_free(ad);
  if (h->bw_field) (void)hipFree(h->bw_field);
  for (auto e : h->ev0) if (e) (void)hipEventDestroy(e);
  for (auto e : h->ev1) if (e) (void)hipEventDestroy(e);
  for (auto e : h->cev0) if (e) (void)hipEventDestroy(e);
  for (auto e : h->cev1) if (e) (void)hipEventDestroy(e);
  delete h;
  return VN_OK;
}

int vn_set_stream(vn_engine* h, void* s) {
  if (!h) return fail(VN_EINVAL, "null handle");
  h->stream = (hipStream_t)s;
  return VN_OK;
}

int vn_param_count(const vn_engine* h, int64_t* n) {
  if (!h || !n) return fail(VN_EINVAL, "null argument");
  *n = h->net.P;
  return VN_OK;
}

int vn_params_init(vn_engine* h, uint64_t seed) {
  if (!h) return fail(VN_EINVAL, "null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  const VnNet& net = h->net;
  std::vector<float> t(net.P, 0.f);
  uint64_t s = seed;
  for (int l = 1; l <= net.L + 1; ++l) {
    const int fi = net.H[l - 1], fo = net.H[l];
    const double lim = std::sqrt(6.0 / (double)(fi + fo));          // keras glorot_uniform
    for (int i = 0; i < fi * fo; ++i) {
      const double u01 = (double)(splitmix64(s) >> 11) * (1.0 / 9007199254740992.0);
      t[net.woff[l] + i] = (float)((2.0 * u01 - 1.0) * lim);
    }
  }
  HIPCHK(hipMemcpyAsync(h->theta, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->m, 0, t.size() * sizeof(float), h->stream));
  if (h->cfg.optimizer == VN_OPT_RMSPROP) {          // TF-1 initialises the mean-square slot to ones
    std::vector<float> ones(net.P, 1.f);
    HIPCHK(hipMemcpyAsync(h->v, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  } else {
    HIPCHK(hipMemsetAsync(h->v, 0, t.size() * sizeof(float), h->stream));
  }
  if (reparam_on(h)) {          // the same draw, factorised with the registered s_init; the scale slots start at zero
    const size_t S = (size_t)h->rp.S;
    HIPCHK(hipMemcpyAsync(h->rp.sc, h->rp.s_init.data(), S * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->rp.sc + S, 0, 2 * S * sizeof(float), h->stream));
    if (int rc = reparam_factorise(h)) return rc;
  }
  // self-adaptive weights start over from their registered initial state (a static part of the BC/IC rows: its weights, rebuilt)
  if (int rc = adapt_each(h, [&](Adapt& ad) -> int { return adapt_reset(h, ad); })) return rc;
  adapt_point_omega(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  h->step = 0;
  lbfgs_invalidate(h);
  return VN_OK;
}

int vn_params_get(vn_engine* h, float* host, int64_t n) {
  if (!h || !host) return fail(VN_EINVAL, "null argument");
  if (n != h->net.P) return fail(VN_EINVAL, "expected %d parameters, got %lld", h->net.P, (long long)n);
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipMemcpyAsync(host, h->theta, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VN_OK;
}

int vn_params_set(vn_engine* h, const float* host, int64_t n) {
  if (!h || !host) return fail(VN_EINVAL, "null argument");
  if (n != h->net.P) return fail(VN_EINVAL, "expected %d parameters, got %lld", h->net.P, (long long)n);
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipMemcpyAsync(h->theta, host, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if (reparam_on(h))
    if (int rc = reparam_factorise(h)) return rc;          // with the current s; the slots stay, as they do without scales
  HIPCHK(hipStreamSynchronize(h->stream));
  lbfgs_invalidate(h);
  return VN_OK;
}

int vn_state_size(const vn_engine* h, int64_t* bytes) {
  if (!h || !bytes) return fail(VN_EINVAL, "null argument");
  *bytes = (int64_t)sizeof(int64_t) + 3ll * h->net.P * (int64_t)sizeof(float);
  // the adaptive state of every registered batch, in batch order, then that of every registered part of the BC/IC rows, bc first
  adapt_each(h, [&](Adapt& ad) -> int { *bytes += adapt_bytes(ad); return VN_OK; });
  return VN_OK;
}

int vn_state_export(vn_engine* h, void* host, int64_t bytes) {
  int64_t need = 0;
  if (!h || !host) return fail(VN_EINVAL, "null argument");
  vn_state_size(h, &need);
  if (bytes != need) return fail(VN_EINVAL, "state buffer must be %lld bytes", (long long)need);
  HIPCHK(hipSetDevice(h->cfg.device));
  char* p = (char*)host;
  memcpy(p, &h->step, sizeof(int64_t));
  p += sizeof(int64_t);
  const size_t nb = (size_t)h->net.P * sizeof(float);
  HIPCHK(hipMemcpyAsync(p, h->theta, nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(p + nb, h->m, nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(p + 2 * nb, h->v, nb, hipMemcpyDeviceToHost, h->stream));
  p += 3 * nb;
  if (int rc = adapt_each(h, [&](Adapt& ad) -> int { return adapt_host_copy(h, ad, p, false); })) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return VN_OK;
}

// Device-side snapshot of the optimizer state (parameters, both slots, step counter) and the way back to it: no host copy, no
// synchronisation -- everything is ordered on the engine stream.  What train()'s lossLag blocks stand on: a block of k epochs is
// enqueued before ONE read-back of its k losses; when the stopping test fires inside the block, the state is rolled back to the
// block's start and the epochs up to the one that met the tolerance are replayed (the steps are bitwise reproducible), so the
// run ends in exactly the state the reference's one-read-back-per-epoch loop ends in (VarNet.py:1346-1383).
int vn_state_snapshot(vn_engine* h) {
  if (!h) return fail(VN_EINVAL, "null handle");
  NOT_LBFGS("vn_state_snapshot (the block read-back of Adam / RMSProp epochs)");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t nb = (size_t)h->net.P * sizeof(float);
  if (!h->snap) HIPCHK(hipMalloc((void**)&h->snap, 3 * nb));
  HIPCHK(hipMemcpyAsync(h->snap, h->theta, nb, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->snap + h->net.P, h->m, nb, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->snap + 2 * (size_t)h->net.P, h->v, nb, hipMemcpyDeviceToDevice, h->stream));
  if (int rc = learnt_copy(h, false)) return rc;
  if (reparam_on(h)) {
    const size_t S = (size_t)h->rp.S;
    HIPCHK(hipMemcpyAsync(h->rp.snap, h->rp.V, nb, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->rp.snap + h->net.P, h->rp.sc, 4 * S * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  }
  // self-adaptive weights: the committed half (a pending one belongs to no step yet)
  if (int rc = adapt_each(h, [&](Adapt& ad) -> int { return adapt_snap_copy(h, ad, false); })) return rc;
  h->snap_step = h->step;
  return VN_OK;
}

int vn_state_rollback(vn_engine* h) {
  if (!h) return fail(VN_EINVAL, "null handle");
  NOT_LBFGS("vn_state_rollback (the block read-back of Adam / RMSProp epochs)");
  if (!h->snap || h->snap_step < 0) return fail(VN_ESTATE, "no snapshot to roll back to (call vn_state_snapshot first)");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t nb = (size_t)h->net.P * sizeof(float);
  HIPCHK(hipMemcpyAsync(h->theta, h->snap, nb, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->m, h->snap + h->net.P, nb, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->v, h->snap + 2 * (size_t)h->net.P, nb, hipMemcpyDeviceToDevice, h->stream));
  if (int rc = learnt_copy(h, true)) return rc;
  if (reparam_on(h)) {
    const size_t S = (size_t)h->rp.S;
    HIPCHK(hipMemcpyAsync(h->rp.V, h->rp.snap, nb, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->rp.sc, h->rp.snap + h->net.P, 4 * S * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  }
  if (int rc = adapt_each(h, [&](Adapt& ad) -> int { return adapt_snap_copy(h, ad, true); })) return rc;
  adapt_point_omega(h);
  h->step = h->snap_step;
  return VN_OK;
}

int vn_state_import(vn_engine* h, const void* host, int64_t bytes) {
  int64_t need = 0;
  if (!h || !host) return fail(VN_EINVAL, "null argument");
  vn_state_size(h, &need);
  if (bytes != need) return fail(VN_EINVAL, "state buffer must be %lld bytes", (long long)need);
  HIPCHK(hipSetDevice(h->cfg.device));
  const char* p = (const char*)host;
  memcpy(&h->step, p, sizeof(int64_t));
  p += sizeof(int64_t);
  const size_t nb = (size_t)h->net.P * sizeof(float);
  HIPCHK(hipMemcpyAsync(h->theta, p, nb, hipMemcpyHostToDevice, h->stream));
  if (!is_lbfgs(h)) {          // L-BFGS has no slots: a checkpoint's are ignored (and exported as the zeros vn_create left)
    HIPCHK(hipMemcpyAsync(h->m, p + nb, nb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->v, p + 2 * nb, nb, hipMemcpyHostToDevice, h->stream));
  }
  if (reparam_on(h))            // V from the imported theta_eff with the current s; a full restore calls vn_set_reparam_state next
    if (int rc = reparam_factorise(h)) return rc;
  char* q = const_cast<char*>(p) + 3 * nb;   // (read only: load)
  if (int rc = adapt_each(h, [&](Adapt& ad) -> int { return adapt_host_copy(h, ad, q, true); })) return rc;
  adapt_point_omega(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  lbfgs_invalidate(h);
  return VN_OK;
}

int vn_set_fe_table(vn_engine* h, const float* N, const float* dNt, const float* integW) {
  if (!h || !N || !dNt) return fail(VN_EINVAL, "null argument");
  if (h->cfg.has_integw && !integW) return fail(VN_EINVAL, "config has integW but none was given");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t nb = (size_t)h->cfg.integ_num * sizeof(float);
  HIPCHK(hipMemcpyAsync(h->feN, N, nb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->fedNt, dNt, nb, hipMemcpyHostToDevice, h->stream));
  if (integW) HIPCHK(hipMemcpyAsync(h->feW, integW, nb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // host buffers may be released on return
  h->has_fe = true;
  h->has_feW = integW != nullptr;
  h->feN_zero = false;
  for (int p = 0; p < h->cfg.integ_num; ++p) h->feN_zero = h->feN_zero || N[p] == 0.f;
  return VN_OK;
}

int vn_set_interior(vn_engine* h, int32_t batch, const float* Input, const float* gcoef, const float* source,
                    int64_t n_k, const float* detJ_dev, double detJ, const float* N_rows, const float* dNt_rows) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (batch < 0 || batch > 65535) return fail(VN_EINVAL, "batch index %d out of range", batch);
  if (n_k < 0) return fail(VN_EINVAL, "negative number of test functions");
  // n_k == 0 is a legal, empty tower feed (VarNetUtility.py:830-838 slices past the end): only the BC/IC rows
  // contribute, and the rank still takes part in the gradient SUM.
  if (n_k > 0 && (!Input || !gcoef)) return fail(VN_EINVAL, "null argument");
  if (n_k > 0 && h->cfg.has_source && !source) return fail(VN_EINVAL, "config has a source term but source is NULL");
  if ((N_rows == nullptr) != (dNt_rows == nullptr)) return fail(VN_EINVAL, "N_rows and dNt_rows must be given together");
  HIPCHK(hipSetDevice(h->cfg.device));
  if ((int)h->batches.size() <= batch) h->batches.resize(batch + 1);
  lbfgs_invalidate(h, batch);
  Batch& b = h->batches[batch];
  b.Input = Input; b.gcoef = gcoef; b.source = source; b.detJv = detJ_dev; b.detJ = detJ;
  b.Nrow = N_rows; b.dNtrow = dNt_rows; b.n_k = n_k; b.set = true;
  b.Xu = nullptr; b.uid = nullptr; b.rowptr = nullptr; b.rowidx = nullptr; b.U = 0;   // re-register with vn_set_dedup
  b.biInput = nullptr; b.biLabel = nullptr;                                            // ... and vn_set_batch_bic
  b.sb_phi = nullptr; b.sb_J = 0;                                                      // ... and vn_set_source_basis
  b.fb_G = nullptr; b.fb_J = 0;                                                        // ... and vn_set_field_basis
  b.bb_B = nullptr; b.bb_J = 0;                                                        // ... and vn_set_bic_basis of its own copy
  const Batch fresh;
  b.react = fresh.react; b.nlflux = fresh.nlflux; b.nldiff = fresh.nldiff;             // ... and the three term setters
  clear_weights(b);                                                                    // ... and vn_set_tf_weights / vn_set_causal
  b.az = Ansatz(); b.azp = Ansatz();                                                   // ... and vn_set_ansatz / vn_set_ansatz_points
  const long nT = n_k * h->cfg.integ_num;
  if (nT > h->work_rows) {
    long c0 = h->work_rows, c1 = h->work_rows, c2 = h->work_rows, c3 = h->work_rows;
    if (int rc = ensure(&h->u, &c0, nT)) return rc;
    if (int rc = ensure(&h->ud, &c1, nT)) return rc;
    if (int rc = ensure(&h->ubar, &c2, nT)) return rc;
    if (int rc = ensure(&h->udbar, &c3, nT)) return rc;
    h->work_rows = nT;
  }
  return VN_OK;
}

int vn_set_dedup(vn_engine* h, int32_t batch, const float* Xu, int64_t U, const int32_t* uid,
                 const int32_t* rowptr, const int32_t* rowidx) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (batch < 0 || batch >= (int)h->batches.size() || !h->batches[batch].set)
    return fail(VN_ESTATE, "batch %d has no interior data (call vn_set_interior first)", batch);
  lbfgs_invalidate(h, batch);
  Batch& b = h->batches[batch];
  b.azp = Ansatz();                            // the ansatz streams at the previous map's points go with it (vn_set_ansatz_points)
  if (!Xu) {                                   // switch the formulation off for this batch
    b.Xu = nullptr; b.uid = nullptr; b.rowptr = nullptr; b.rowidx = nullptr; b.U = 0;
    return VN_OK;
  }
  // A registration replaces the previous one: from here on the batch is row-wise until THIS map has been accepted, so a
  // rejected call never leaves the engine pointing at the previous call's arrays (which the caller may release on error).
  b.Xu = nullptr; b.uid = nullptr; b.rowptr = nullptr; b.rowidx = nullptr; b.U = 0;
  if (b.n_k <= 0) return fail(VN_EINVAL, "batch %d has no interior rows: nothing to de-duplicate", batch);
  if (!uid || !rowptr || !rowidx || U <= 0) return fail(VN_EINVAL, "null argument");
  // the formulation has no tiles of whole test functions (its rows are unique points), so it also serves integ_num beyond one
  // 128-point tile -- the networks of the two-pass route (216: three-point Gauss in 2D+t) -- up to the seed kernel's 256-row chunk
  if (!on_8wave(h)) return fail(VN_EUNSUPPORTED, "de-duplication needs the 8-wave fused kernel for this network");
  if (h->cfg.integ_num > 256) return fail(VN_EUNSUPPORTED, "de-duplication supports integ_num <= 256");
  if (b.Nrow || b.detJv) return fail(VN_EUNSUPPORTED, "de-duplication needs uniform supports (no per-row tables)");
  if (h->cfg.dim > 3) return fail(VN_EUNSUPPORTED, "de-duplication supports dim <= 3");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int dim = h->cfg.dim;
  const long nT = b.n_k * h->cfg.integ_num;
  if (int rc = ensure(&h->dd_uv, &h->dd_uv_cap, 4 * U)) return rc;          // [U, 4] packed (u, grad u) records
  if (int rc = ensure(&h->dd_su, &h->dd_su_cap, U)) return rc;
  if (int rc = ensure(&h->dd_sg, &h->dd_sg_cap, U * dim)) return rc;
  if (int rc = ensure(&h->dd_partial, &h->dd_partial_cap, (long)h->ncu * h->net.P)) return rc;
  if (int rc = ensure(&h->dd_losspart, &h->dd_cap_lp, ((long)h->ncu + (b.n_k + VN_DEDUP_TFB - 1) / VN_DEDUP_TFB) * 3)) return rc;
  // The map indexes device memory in every later kernel: validate it once, here (a registration call may synchronise), so
  // that an inconsistent map is an error code and never a GPU fault.  The rowptr reads assume U + 1 entries, rowidx / uid nT.
  int bad = 0;
  auto check = [&](int* err_dev) { return vn_dedup_check_launch(uid, rowptr, rowidx, nT, U, err_dev, h->stream); };
  if (int rc = count_on_device(h, check, &bad)) return rc;
  if (bad) return fail(VN_EINVAL, "inconsistent de-duplication map: %d violation(s) (need 0 <= uid < U, rowptr[0] = 0 <= ... <= rowptr[U] = n_k*integ_num, "
                                  "0 <= rowidx < n_k*integ_num, uid[rowidx[e]] = the point whose segment holds e, rows of a point in increasing order)", bad);
  // With constant coefficients gcoef = kappa dN/dx + v N repeats with period integ_num along the rows (the reference tiles the
  // tables to nT rows, VarNet.py:837): detected here, bitwise, and both assembly kernels then read the rows of test function 0
  // as an integ_num-entry table instead of 8 bytes per row each.  Otherwise the gather kernel gets gcoef in CSR order (it then
  // reads it, like rowidx, as one contiguous stream: a per-row gather of 8-byte entries fetched 2.6 x the bytes it used,
  // profiles/r5_pmc_traffic_dedup.json).  gcoef is static per batch: examined / permuted once, here.
  auto periodic = [&](int* err_dev) { return vn_dedup_periodic_launch(b.gcoef, nT, h->cfg.integ_num, dim, err_dev, h->stream); };
  if (int rc = count_on_device(h, periodic, &bad)) return rc;
  b.gper = bad == 0 && !h->no_gtable;
  if (!b.gper) {
    if (int rc = ensure(&b.gcsr, &b.gcsr_cap, nT * dim)) return rc;
    HIPCHK(vn_dedup_permute_launch(b.gcoef, rowidx, b.gcsr, nT, dim, h->stream));
  }
  if (has_terms(b))
    if (int rc = ensure(&h->rx_seff, &h->rx_seff_cap, nT)) return rc;
  for (const TermKind* k : kTerms)
    if ((b.*(k->slot)).on)
      if (int rc = check_Np(h, *k, batch, "cannot be de-duplicated")) return rc;
  b.Xu = Xu; b.U = U; b.uid = uid; b.rowptr = rowptr; b.rowidx = rowidx;
  return VN_OK;
}

// vn_set_reaction, vn_set_nlflux, vn_set_nldiff: coef == NULL, or the coefficients of an unregistered term (for D(u): D = 1 and
// no psi, which is advection on the value side), clear the term; a de-duplication map and the other terms stay
static int set_term(vn_engine* h, int32_t batch, const TermKind& k, const float* stream, const double coef[3]) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (batch < 0 || batch >= (int)h->batches.size() || !h->batches[batch].set)
    return fail(VN_ESTATE, "batch %d has no interior data (call vn_set_interior first)", batch);
  if (coef && !(std::isfinite(coef[0]) && std::isfinite(coef[1]) && std::isfinite(coef[2])))
    return fail(VN_EINVAL, "%s coefficients (%g, %g, %g) must be finite", k.coefs, coef[0], coef[1], coef[2]);
  Batch& b = h->batches[batch];
  if (b.n_k <= 0) return fail(VN_EINVAL, "batch %d has no interior rows: no %s to integrate", batch, k.integrand);
  lbfgs_invalidate(h, batch);
  const Term off = Batch().*(k.slot);
  // (a term with a learnt entry stays registered whatever `coef` says: its coefficients are the engine's, vn_set_coef_learn)
  const bool learnt = h->lv[LV_COEF].on && (h->lv[LV_COEF].mask >> (3 * (&k == &kReact ? 0 : &k == &kNlflux ? 1 : 2)) & 7u);
  if (!coef || (!learnt && std::equal(coef, coef + 3, off.c) && !(&k == &kNldiff && stream))) {
    b.*(k.slot) = off;
    return VN_OK;
  }
  if (&k == &kNlflux && !stream)
    return fail(VN_EINVAL, "the flux term needs phi = sum_d w_d dN/dx_d per interior row (phi_dev is NULL)");
  if (h->route == Route::fused4)
    return fail(VN_EUNSUPPORTED, "the %s is not built for VN_KERNEL_FUSED (the 4-wave cross-check geometry): its single "
                                 "launch has no place for the term; every other kernel family carries it", k.name);
  if (b.Xu)
    if (int rc = check_Np(h, k, batch, "cannot join its de-duplication map")) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  // (the row-wise work buffers u / ud / ubar / udbar of the two-pass sequence exist since vn_set_interior, on every route;
  // A_r of the D(u) pair is allocated when a batch first carries the term, and the steps grow it if a larger batch follows)
  if (&k == &kNldiff)
    if (int rc = ensure(&h->nd_A, &h->nd_A_cap, b.n_k * h->cfg.integ_num)) return rc;
  if (b.Xu)
    if (int rc = ensure(&h->rx_seff, &h->rx_seff_cap, b.n_k * h->cfg.integ_num)) return rc;
  Term& t = b.*(k.slot);
  t.on = true; t.stream = stream; std::copy(coef, coef + 3, t.c);
  return VN_OK;
}

int vn_set_reaction(vn_engine* h, int32_t batch, const float* rate, const double coef[3]) { return set_term(h, batch, kReact, rate, coef); }
int vn_set_nlflux(vn_engine* h, int32_t batch, const float* phi, const double coef[3]) { return set_term(h, batch, kNlflux, phi, coef); }
int vn_set_nldiff(vn_engine* h, int32_t batch, const float* psi, const double coef[3]) { return set_term(h, batch, kNldiff, psi, coef); }

// ---- learnt vectors: what vn_set_*_learn, vn_get_* and vn_set_* of the three share ----
// vn_set_*_learn: mask == NULL switches the vector off and frees it; `extra` holds the refusals that are the feature's own.
// Every call, also a failing one, invalidates the snapshot and the L-BFGS state and drops the vector's prior (vn_set_learnt_prior).
static int learnt_set_learn(vn_engine* h, int id, int32_t J, const int32_t* mask, const double* init, const double* lo, const double* hi,
                            double lr, int (*extra)(vn_engine*) = nullptr) {
  const LearntKind& k = kLearnt[id];
  if (!h) return fail(VN_EINVAL, "null handle");
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(h->cfg.device));
  h->snap_step = -1;
  lbfgs_invalidate(h);
  if (h->lv[id].pen) {                          // a prior belongs to one registration: every call, also a failing one, drops it
    HIPCHK(hipStreamSynchronize(h->stream));
    learnt_prior_drop(h->lv[id]);
  }
  if (!mask) {
    HIPCHK(hipStreamSynchronize(h->stream));
    learnt_free(h, id);
    return VN_OK;
  }
  if (!init || !lo || !hi) return fail(VN_EINVAL, "null argument");
  if (J < 1 || J > k.cap) return fail(VN_EINVAL, "1 to %d %s can be learnt, got %d", k.cap, k.what, J);
  if (h->cfg.optimizer != VN_OPT_ADAM)
    return fail(VN_EUNSUPPORTED, "%s on %s engine: the %ss are updated with the arithmetic of the Adam step only%s", k.setter,
                is_lbfgs(h) ? "an L-BFGS" : "an RMSProp", k.noun, is_lbfgs(h) ? " (vn_lbfgs_step searches over the parameters alone)" : "");
  if (h->comm)
    return fail(VN_EUNSUPPORTED, "%s under a communicator: %s are not in the all-reduced buffer, so every rank would follow its own "
                                 "shard's", k.setter, k.grads);
  if (extra)
    if (int rc = extra(h)) return rc;
  for (size_t i = 0; i < h->batches.size(); ++i)
    if (has_weights(h->batches[i])) return learnt_weights_refusal(k, (int)i);
  if (bicw_on(h))
    return fail(VN_EUNSUPPORTED, "%s next to weights on the BC/IC rows (vn_set_bic_weights / vn_set_bic_adapt): the %s sums next to the "
                                 "rows' own pass are not built", k.setter, k.noun);
  if (!(std::isfinite(lr) && lr > 0.0)) return fail(VN_EINVAL, "%s learning rate %g must be finite and > 0", k.noun, lr);
  for (int i = 0; i < J; ++i) {
    if (!std::isfinite(init[i])) return fail(VN_EINVAL, "initial %s %d = %g must be finite", k.noun, i, init[i]);
    if (std::isnan(lo[i]) || std::isnan(hi[i]) || lo[i] > hi[i])
      return fail(VN_EINVAL, "bounds of %s %d: [%g, %g] is no interval", k.noun, i, lo[i], hi[i]);
  }
  Learnt& v = h->lv[id];
  if (!v.state) {
    hipError_t e = hipMalloc((void**)&v.state, 6 * (size_t)k.cap * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&v.bounds, 2 * (size_t)k.cap * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&v.grad, (size_t)k.cap * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&v.part, (size_t)VN_LEARNT_MAXBLK * k.cap * sizeof(float));
    if (e != hipSuccess) { (void)hipGetLastError(); learnt_free(h, id); return fail(VN_ENOMEM, "%s: %s", k.setter, hipGetErrorString(e)); }
  }
  float st[6 * LV_CAP] = {}, bd[2 * LV_CAP] = {};    // (m, v and the snapshot copy start at zero)
  v.mask = 0;
  for (int i = 0; i < J; ++i) {
    st[i] = (float)init[i];
    bd[i] = (float)lo[i]; bd[k.cap + i] = (float)hi[i];
    if (mask[i]) v.mask |= 1ull << i;
  }
  v.lr = lr;
  v.J = J;
  HIPCHK(hipMemcpyAsync(v.state, st, 6 * (size_t)k.cap * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(v.bounds, bd, 2 * (size_t)k.cap * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(v.grad, 0, (size_t)k.cap * sizeof(double), h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));      // (st, bd leave scope)
  v.on = true;
  v.blocks = 0;
  return VN_OK;
}

// vn_get_*: the values at the current state, widened, and with `grad` the gradient of the last gradient evaluation
static int learnt_get(vn_engine* h, int id, double* val, double* grad, int32_t J) {
  const LearntKind& k = kLearnt[id];
  if (!h || !val) return fail(VN_EINVAL, "null argument");
  const Learnt& v = h->lv[id];
  if (!v.on) return fail(VN_ESTATE, "no learnt %s (call %s first)", k.what, k.setter);
  if (J != v.J) return fail(VN_EINVAL, "the engine holds %d %s, the caller asks for %d", v.J, k.what, J);
  HIPCHK(hipSetDevice(h->cfg.device));
  float c[LV_CAP];
  HIPCHK(hipMemcpyAsync(c, v.state, (size_t)J * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (grad) HIPCHK(hipMemcpyAsync(grad, v.grad, (size_t)J * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < J; ++i) val[i] = (double)c[i];
  return VN_OK;
}

// vn_set_*: the values overwritten (rounded to fp32, not clamped; the Adam slots stay); the snapshot and the L-BFGS state go
static int learnt_put(vn_engine* h, int id, const double* val, int32_t J) {
  const LearntKind& k = kLearnt[id];
  if (!h || !val) return fail(VN_EINVAL, "null argument");
  const Learnt& v = h->lv[id];
  if (!v.on) return fail(VN_ESTATE, "no learnt %s (call %s first)", k.what, k.setter);
  if (J != v.J) return fail(VN_EINVAL, "the engine holds %d %s, the caller passes %d", v.J, k.what, J);
  float c[LV_CAP];
  for (int i = 0; i < J; ++i) {
    if (!std::isfinite(val[i])) return fail(VN_EINVAL, "%s %d = %g must be finite", k.noun, i, val[i]);
    c[i] = (float)val[i];
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipMemcpyAsync(v.state, c, (size_t)J * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->snap_step = -1;
  lbfgs_invalidate(h);
  return VN_OK;
}

// vn_set_learnt_prior: the quadratic prior and the L1 weights of one learnt vector.  Static data: the Adam
// slots, the snapshot and the values stay as they are, so it may be called between steps to re-weight.
int vn_set_learnt_prior(vn_engine* h, int32_t kind, int32_t J, double weight, const double* R, const double* mean, const double* l1) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (kind < 0 || kind >= LV_N) return fail(VN_EINVAL, "learnt vector kind %d is none of VN_LEARNT_COEF .. VN_LEARNT_FLUXBC (0 to %d)", kind, LV_N - 1);
  const LearntKind& k = kLearnt[kind];
  Learnt& v = h->lv[kind];
  if (!v.on) return fail(VN_ESTATE, "no learnt %s (call %s first)", k.what, k.setter);
  if (J != v.J) return fail(VN_EINVAL, "the engine holds %d %s, the prior is for %d", v.J, k.what, J);
  if (!(std::isfinite(weight) && weight >= 0.0)) return fail(VN_EINVAL, "prior weight %g must be finite and >= 0", weight);
  if (R)
    for (int i = 0; i < J; ++i)
      for (int j = 0; j <= i; ++j) {
        const double x = R[(long)i * J + j], y = R[(long)j * J + i];
        if (!std::isfinite(x) || !std::isfinite(y))
          return fail(VN_EINVAL, "prior matrix entries (%d, %d) = %g and (%d, %d) = %g must be finite", i, j, x, j, i, y);
        if (x != y) return fail(VN_EINVAL, "prior matrix is not symmetric: entry (%d, %d) = %.17g, entry (%d, %d) = %.17g", i, j, x, j, i, y);
      }
  if (mean)
    for (int i = 0; i < J; ++i)
      if (!std::isfinite(mean[i])) return fail(VN_EINVAL, "prior mean of %s %d = %g must be finite", k.noun, i, mean[i]);
  if (l1)
    for (int i = 0; i < J; ++i)
      if (!(std::isfinite(l1[i]) && l1[i] >= 0.0)) return fail(VN_EINVAL, "L1 weight of %s %d = %g must be finite and >= 0", k.noun, i, l1[i]);
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));        // (a step in flight reads the buffers replaced below)
  learnt_prior_drop(v);
  if (weight == 0.0 && !l1) return VN_OK;
  const bool quad = weight > 0.0;
  hipError_t e = hipMalloc((void**)&v.pen, 2 * sizeof(double));
  if (e == hipSuccess && quad) e = hipMalloc((void**)&v.mean, (size_t)k.cap * sizeof(double));
  if (e == hipSuccess && quad && R) e = hipMalloc((void**)&v.R, (size_t)J * J * sizeof(double));
  if (e == hipSuccess && l1) e = hipMalloc((void**)&v.l1, (size_t)k.cap * sizeof(float));
  if (e != hipSuccess) { (void)hipGetLastError(); learnt_prior_drop(v); return fail(VN_ENOMEM, "vn_set_learnt_prior: %s", hipGetErrorString(e)); }
  double mu[LV_CAP] = {};
  float lam[LV_CAP] = {};
  for (int i = 0; i < J; ++i) {
    if (mean) mu[i] = mean[i];
    if (l1) lam[i] = (float)l1[i];
  }
  if (quad) HIPCHK(hipMemcpyAsync(v.mean, mu, (size_t)k.cap * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (v.R) HIPCHK(hipMemcpyAsync(v.R, R, (size_t)J * J * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (v.l1) HIPCHK(hipMemcpyAsync(v.l1, lam, (size_t)k.cap * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));        // (mu, lam leave scope; R is the caller's)
  v.weight = weight;
  return VN_OK;
}

// vn_get_learnt_prior: (Q, sum lambda |a|) at the current values -- the apply kernel's evaluate-only mode; changes no state
int vn_get_learnt_prior(vn_engine* h, int32_t kind, double out[2]) {
  if (!h || !out) return fail(VN_EINVAL, "null argument");
  if (kind < 0 || kind >= LV_N) return fail(VN_EINVAL, "learnt vector kind %d is none of VN_LEARNT_COEF .. VN_LEARNT_FLUXBC (0 to %d)", kind, LV_N - 1);
  const LearntKind& k = kLearnt[kind];
  const Learnt& v = h->lv[kind];
  if (!v.on) return fail(VN_ESTATE, "no learnt %s (call %s first)", k.what, k.setter);
  out[0] = out[1] = 0.0;
  if (!v.pen) return VN_OK;                       // no prior: both are 0
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(h->cfg.device));
  VnLearntApplyArgs a{};
  a.J = v.J; a.lanes = k.lanes; a.val = v.state; a.mask = v.mask;
  a.R = v.R; a.mean = v.mean; a.weight = v.weight; a.l1 = v.l1; a.pen = v.pen;
  HIPCHK(vn_learnt_apply_launch(a, h->stream));
  HIPCHK(hipMemcpyAsync(out, v.pen, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VN_OK;
}

// ---- inverse mode: the nine coefficients on the device, learnt next to the parameters (vn_learnt.hip) ----
int vn_set_coef_learn(vn_engine* h, const int32_t mask[9], const double init[9], const double lo[9], const double hi[9], double lr) {
  return learnt_set_learn(h, LV_COEF, VN_COEF_N, mask, init, lo, hi, lr);
}
int vn_get_coefs(vn_engine* h, double coef[9], double grad[9]) { return learnt_get(h, LV_COEF, coef, grad, VN_COEF_N); }
int vn_set_coefs(vn_engine* h, const double coef[9]) { return learnt_put(h, LV_COEF, coef, VN_COEF_N); }

// ---- source identification: basis streams per batch, amplitudes on the device, learnt next to the parameters (vn_learnt.hip) ----
int vn_set_source_basis(vn_engine* h, int32_t batch, const float* phi_dev, int32_t J) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (batch < 0 || batch >= (int)h->batches.size() || !h->batches[batch].set)
    return fail(VN_ESTATE, "batch %d has no interior data (call vn_set_interior first)", batch);
  Batch& b = h->batches[batch];
  lbfgs_invalidate(h, batch);
  b.sb_phi = nullptr; b.sb_J = 0;                  // a call replaces the previous registration, also when it fails
  if (!phi_dev || J == 0) return VN_OK;
  if (J < 0 || J > VN_SRC_MAX) return fail(VN_EINVAL, "a source basis has 1 to %d streams, got %d", VN_SRC_MAX, J);
  if (!h->cfg.has_source)
    return fail(VN_ESTATE, "vn_set_source_basis needs an engine created with has_source = 1 (pass a zero source stream to "
                           "vn_set_interior when the PDE has none)");
  if (b.n_k <= 0) return fail(VN_EINVAL, "batch %d has no interior rows: no source to integrate", batch);
  b.sb_phi = phi_dev; b.sb_J = J;
  return VN_OK;
}

int vn_set_source_learn(vn_engine* h, int32_t J, const int32_t* mask, const double* init, const double* lo, const double* hi, double lr) {
  return learnt_set_learn(h, LV_SRC, J, mask, init, lo, hi, lr);
}
int vn_get_source_amps(vn_engine* h, double* amp, double* grad, int32_t J) { return learnt_get(h, LV_SRC, amp, grad, J); }
int vn_set_source_amps(vn_engine* h, const double* amp, int32_t J) { return learnt_put(h, LV_SRC, amp, J); }

// ---- field identification: basis streams of gcoef per batch, amplitudes on the device, learnt next to the parameters (vn_learnt.hip) ----
int vn_set_field_basis(vn_engine* h, int32_t batch, const float* G_dev, int32_t J) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (batch < 0 || batch >= (int)h->batches.size() || !h->batches[batch].set)
    return fail(VN_ESTATE, "batch %d has no interior data (call vn_set_interior first)", batch);
  Batch& b = h->batches[batch];
  lbfgs_invalidate(h, batch);
  b.fb_G = nullptr; b.fb_J = 0;                  // a call replaces the previous registration, also when it fails
  if (!G_dev || J == 0) return VN_OK;
  if (J < 0 || J > VN_FLD_MAX) return fail(VN_EINVAL, "a field basis has 1 to %d streams, got %d", VN_FLD_MAX, J);
  if (b.n_k <= 0) return fail(VN_EINVAL, "batch %d has no interior rows: no direction to mix", batch);
  b.fb_G = G_dev; b.fb_J = J;
  return VN_OK;
}

// what vn_set_field_learn refuses on its own: the amplitude reduction reads the rows' grad u from an 8-wave point pass
static int field_learn_checks(vn_engine* h) {
  if (h->cfg.dim > 3)
    return fail(VN_EUNSUPPORTED, "learnt field amplitudes need dim <= 3, got %d: the point pass that gives the rows' grad u carries "
                                 "three gradient components", h->cfg.dim);
  if (h->route == Route::layered)
    return fail(VN_EUNSUPPORTED, "learnt field amplitudes are not built for the layer-by-layer route: it has no point pass for the "
                                 "rows' grad u; networks of the hand-written kernels carry one");
  if (h->route == Route::fused4)
    return fail(VN_EUNSUPPORTED, "learnt field amplitudes are not built for VN_KERNEL_FUSED (the 4-wave cross-check geometry): its "
                                 "single launch leaves no row seeds to reduce; every other kernel family carries them");
  if (!on_8wave(h) && !(vn_fused16_net_supported(h->net) && h->net.act != VN_ACT_PER_LAYER))
    return fail(VN_EUNSUPPORTED, "learnt field amplitudes on the generic kernels need a network of the 8-wave point pass for the rows' "
                                 "grad u; this one (%d layers, widest %d, %d inputs%s) has none", h->net.L, h->net.hmax, h->net.d_in,
                h->net.act == VN_ACT_PER_LAYER ? ", mixed activations" : "");
  return VN_OK;
}

int vn_set_field_learn(vn_engine* h, int32_t J, const int32_t* mask, const double* init, const double* lo, const double* hi, double lr) {
  return learnt_set_learn(h, LV_FLD, J, mask, init, lo, hi, lr, field_learn_checks);
}
int vn_get_field_amps(vn_engine* h, double* amp, double* grad, int32_t J) { return learnt_get(h, LV_FLD, amp, grad, J); }
int vn_set_field_amps(vn_engine* h, const double* amp, int32_t J) { return learnt_put(h, LV_FLD, amp, J); }

// ---- boundary data identification: basis streams of the BC/IC labels per row set, amplitudes on the device (vn_learnt.hip) ----
int vn_set_bic_basis(vn_engine* h, int32_t batch, const float* B_dev, int32_t J) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (batch < -1) return fail(VN_EINVAL, "batch index %d out of range (-1: the rows of vn_set_bic)", batch);
  if (batch >= 0 && (batch >= (int)h->batches.size() || !h->batches[batch].set))
    return fail(VN_ESTATE, "batch %d has no interior data (call vn_set_interior first)", batch);
  const float** B = batch < 0 ? &h->bicB : &h->batches[batch].bb_B;
  int* Jreg = batch < 0 ? &h->bicJ : &h->batches[batch].bb_J;
  h->snap_step = -1;
  if (batch < 0) lbfgs_invalidate(h); else lbfgs_invalidate(h, batch);
  *B = nullptr; *Jreg = 0;                         // a call replaces the previous registration, also when it fails
  if (!B_dev || J == 0) return VN_OK;
  if (J < 0 || J > VN_BIC_MAX) return fail(VN_EINVAL, "a BC/IC basis has 1 to %d streams, got %d", VN_BIC_MAX, J);
  if (batch >= 0 && !h->batches[batch].biLabel)
    return fail(VN_ESTATE, "batch %d has no BC/IC rows of its own (call vn_set_batch_bic first, or pass batch = -1 for the rows of vn_set_bic)", batch);
  if (h->nBreg <= 0) return fail(VN_EINVAL, "no BC/IC rows are registered (vn_set_bic): no label to mix");
  *B = B_dev; *Jreg = J;
  return VN_OK;
}

// what vn_set_bic_learn refuses on its own
static int bic_learn_checks(vn_engine* h) {
  if (h->route == Route::fused4)
    return fail(VN_EUNSUPPORTED, "learnt boundary and initial amplitudes are not built for VN_KERNEL_FUSED (the 4-wave cross-check "
                                 "geometry): its single launch leaves no values of the BC/IC rows to reduce; every other kernel family carries them");
  return VN_OK;
}

int vn_set_bic_learn(vn_engine* h, int32_t J, const int32_t* mask, const double* init, const double* lo, const double* hi, double lr) {
  return learnt_set_learn(h, LV_BIC, J, mask, init, lo, hi, lr, bic_learn_checks);
}
int vn_get_bic_amps(vn_engine* h, double* amp, double* grad, int32_t J) { return learnt_get(h, LV_BIC, amp, grad, J); }
int vn_set_bic_amps(vn_engine* h, const double* amp, int32_t J) { return learnt_put(h, LV_BIC, amp, J); }

// ---- flux boundary identification: basis streams of the flux rows' datum and coefficient, amplitudes on the device (vn_learnt.hip) ----
int vn_set_fluxbc_basis(vn_engine* h, const float* S_dev, int32_t J_flux, int32_t J_robin) {
  if (!h) return fail(VN_EINVAL, "null handle");
  h->snap_step = -1;
  lbfgs_invalidate(h);
  h->fbcS = nullptr; h->fbcJl = h->fbcJc = 0;      // a call replaces the previous registration, also when it fails
  if (!S_dev || (J_flux == 0 && J_robin == 0)) return VN_OK;
  if (J_flux < 0 || J_robin < 0 || (long)J_flux + J_robin > VN_FBC_MAX)
    return fail(VN_EINVAL, "a flux-row basis has 1 to %d streams (flux datum and Robin coefficient together), got %d + %d", VN_FBC_MAX,
                J_flux, J_robin);
  if (h->es[VN_EDGE_FLUX].count <= 0)
    return fail(VN_ESTATE, "no boundary-flux rows are registered (call vn_set_flux_bc first): no datum or coefficient to mix");
  h->fbcS = S_dev; h->fbcJl = J_flux; h->fbcJc = J_robin;
  return VN_OK;
}

int vn_set_fluxbc_learn(vn_engine* h, int32_t J, const int32_t* mask, const double* init, const double* lo, const double* hi, double lr) {
  return learnt_set_learn(h, LV_FBC, J, mask, init, lo, hi, lr);
}
int vn_get_fluxbc_amps(vn_engine* h, double* amp, double* grad, int32_t J) { return learnt_get(h, LV_FBC, amp, grad, J); }
int vn_set_fluxbc_amps(vn_engine* h, const double* amp, int32_t J) { return learnt_put(h, LV_FBC, amp, J); }

// vn_set_tf_weights / vn_set_causal: what both check before they touch the batch; *clear: the call unregisters
static int weights_common(vn_engine* h, int32_t batch, bool clear, const char* who) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (batch < 0 || batch >= (int)h->batches.size() || !h->batches[batch].set)
    return fail(VN_ESTATE, "batch %d has no interior data (call vn_set_interior first)", batch);
  Batch& b = h->batches[batch];
  if (clear) {
    HIPCHK(hipSetDevice(h->cfg.device));
    lbfgs_invalidate(h, batch);
    clear_weights(b);
    return VN_OK;
  }
  if (b.n_k <= 0) return fail(VN_EINVAL, "batch %d has no interior rows: no test function to weight", batch);
  if (const LearntKind* k = learnt_any(h)) return learnt_weights_refusal(*k, batch);
  if (h->route == Route::fused4)
    return fail(VN_EUNSUPPORTED, "%s is not built for VN_KERNEL_FUSED (the 4-wave cross-check geometry): its single launch has no "
                                 "place for the weights; every other kernel family carries them", who);
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = ensure(&h->wt_lvec, &h->wt_lvec_cap, b.n_k)) return rc;
  return VN_OK;
}

int vn_set_tf_weights(vn_engine* h, int32_t batch, const float* omega_dev) {
  if (int rc = weights_common(h, batch, omega_dev == nullptr, "vn_set_tf_weights")) return rc;
  if (!omega_dev) return VN_OK;
  lbfgs_invalidate(h, batch);
  Batch& b = h->batches[batch];
  clear_weights(b);                                  // replaces a causal registration
  b.wt.omega = omega_dev;
  return VN_OK;
}

int vn_set_causal(vn_engine* h, int32_t batch, const int32_t* slab_dev, int32_t n_slabs, double eps) {
  if (slab_dev) {
    if (!(std::isfinite(eps) && eps >= 0.0)) return fail(VN_EINVAL, "causal eps = %g must be finite and >= 0", eps);
    if (n_slabs < 1 || n_slabs > VN_WEIGHTS_MAX_SLABS)
      return fail(VN_EINVAL, "n_slabs = %d outside [1, %d]", n_slabs, VN_WEIGHTS_MAX_SLABS);
    if (h && h->comm)
      return fail(VN_EUNSUPPORTED, "vn_set_causal under a communicator: a rank's slab means would cover only its shard, so the "
                                   "ranks together would train another objective than one rank");
  }
  if (int rc = weights_common(h, batch, slab_dev == nullptr, "vn_set_causal")) return rc;
  if (!slab_dev) return VN_OK;
  Batch& b = h->batches[batch];
  const long n_k = b.n_k;
  const int S = n_slabs;
  // the ids index LDS and the CSR in every later step: validated here, on the device, so that a bad id is an error code
  int bad = 0;
  auto check = [&](int* err_dev) { return vn_weights_check_launch(slab_dev, n_k, S, err_dev, h->stream); };
  if (int rc = count_on_device(h, check, &bad)) return rc;
  if (bad) return fail(VN_EINVAL, "%d slab id(s) outside [0, %d)", bad, S);
  if (int rc = ensure(&h->wt_omega, &h->wt_omega_cap, n_k)) return rc;
  if (int rc = ensure(&h->wt_stat, &h->wt_stat_cap, kWtStat)) return rc;
  // copied at this call (the caller's array need not outlive it); CSR slab -> test functions in increasing k, by counting sort
  std::vector<int> own((size_t)n_k + (size_t)S + 1 + (size_t)n_k);
  int* slab = own.data();
  int* sptr = slab + n_k;
  int* sidx = sptr + S + 1;
  HIPCHK(hipMemcpyAsync(slab, slab_dev, (size_t)n_k * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::fill(sptr, sptr + S + 1, 0);
  for (long k = 0; k < n_k; ++k) sptr[slab[k] + 1] += 1;
  long most = 0;
  for (int s = 0; s < S; ++s) { most = std::max<long>(most, sptr[s + 1]); sptr[s + 1] += sptr[s]; }
  std::vector<int> fill(sptr, sptr + S);
  for (long k = 0; k < n_k; ++k) sidx[fill[slab[k]]++] = (int)k;
  int* dev = nullptr;
  HIPCHK(hipMalloc((void**)&dev, own.size() * sizeof(int)));
  hipError_t e = hipMemcpyAsync(dev, own.data(), own.size() * sizeof(int), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { (void)hipFree(dev); return fail(VN_EHIP, "vn_set_causal: %s", hipGetErrorString(e)); }
  lbfgs_invalidate(h, batch);
  clear_weights(b);                                  // replaces a static (or an earlier causal) registration
  b.wt_own = dev;
  b.wt.slab = dev; b.wt.sptr = dev + n_k; b.wt.sidx = dev + n_k + S + 1;
  b.wt.S = S; b.wt.eps = eps;
  // workgroups per slab: one per 1024 test functions of the fullest slab (four loads in flight per thread)
  b.wt.chunks = (int)std::min<long>(VN_WEIGHTS_MAX_CHUNKS, std::max<long>(1, (most + 1023) / 1024));
  return VN_OK;
}

int vn_causal_weights(vn_engine* h, int32_t batch, double* omega_slab_host, int32_t n_slabs) {
  if (!h || !omega_slab_host) return fail(VN_EINVAL, "null argument");
  (void)hipGetLastError();
  if (int rc = check_batch(h, batch)) return rc;
  const Batch& b = h->batches[batch];
  if (b.wt.S <= 0) return fail(VN_ESTATE, "batch %d has no causal registration (call vn_set_causal first)", batch);
  if (n_slabs != b.wt.S) return fail(VN_EINVAL, "n_slabs = %d, batch %d was registered with %d", n_slabs, batch, b.wt.S);
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = run_forward_and_seed(h, b, false, nullptr, nullptr)) return rc;      // loss only: the interior loss field and its weights
  HIPCHK(hipMemcpyAsync(omega_slab_host, weights_work(h).oslab, (size_t)b.wt.S * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VN_OK;
}

// ---- self-adaptive weights (vn_adapt.hip) ----
// par: [0], [1] = (gamma, eta) of rba or (lr, cap) of sa; [2..4] = beta1, beta2, eps of sa; [5] power; [6] init; [7] normalize;
// [8] every; [9] reserved
// The rule and its parameters (par: the layout above), as vn_set_tf_adapt and vn_set_bic_adapt check them
static int adapt_check_par(const char* who, int32_t rule, const double par[10]) {
  if (rule != VN_ADAPT_RBA && rule != VN_ADAPT_SA) return fail(VN_EINVAL, "%s: rule = %d is none of 0 (clear), 1 (rba), 2 (sa)", who, rule);
  if (!par) return fail(VN_EINVAL, "%s: null parameter array", who);
  for (int i = 0; i < 10; ++i)
    if (!std::isfinite(par[i])) return fail(VN_EINVAL, "%s: par[%d] = %g is not finite", who, i, par[i]);
  if (rule == VN_ADAPT_RBA) {
    if (!(par[0] >= 0.0 && par[0] <= 1.0)) return fail(VN_EINVAL, "%s: rba gamma = %g must lie in [0, 1]", who, par[0]);
    if (!(par[1] >= 0.0)) return fail(VN_EINVAL, "%s: rba eta = %g must be >= 0", who, par[1]);
  } else {
    if (!(par[0] >= 0.0)) return fail(VN_EINVAL, "%s: sa lr = %g must be >= 0", who, par[0]);
    if (!(par[1] > 0.0)) return fail(VN_EINVAL, "%s: sa cap = %g must be positive", who, par[1]);
    if (!(par[2] >= 0.0 && par[2] < 1.0) || !(par[3] >= 0.0 && par[3] < 1.0))
      return fail(VN_EINVAL, "%s: sa beta1 = %g, beta2 = %g must lie in [0, 1)", who, par[2], par[3]);
    if (!(par[4] > 0.0)) return fail(VN_EINVAL, "%s: sa eps = %g must be positive", who, par[4]);
  }
  if (par[5] != 1.0 && par[5] != 2.0) return fail(VN_EINVAL, "%s: power = %g must be 1 or 2", who, par[5]);
  if (!(par[6] >= 0.0)) return fail(VN_EINVAL, "%s: init = %g must be >= 0", who, par[6]);
  if (par[7] != 0.0 && par[7] != 1.0) return fail(VN_EINVAL, "%s: normalize = %g must be 0 or 1", who, par[7]);
  if (!(par[8] >= 1.0) || par[8] != std::floor(par[8]) || par[8] > 1e15)
    return fail(VN_EINVAL, "%s: every = %g must be a whole number >= 1", who, par[8]);
  return VN_OK;
}

// One state of n weights, built and brought to its initial values: lambda from init_dev (validated on the device: finite, >= 0;
// copied, so the caller's array need not outlive the call), else par[6].  power, normalize and every come from par as well.
// who, rows and what word the messages ("<who>: the state of <n> <rows> does not fit", "<who>: <count> <what> negative or not
// finite").  *out on success; on failure nothing is kept.
static int adapt_make(vn_engine* h, const char* who, const char* rows, const char* what, long n, int rule, const double par[10],
                      const float* init_dev, Adapt** out) {
  Adapt* ad = new Adapt();
  ad->rule = rule; ad->power = (int)par[5]; ad->normalize = (int)par[7]; ad->every = (long)par[8];
  std::copy(par, par + 10, ad->par);
  ad->n_k = n; ad->stride = vn_adapt_stride(n);
  hipError_t e = hipMalloc((void**)&ad->f, (size_t)(kAdaptPieces * ad->stride) * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&ad->d, (size_t)kAdaptDoubles * sizeof(double));
  if (e == hipSuccess) e = hipMemsetAsync(ad->f, 0, (size_t)(kAdaptPieces * ad->stride) * sizeof(float), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(ad->d, 0, (size_t)kAdaptDoubles * sizeof(double), h->stream);
  int rc = VN_OK;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    rc = fail(VN_ENOMEM, "%s: the state of %ld %s does not fit: %s", who, n, rows, hipGetErrorString(e));
  } else if (init_dev) {
    int bad = 0;
    auto check = [&](int* err_dev) { return vn_adapt_check_copy_launch(init_dev, n, adapt_lambda0(*ad), err_dev, h->stream); };
    rc = count_on_device(h, check, &bad);
    if (rc == VN_OK && bad) rc = fail(VN_EINVAL, "%s: %d %s negative or not finite", who, bad, what);
  } else {
    e = vn_adapt_fill_launch(adapt_lambda0(*ad), n, (float)par[6], h->stream);
    if (e != hipSuccess) rc = fail(VN_EHIP, "%s: %s", who, hipGetErrorString(e));
  }
  if (rc == VN_OK) rc = adapt_reset(h, *ad);
  if (rc == VN_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(VN_EHIP, "%s: the initial state could not be formed", who);
  if (rc != VN_OK) { adapt_free(ad); return rc; }
  *out = ad;
  return VN_OK;
}

// The committed half read back, every array optional: lambda, omega [n_k], slots [2 n_k] (the caller has checked that the rule
// has them), n_k floats of extra_dev (the rows' loss field), the six statistics
static int adapt_get(vn_engine* h, const Adapt& ad, float* lambda_host, float* omega_host, float* slots_host, const float* extra_dev,
                     float* extra_host, double stats[6]) {
  const VnAdaptState s = adapt_state(ad, ad.cur);
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t nk = (size_t)ad.n_k * sizeof(float);
  if (lambda_host) HIPCHK(hipMemcpyAsync(lambda_host, s.lambda, nk, hipMemcpyDeviceToHost, h->stream));
  if (omega_host) HIPCHK(hipMemcpyAsync(omega_host, s.omega, nk, hipMemcpyDeviceToHost, h->stream));
  if (slots_host) {
    HIPCHK(hipMemcpyAsync(slots_host, s.m1, nk, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(slots_host + ad.n_k, s.m2, nk, hipMemcpyDeviceToHost, h->stream));
  }
  if (extra_host) HIPCHK(hipMemcpyAsync(extra_host, extra_dev, nk, hipMemcpyDeviceToHost, h->stream));
  if (stats) HIPCHK(hipMemcpyAsync(stats, s.scal, 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VN_OK;
}

// A state put back into the committed half: lambda (checked here: finite, >= 0), the sa slots (NULL: zeros) and tau; omega, Z
// and the statistics are rebuilt from them.  subject ("batch 0", "the bc part") words the refusal of slots under the rba rule.
static int adapt_put(vn_engine* h, Adapt& ad, const char* who, const char* subject, const float* lambda_host, const float* slots_host,
                     int64_t tau) {
  if (!lambda_host) return fail(VN_EINVAL, "%s: null lambda", who);
  if (tau < 0) return fail(VN_EINVAL, "%s: tau = %lld must be >= 0", who, (long long)tau);
  if (slots_host && ad.rule != VN_ADAPT_SA) return fail(VN_EINVAL, "%s: %s runs the rba rule, which has no slots", who, subject);
  for (long k = 0; k < ad.n_k; ++k)
    if (!(lambda_host[k] >= 0.f && std::isfinite(lambda_host[k])))
      return fail(VN_EINVAL, "%s: lambda[%ld] = %g is negative or not finite", who, k, (double)lambda_host[k]);
  HIPCHK(hipSetDevice(h->cfg.device));
  const VnAdaptState s = adapt_state(ad, ad.cur);
  const size_t nk = (size_t)ad.n_k * sizeof(float);
  double scal[VN_ADAPT_SCAL] = {};
  scal[5] = (double)tau;
  HIPCHK(hipMemcpyAsync(s.lambda, lambda_host, nk, hipMemcpyHostToDevice, h->stream));
  if (s.m1) {                   // NULL slots: zeros
    if (slots_host) {
      HIPCHK(hipMemcpyAsync(s.m1, slots_host, nk, hipMemcpyHostToDevice, h->stream));
      HIPCHK(hipMemcpyAsync(s.m2, slots_host + ad.n_k, nk, hipMemcpyHostToDevice, h->stream));
    } else {
      HIPCHK(hipMemsetAsync(s.m1, 0, 2 * (size_t)ad.stride * sizeof(float), h->stream));
    }
  }
  HIPCHK(hipMemcpyAsync(s.scal, scal, sizeof scal, hipMemcpyHostToDevice, h->stream));
  if (int rc = adapt_rebuild(h, ad)) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));   // the host arrays may be released on return
  return VN_OK;
}

int vn_set_tf_adapt(vn_engine* h, int32_t batch, int32_t rule, const double par[10], const float* lambda_init_dev) {
  const bool clear = rule == VN_ADAPT_NONE;
  if (!clear) {
    if (int rc = adapt_check_par("vn_set_tf_adapt", rule, par)) return rc;
    if (h && h->comm)
      return fail(VN_EUNSUPPORTED, "vn_set_tf_adapt under a communicator: a rank's max, mean and Z would cover only its shard, so the "
                                   "ranks together would train another objective than one rank");
  }
  if (int rc = weights_common(h, batch, clear, "vn_set_tf_adapt")) return rc;
  if (clear) return VN_OK;
  Batch& b = h->batches[batch];
  Adapt* ad = nullptr;          // on failure the batch keeps what it had
  if (int rc = adapt_make(h, "vn_set_tf_adapt", "test functions", "initial lambda(s)", b.n_k, rule, par, lambda_init_dev, &ad)) return rc;
  lbfgs_invalidate(h, batch);
  clear_weights(b);                                  // replaces a static, a causal or an earlier adaptive registration
  b.ad = ad;
  adapt_point_omega(h);
  return VN_OK;
}

static int adapt_of(vn_engine* h, int32_t batch, const char* who, Adapt** ad) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (batch < 0 || batch >= (int)h->batches.size() || !h->batches[batch].set)
    return fail(VN_ESTATE, "batch %d has no interior data (call vn_set_interior first)", batch);
  if (!h->batches[batch].ad) return fail(VN_ESTATE, "%s: batch %d has no adaptive registration (call vn_set_tf_adapt first)", who, batch);
  *ad = h->batches[batch].ad;
  return VN_OK;
}

int vn_get_tf_adapt(vn_engine* h, int32_t batch, float* lambda_host, float* omega_host, float* slots_host, double stats[6]) {
  Adapt* ad = nullptr;
  if (int rc = adapt_of(h, batch, "vn_get_tf_adapt", &ad)) return rc;
  if (slots_host && ad->rule != VN_ADAPT_SA) return fail(VN_EINVAL, "vn_get_tf_adapt: batch %d runs the rba rule, which has no slots", batch);
  return adapt_get(h, *ad, lambda_host, omega_host, slots_host, nullptr, nullptr, stats);
}

int vn_set_tf_adapt_state(vn_engine* h, int32_t batch, const float* lambda_host, const float* slots_host, int64_t tau) {
  Adapt* ad = nullptr;
  if (int rc = adapt_of(h, batch, "vn_set_tf_adapt_state", &ad)) return rc;
  char subject[32];
  snprintf(subject, sizeof subject, "batch %d", batch);
  if (int rc = adapt_put(h, *ad, "vn_set_tf_adapt_state", subject, lambda_host, slots_host, tau)) return rc;
  lbfgs_invalidate(h, batch);
  return VN_OK;
}

// ---- weights on the BC/IC rows (vn_bicadapt.hip): static (vn_set_bic_weights) or self-adaptive (vn_set_bic_adapt), per part ----
static const char* const kBicPart[2] = {"bc", "ic"};
// ... as the messages of adapt_make and adapt_put name a part, its rows and its values
static const char* const kBicThePart[2] = {"the bc part", "the ic part"};
static const char* const kBicRows[2] = {"bc rows", "ic rows"};
static const char* const kBicWeights[2] = {"weight(s) of the bc part", "weight(s) of the ic part"};
static const char* const kBicLambdas[2] = {"initial lambda(s) of the bc part", "initial lambda(s) of the ic part"};

// What both registrations check before they build a state
static int bicw_common(vn_engine* h, const char* who) {
  if (h->nB <= 0) return fail(VN_ESTATE, "%s: no BC/IC rows are registered (call vn_set_bic first)", who);
  if (h->route == Route::layered || !vn_net_in_kernel_range(h->net))
    return fail(VN_EUNSUPPORTED, "%s needs a network of the hand-written kernels (<= %d hidden layers, width <= %d, <= %d inputs, one "
                "activation): the rows' own pass runs on the generic kernels; this one (%d layers, widest %d, %d inputs%s) runs on the "
                "layer-by-layer route or the deep fused kernel only", who, VN_KMAX_LAYERS, VN_KMAX_WIDTH, VN_KMAX_DIN, h->net.L,
                h->net.hmax, h->net.d_in, h->net.act == VN_ACT_PER_LAYER ? ", mixed activations" : "");
  if (h->route == Route::fused4)
    return fail(VN_EUNSUPPORTED, "%s is not built for VN_KERNEL_FUSED (the 4-wave cross-check geometry); every other kernel family "
                                 "carries the rows' own pass", who);
  if (int rc = bicw_check(h, who)) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  const long need = vn_adapt_stride(h->bDof) + vn_adapt_stride(h->nB - h->bDof);
  if (need > h->bw_field_cap) {
    if (int rc = ensure(&h->bw_field, &h->bw_field_cap, need)) return rc;
    HIPCHK(hipMemsetAsync(h->bw_field, 0, (size_t)need * sizeof(float), h->stream));
  }
  return VN_OK;
}

int vn_set_bic_weights(vn_engine* h, const float* omega_dev, int32_t normalize) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (!omega_dev) {                                  // clear: both parts, whatever they hold
    if (!bicw_on(h)) return VN_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (Adapt*& ad : h->bw) adapt_free(ad);
    lbfgs_invalidate(h);
    return VN_OK;
  }
  if (normalize != 0 && normalize != 1) return fail(VN_EINVAL, "vn_set_bic_weights: normalize = %d must be 0 or 1", normalize);
  (void)hipGetLastError();
  if (int rc = bicw_common(h, "vn_set_bic_weights")) return rc;
  Adapt* made[2] = {nullptr, nullptr};
  // a state that never moves: lambda = the caller's omega, m(x) = x (power 1), Z = its mean over the part (normalize) or 1
  const double par[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, (double)normalize, 1.0, 0.0};
  for (int s = 0; s < 2; ++s) {
    if (bicw_count(h, s) <= 0) continue;
    if (int rc = adapt_make(h, "vn_set_bic_weights", kBicRows[s], kBicWeights[s], bicw_count(h, s), VN_ADAPT_NONE, par,
                            omega_dev + (s ? h->bDof : 0), &made[s])) {
      adapt_free(made[0]);
      return rc;                                     // the rows keep what they had
    }
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int s = 0; s < 2; ++s) { adapt_free(h->bw[s]); h->bw[s] = made[s]; }   // replaces a static or an adaptive registration
  lbfgs_invalidate(h);
  return VN_OK;
}

int vn_set_bic_adapt(vn_engine* h, int32_t part, int32_t rule, const double par[10], const float* lambda_init_dev) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (part != 0 && part != 1) return fail(VN_EINVAL, "vn_set_bic_adapt: part = %d is neither 0 (bc) nor 1 (ic)", part);
  if (rule == VN_ADAPT_NONE) {                       // clear this part
    if (!h->bw[part]) return VN_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    adapt_free(h->bw[part]);
    lbfgs_invalidate(h);
    return VN_OK;
  }
  if (int rc = adapt_check_par("vn_set_bic_adapt", rule, par)) return rc;
  if (is_lbfgs(h))
    return fail(VN_EUNSUPPORTED, "vn_set_bic_adapt on an L-BFGS engine: the weights move from step to step but are held constant for the "
                                 "gradient, so an Armijo test across steps means nothing; static weights (vn_set_bic_weights) work");
  (void)hipGetLastError();
  if (int rc = bicw_common(h, "vn_set_bic_adapt")) return rc;
  if (bicw_count(h, part) <= 0)
    return fail(VN_ESTATE, "vn_set_bic_adapt: the %s part has no rows (nB = %ld, bDof = %ld%s)", kBicPart[part], h->nB, h->bDof,
                h->cfg.time_dependent ? "" : ", a steady engine has no initial rows");
  Adapt* ad = nullptr;
  if (int rc = adapt_make(h, "vn_set_bic_adapt", kBicRows[part], kBicLambdas[part], bicw_count(h, part), rule, par, lambda_init_dev, &ad))
    return rc;
  adapt_free(h->bw[part]);                           // replaces a static or an earlier adaptive registration of this part
  h->bw[part] = ad;
  lbfgs_invalidate(h);
  return VN_OK;
}

static int bicw_of(vn_engine* h, int32_t part, const char* who, Adapt** ad) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (part != 0 && part != 1) return fail(VN_EINVAL, "%s: part = %d is neither 0 (bc) nor 1 (ic)", who, part);
  if (!h->bw[part])
    return fail(VN_ESTATE, "%s: the %s part has no registration (call vn_set_bic_weights or vn_set_bic_adapt first)", who, kBicPart[part]);
  *ad = h->bw[part];
  return VN_OK;
}

int vn_get_bic_adapt(vn_engine* h, int32_t part, float* lambda_host, float* omega_host, float* slots_host, float* lossfield_host,
                     double stats[6]) {
  Adapt* ad = nullptr;
  if (int rc = bicw_of(h, part, "vn_get_bic_adapt", &ad)) return rc;
  if (slots_host && ad->rule != VN_ADAPT_SA)
    return fail(VN_EINVAL, "vn_get_bic_adapt: the %s part runs no sa rule, so it has no slots", kBicPart[part]);
  return adapt_get(h, *ad, lambda_host, omega_host, slots_host, bicw_field(h, part), lossfield_host, stats);
}

int vn_set_bic_adapt_state(vn_engine* h, int32_t part, const float* lambda_host, const float* slots_host, int64_t tau) {
  Adapt* ad = nullptr;
  if (int rc = bicw_of(h, part, "vn_set_bic_adapt_state", &ad)) return rc;
  if (ad->rule == VN_ADAPT_NONE)
    return fail(VN_ESTATE, "vn_set_bic_adapt_state: the %s part holds static weights (vn_set_bic_weights), which have no state to set",
                kBicPart[part]);
  if (int rc = adapt_put(h, *ad, "vn_set_bic_adapt_state", kBicThePart[part], lambda_host, slots_host, tau)) return rc;
  lbfgs_invalidate(h);
  return VN_OK;
}

int vn_set_bic(vn_engine* h, const float* biInput, const float* biLabel, int64_t nB, int64_t bDof, double biDimVal) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (nB < 0 || bDof < 0 || bDof > nB) return fail(VN_EINVAL, "need 0 <= bDof <= nB");
  if (nB > 0 && (!biInput || !biLabel)) return fail(VN_EINVAL, "null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  // a steady problem has no initial condition (TFModel.py:646-650): rows behind bDof are never part of its loss
  h->nBreg = nB;
  h->bicB = nullptr; h->bicJ = 0;                    // the shared set's basis goes with it (vn_set_bic_basis)
  h->az_bic = Ansatz();                              // ... and its ansatz streams (vn_set_ansatz_rows)
  if (bicw_on(h)) {                                  // ... and the rows' weights (vn_set_bic_weights, vn_set_bic_adapt)
    HIPCHK(hipStreamSynchronize(h->stream));
    for (Adapt*& ad : h->bw) adapt_free(ad);
  }
  if (!h->cfg.time_dependent) nB = bDof;
  h->biInput = biInput; h->biLabel = biLabel; h->nB = nB; h->bDof = bDof; h->biDimVal = biDimVal;
  lbfgs_invalidate(h);
  if (nB > h->work_b) {
    long c0 = h->work_b, c1 = h->work_b;
    if (int rc = ensure(&h->ub, &c0, nB)) return rc;
    if (int rc = ensure(&h->ubar_b, &c1, nB)) return rc;
    h->work_b = nB;
  }
  return VN_OK;
}

int vn_set_flux_bc(vn_engine* h, const float* X, const float* normal, const float* coef, const float* label, int64_t nF,
                   double biDimVal) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (nF < 0) return fail(VN_EINVAL, "negative number of flux rows");
  edge_drop(h, VN_EDGE_FLUX);
  h->fcoef = h->flabel = nullptr;
  h->fbcS = nullptr; h->fbcJl = h->fbcJc = 0;        // the rows' basis goes with them (vn_set_fluxbc_basis)
  if (nF == 0 || !X) return VN_OK;
  if (!normal || !coef || !label) return fail(VN_EINVAL, "null argument");
  if (int rc = edge_check_route(h, VN_EDGE_FLUX)) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = edge_alloc(h, VN_EDGE_FLUX, nF, nF, true)) return rc;
  EdgeSet& e = h->es[VN_EDGE_FLUX];
  e.X = X; e.G = normal; e.count = nF;
  h->fcoef = coef; h->flabel = label; h->fbiDimVal = biDimVal;
  return VN_OK;
}

int vn_set_periodic(vn_engine* h, const float* X, const float* dir, int64_t nP, double gamma, double biDimVal) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (nP < 0) return fail(VN_EINVAL, "negative number of periodic pairs");
  edge_drop(h, VN_EDGE_PERIODIC);
  if (nP == 0 || !X) return VN_OK;
  if (!dir) return fail(VN_EINVAL, "null argument");
  if (!(gamma >= 0.0) || !std::isfinite(gamma))
    return fail(VN_EINVAL, "periodic pairs: the derivative weight gamma = %g must be finite and >= 0", gamma);
  if (int rc = edge_check_route(h, VN_EDGE_PERIODIC)) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  const bool deriv = gamma > 0.0;                     // gamma == 0: no tangent stream, no derivative seed
  if (int rc = edge_alloc(h, VN_EDGE_PERIODIC, 2 * nP, nP, deriv)) return rc;
  EdgeSet& e = h->es[VN_EDGE_PERIODIC];
  e.X = X; e.G = deriv ? dir : nullptr; e.count = nP;
  h->pgamma = gamma; h->pbiDimVal = biDimVal;
  return VN_OK;
}

int vn_set_observations(vn_engine* h, const float* X, const float* q, const float* dir, const int32_t* rowptr, const float* value,
                        const float* wgt, int64_t n, int64_t nO, double lambda) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (n < 0 || nO < 0) return fail(VN_EINVAL, "negative number of observations or of observed points");
  edge_drop(h, VN_EDGE_OBS);
  h->oQ = h->oval = h->owgt = nullptr;
  h->orowptr = nullptr;
  if (nO == 0) return VN_OK;
  if (!X || !value) return fail(VN_EINVAL, "null argument");
  if (!(lambda >= 0.0) || !std::isfinite(lambda))
    return fail(VN_EINVAL, "observations: the weight lambda = %g must be finite and >= 0", lambda);
  if (n > 0x7fffffffL) return fail(VN_EINVAL, "observations: %lld points exceed the 32-bit row pointers", (long long)n);
  if (!rowptr && n != nO)
    return fail(VN_EINVAL, "observations: point sensors (rowptr == NULL) have one point each, but n = %lld and nO = %lld",
                (long long)n, (long long)nO);
  if (n < nO) return fail(VN_EINVAL, "observations: %lld points cannot fill %lld non-empty segments", (long long)n, (long long)nO);
  if (int rc = edge_check_route(h, VN_EDGE_OBS)) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  // rowptr indexes device memory in the seed kernel: validated once, here (a registration call may synchronise), so that an
  // inconsistent registration is an error code and never a GPU fault.  The reads assume nO + 1 entries of rowptr.
  int bad = 0;
  auto check = [&](int* err_dev) { return vn_obs_check_launch(q, dir, rowptr, value, wgt, n, nO, h->cfg.dim, err_dev, h->stream); };
  if (int rc = count_on_device(h, check, &bad)) return rc;
  if (bad)
    return fail(VN_EINVAL, "inconsistent observations: %d violation(s) (need rowptr[0] = 0 < rowptr[1] < ... < rowptr[nO] = n, no empty "
                           "segment; value finite; wgt finite and >= 0; q and dir finite)", bad);
  if (int rc = edge_alloc(h, VN_EDGE_OBS, n, nO, dir != nullptr)) return rc;   // no directions: no tangent stream, no derivative seed
  if (!h->omisfit) {
    HIPCHK(hipMalloc((void**)&h->omisfit, sizeof(double)));
    HIPCHK(hipMemsetAsync(h->omisfit, 0, sizeof(double), h->stream));
  }
  EdgeSet& e = h->es[VN_EDGE_OBS];
  e.X = X; e.G = dir; e.count = nO;
  h->oQ = q; h->orowptr = rowptr; h->oval = value; h->owgt = wgt; h->olambda = lambda;
  return VN_OK;
}

int vn_set_obs_weight(vn_engine* h, double lambda) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (!(lambda >= 0.0) || !std::isfinite(lambda))
    return fail(VN_EINVAL, "observations: the weight lambda = %g must be finite and >= 0", lambda);
  if (lambda != h->olambda) lbfgs_invalidate(h);     // another objective: (f_k, g_k) and the ring are stale
  h->olambda = lambda;
  return VN_OK;
}

int vn_get_obs_misfit(vn_engine* h, double* misfit) {
  if (!h || !misfit) return fail(VN_EINVAL, "null argument");
  if (h->es[VN_EDGE_OBS].count <= 0) return fail(VN_ESTATE, "vn_get_obs_misfit: no observations are registered (vn_set_observations)");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipMemcpyAsync(misfit, h->omisfit, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VN_OK;
}

// ---- hard-constraint ansatz (vn_ansatz.hip): the three registrations ----
int vn_set_ansatz(vn_engine* h, int32_t batch, const float* A, const float* B, const float* a, const float* b_) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (batch < 0 || batch >= (int)h->batches.size() || !h->batches[batch].set)
    return fail(VN_ESTATE, "batch %d has no interior data (call vn_set_interior first)", batch);
  Batch& b = h->batches[batch];
  lbfgs_invalidate(h, batch);
  b.az = Ansatz();                                   // a call replaces the previous registration, also when it fails
  if (!A && !B && !a && !b_) return VN_OK;
  if (!B) return fail(VN_EINVAL, "vn_set_ansatz: B_dev is required (u = A + B n; all four NULL clears the registration)");
  if (b.n_k <= 0) return fail(VN_EINVAL, "batch %d has no interior rows: no ansatz to apply", batch);
  if (int rc = ansatz_check_route(h)) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  Ansatz z;
  z.A = A; z.B = B; z.a = a; z.b = b_;
  const long nT = b.n_k * h->cfg.integ_num;
  if (int rc = ansatz_check_finite(h, "vn_set_ansatz", z, nT, nT)) return rc;
  b.az = z;
  return VN_OK;
}

int vn_set_ansatz_points(vn_engine* h, int32_t batch, const float* Au, const float* Bu, const float* gAu, const float* gBu) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (batch < 0 || batch >= (int)h->batches.size() || !h->batches[batch].set)
    return fail(VN_ESTATE, "batch %d has no interior data (call vn_set_interior first)", batch);
  Batch& b = h->batches[batch];
  lbfgs_invalidate(h, batch);
  b.azp = Ansatz();
  if (!Au && !Bu && !gAu && !gBu) return VN_OK;
  if (!b.Xu) return fail(VN_ESTATE, "vn_set_ansatz_points: batch %d has no de-duplication map (call vn_set_dedup first)", batch);
  if (!Bu) return fail(VN_EINVAL, "vn_set_ansatz_points: Bu_dev is required (all four NULL clears the registration)");
  if (h->cfg.dim > 3) return fail(VN_EINVAL, "vn_set_ansatz_points: the point record holds dim <= 3 gradient entries (dim = %d)", h->cfg.dim);
  if (int rc = ansatz_check_route(h)) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  Ansatz z;
  z.A = Au; z.B = Bu; z.a = gAu; z.b = gBu;
  if (int rc = ansatz_check_finite(h, "vn_set_ansatz_points", z, b.U, b.U * h->cfg.dim)) return rc;
  b.azp = z;
  return VN_OK;
}

int vn_set_ansatz_rows(vn_engine* h, int32_t set, const float* A, const float* B, const float* a, const float* b_) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (set < VN_ANSATZ_BIC || set > VN_ANSATZ_OBS)
    return fail(VN_EINVAL, "vn_set_ansatz_rows: set %d is none of VN_ANSATZ_BIC, VN_ANSATZ_FLUX, VN_ANSATZ_PERIODIC, VN_ANSATZ_OBS", set);
  Ansatz& slot = set == VN_ANSATZ_BIC ? h->az_bic : h->az_edge[set - VN_ANSATZ_FLUX];
  lbfgs_invalidate(h);
  slot = Ansatz();
  if (!A && !B && !a && !b_) return VN_OK;
  // rows as the caller counts them, and whether the set has a direction to differentiate along
  long rows = 0;
  bool deriv = false;
  if (set == VN_ANSATZ_BIC) rows = h->nBreg;
  else { const EdgeSet& e = h->es[set - VN_ANSATZ_FLUX]; rows = e.count > 0 ? e.rows : 0; deriv = e.G != nullptr; }
  if (rows <= 0) return fail(VN_ESTATE, "vn_set_ansatz_rows: %s are not registered", kAnsatzSet[set]);
  if (!B) return fail(VN_EINVAL, "vn_set_ansatz_rows: B_dev is required (all four NULL clears the registration)");
  if (!deriv && (a || b_))
    return fail(VN_EINVAL, "vn_set_ansatz_rows: %s have no direction, so a_dev and b_dev (the derivatives of A and B along it) must be NULL",
                kAnsatzSet[set]);
  if (set == VN_ANSATZ_BIC)
    for (size_t i = 0; i < h->batches.size(); ++i)
      if (h->batches[i].biInput)
        return fail(VN_EUNSUPPORTED, "vn_set_ansatz_rows(VN_ANSATZ_BIC) next to batch %zu's own copy of the BC/IC rows (vn_set_batch_bic): "
                                     "the streams belong to the rows of vn_set_bic", i);
  if (set == VN_ANSATZ_BIC && bicw_on(h))
    return fail(VN_EUNSUPPORTED, "vn_set_ansatz_rows(VN_ANSATZ_BIC) next to weights on the BC/IC rows (vn_set_bic_weights / vn_set_bic_adapt): "
                                 "under a hard-constraint ansatz the rows' error is zero by construction, there is nothing to weight");
  if (int rc = ansatz_check_route(h)) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  Ansatz z;
  z.A = A; z.B = B; z.a = a; z.b = b_;
  if (int rc = ansatz_check_finite(h, "vn_set_ansatz_rows", z, rows, rows)) return rc;
  slot = z;
  return VN_OK;
}

int vn_set_batch_bic(vn_engine* h, int32_t batch, const float* biInput, const float* biLabel) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (batch < 0 || batch >= (int)h->batches.size() || !h->batches[batch].set)
    return fail(VN_ESTATE, "batch %d has no interior data (call vn_set_interior first)", batch);
  if ((biInput == nullptr) != (biLabel == nullptr)) return fail(VN_EINVAL, "biInput and biLabel must be given together");
  if (biInput && h->az_bic.B)
    return fail(VN_EUNSUPPORTED, "vn_set_batch_bic next to BC/IC ansatz streams (vn_set_ansatz_rows): the streams belong to the rows of "
                                 "vn_set_bic, a batch's own copy of the rows would be evaluated with them");
  if (biInput && bicw_on(h))
    return fail(VN_EUNSUPPORTED, "vn_set_batch_bic next to weights on the BC/IC rows (vn_set_bic_weights / vn_set_bic_adapt): the weights "
                                 "belong to the rows of vn_set_bic, one state per row");
  h->batches[batch].biInput = biInput;
  h->batches[batch].biLabel = biLabel;
  h->batches[batch].bb_B = nullptr; h->batches[batch].bb_J = 0;     // the copy's basis goes with it (vn_set_bic_basis)
  lbfgs_invalidate(h, batch);
  return VN_OK;
}

int vn_set_reparam(vn_engine* h, int32_t mode, int32_t granularity, double n, const double* s_init, int32_t S, double lr) {
  if (!h) return fail(VN_EINVAL, "null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (mode == VN_REPARAM_NONE) {          // theta keeps its effective values; m and v are the slots of theta again
    if (reparam_on(h)) {
      HIPCHK(hipStreamSynchronize(h->stream));
      reparam_free(h);
      h->snap_step = -1;
    }
    return VN_OK;
  }
  if (mode != VN_REPARAM_RWF && mode != VN_REPARAM_SLOPE) return fail(VN_EINVAL, "vn_set_reparam: unknown mode %d", mode);
  if (mode == VN_REPARAM_SLOPE && granularity != VN_REPARAM_PER_NEURON && granularity != VN_REPARAM_PER_LAYER)
    return fail(VN_EINVAL, "vn_set_reparam: unknown granularity %d", granularity);
  if (h->cfg.optimizer != VN_OPT_ADAM)
    return fail(VN_EUNSUPPORTED, "vn_set_reparam on %s engine: its optimizer state would live in theta_eff space; the joint step on "
                                 "(V, s) is built for Adam", is_lbfgs(h) ? "an L-BFGS" : "an RMSProp");
  if (h->comm)
    return fail(VN_EUNSUPPORTED, "vn_set_reparam under a communicator: the scales' gradient is formed from each rank's own V after the "
                                 "all-reduce, a route that is not built");
  const VnNet& net = h->net;
  if (h->route == Route::layered || net.L + 1 > VN_RP_MAX_LAYERS || net.hmax > VN_RP_MAX_WIDTH || net.d_in > VN_KMAX_DIN ||
      net.act == VN_ACT_PER_LAYER)
    return fail(VN_EUNSUPPORTED, "vn_set_reparam needs a network of the fused / generic kernels (at most 8 hidden layers, widths <= %d, "
                                 "d_in <= %d, one activation); this one (%d layers, widest %d, %d inputs) runs layer by layer",
                VN_RP_MAX_WIDTH, VN_KMAX_DIN, net.L, net.hmax, net.d_in);
  if (!s_init) return fail(VN_EINVAL, "vn_set_reparam: s_init is NULL");
  if (!(lr >= 0.0) || !std::isfinite(lr)) return fail(VN_EINVAL, "vn_set_reparam: the scales' learning rate must be finite and >= 0");
  if (mode == VN_REPARAM_SLOPE && (!(n >= 1.0) || !std::isfinite(n)))
    return fail(VN_EINVAL, "vn_set_reparam: the slope factor n must be finite and >= 1 (got %g)", n);
  VnReparamArgs lay;
  std::vector<int> group;
  const int need = reparam_layout(net, mode, granularity, lay, group);
  if (S != need) return fail(VN_EINVAL, "vn_set_reparam: this mode has %d scales on this network, got S = %d", need, S);
  std::vector<float> s32((size_t)S);
  for (int i = 0; i < S; ++i) {
    s32[i] = (float)s_init[i];
    if (!std::isfinite(s_init[i]) || !std::isfinite(s32[i])) return fail(VN_EINVAL, "vn_set_reparam: s_init[%d] is not finite", i);
    if (mode == VN_REPARAM_SLOPE && s32[i] == 0.f) return fail(VN_EINVAL, "vn_set_reparam: s_init[%d] == 0 (a zero slope cannot be factorised)", i);
  }
  if (reparam_on(h)) { HIPCHK(hipStreamSynchronize(h->stream)); reparam_free(h); }     // theta holds the effective values
  h->snap_step = -1;
  vn_engine::Reparam& r = h->rp;
  const size_t P = (size_t)net.P;
  hipError_t a = hipMalloc((void**)&r.V, P * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&r.sc, 4 * (size_t)S * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&r.snap, (P + 4 * (size_t)S) * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&r.gout, (P + (size_t)S) * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&r.group, P * sizeof(int));
  if (a == hipSuccess) a = hipMemcpyAsync(r.group, group.data(), P * sizeof(int), hipMemcpyHostToDevice, h->stream);
  if (a == hipSuccess) a = hipMemsetAsync(r.sc, 0, 4 * (size_t)S * sizeof(float), h->stream);
  if (a == hipSuccess) a = hipMemcpyAsync(r.sc, s32.data(), (size_t)S * sizeof(float), hipMemcpyHostToDevice, h->stream);
  if (a != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(h->stream);
    reparam_free(h);
    return fail(VN_ENOMEM, "vn_set_reparam: device allocation failed: %s", hipGetErrorString(a));
  }
  lay.n = n;
  lay.theta = h->theta; lay.V = r.V; lay.m = h->m; lay.v = h->v;
  lay.s = r.sc; lay.ms = r.sc + S; lay.vs = r.sc + 2 * (size_t)S; lay.f = r.sc + 3 * (size_t)S;
  lay.gV = r.gout; lay.gs = r.gout + P;
  r.lay = lay;
  r.S = S; r.gran = granularity; r.n = n; r.lr = lr;
  r.s_init = s32;
  r.mode = mode;
  if (int rc = reparam_factorise(h)) { (void)hipStreamSynchronize(h->stream); reparam_free(h); return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));          // (group and s32 are host vectors of this call)
  return VN_OK;
}

int vn_get_reparam(vn_engine* h, float* V_host, float* s_host, float* f_host, float* slots_host) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (!reparam_on(h)) return fail(VN_ESTATE, "vn_get_reparam: no weight scales are registered (vn_set_reparam)");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t S = (size_t)h->rp.S;
  if (V_host) HIPCHK(hipMemcpyAsync(V_host, h->rp.V, (size_t)h->net.P * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (s_host) HIPCHK(hipMemcpyAsync(s_host, h->rp.sc, S * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (slots_host) HIPCHK(hipMemcpyAsync(slots_host, h->rp.sc + S, 2 * S * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (f_host) HIPCHK(hipMemcpyAsync(f_host, h->rp.sc + 3 * S, S * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VN_OK;
}

int vn_set_reparam_state(vn_engine* h, const float* V_host, const float* s_host, const float* slots_host) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (!reparam_on(h)) return fail(VN_ESTATE, "vn_set_reparam_state: no weight scales are registered (vn_set_reparam)");
  const size_t S = (size_t)h->rp.S;
  if (s_host)
    for (size_t i = 0; i < S; ++i)
      if (!std::isfinite(s_host[i])) return fail(VN_EINVAL, "vn_set_reparam_state: s[%d] is not finite", (int)i);
  HIPCHK(hipSetDevice(h->cfg.device));
  h->snap_step = -1;
  if (V_host) HIPCHK(hipMemcpyAsync(h->rp.V, V_host, (size_t)h->net.P * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if (s_host) HIPCHK(hipMemcpyAsync(h->rp.sc, s_host, S * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if (slots_host) HIPCHK(hipMemcpyAsync(h->rp.sc + S, slots_host, 2 * S * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(vn_reparam_rebuild_launch(h->rp.lay, h->rp.group, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  lbfgs_invalidate(h);
  return VN_OK;
}

int vn_reparam_grad(vn_engine* h, float* gV_host, float* gs_host) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (!reparam_on(h)) return fail(VN_ESTATE, "vn_reparam_grad: no weight scales are registered (vn_set_reparam)");
  HIPCHK(hipSetDevice(h->cfg.device));
  VnReparamArgs a = h->rp.lay;
  a.g = h->gradbuf;
  HIPCHK(vn_reparam_grad_launch(a, h->stream));
  if (gV_host) HIPCHK(hipMemcpyAsync(gV_host, a.gV, (size_t)h->net.P * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (gs_host) HIPCHK(hipMemcpyAsync(gs_host, a.gs, (size_t)h->rp.S * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VN_OK;
}

int vn_set_weights(vn_engine* h, const double w[3]) {
  if (!h || !w) return fail(VN_EINVAL, "null argument");
  h->w[0] = w[0]; h->w[1] = w[1]; h->w[2] = w[2];   // (VN_OPT_LBFGS: vn_lbfgs_step compares them with those of its (f_k, g_k))
  return VN_OK;
}

int vn_bind_grad_buffer(vn_engine* h, float* dev) {
  if (!h) return fail(VN_EINVAL, "null handle");
  h->gradbuf = dev ? dev : h->gradbuf_int;
  return VN_OK;
}

static int grad_route(vn_engine* h, const Batch& b);

int vn_grad(vn_engine* h, int32_t batch) {
  if (!h) return fail(VN_EINVAL, "null handle");
  (void)hipGetLastError();   // a stale last-error of another library on this thread is not ours to report
  if (int rc = check_batch(h, batch)) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  const Batch& b = h->batches[batch];
  if (int rc = ansatz_check_eval(h, b, batch)) return rc;
  if (bicw_on(h))
    if (int rc = bicw_check(h, "weights on the BC/IC rows (vn_set_bic_weights / vn_set_bic_adapt)")) return rc;
  const LearntKind* learnt = learnt_any(h);
  if (learnt && has_ansatz(b))
    return fail(VN_EUNSUPPORTED, "learnt %s (%s) next to a hard-constraint ansatz (vn_set_ansatz, batch %d): the %s sums next to the "
                                 "ansatz stage are not built", learnt->what, learnt->setter, batch, learnt->noun);
  if (!learnt) return grad_route(h, b);
  if (has_weights(b)) return learnt_weights_refusal(*learnt, batch);
  if (int rc = source_mix(h, b, batch)) return rc;
  if (int rc = field_mix(h, b, batch)) return rc;
  if (int rc = bic_mix(h, b, batch)) return rc;
  if (int rc = fluxbc_mix(h)) return rc;
  for (Learnt& v : h->lv) v.blocks = 0;
  if (int rc = grad_route(h, b)) return rc;
  // after every kernel that reads the coefficients, s_mix or the mixed gcoef (the parameters' update rides in the reduction above);
  // every vector steps on the same counter
  for (int id = 0; id < LV_N; ++id)
    if (h->lv[id].on)
      if (int rc = learnt_finish(h, id, true, h->fuse.kind == VN_OPT_ADAM, (double)h->step)) return rc;
  return VN_OK;
}

static int grad_route(vn_engine* h, const Batch& b) {
  VnEdgeSums fx;
  if (int rc = edge_passes(h, true, &fx)) return rc;   // (no flux rows, no periodic pairs: nothing enqueued, fx empty)
  if (b.Xu) return run_dedup(h, b, h->gradbuf, fx);      // (a de-duplication map: 8-wave routes only)
  switch (h->route) {
    case Route::layered: return run_layered(h, b, h->gradbuf, fx);
    case Route::generic: return run_generic(h, b, h->gradbuf, fx);
    case Route::fused4: return run_fused(h, b, h->gradbuf, fx);
    // a reaction term lives in the row-wise seed kernel, a flux term and a diffusivity D(u) around it: the single-launch route
    // runs the two-pass sequence for such a batch
    // ... and so do per-test-function loss weights, applied after it, and learnt source amplitudes, whose sums read udbar
    // ... and a hard-constraint ansatz, an elementwise stage on either side of it
    case Route::fused8: return has_terms(b) || has_weights(b) || has_ansatz(b) || src_learnt(h, b) || fld_learnt(h, b) ? run_twopass(h, b, h->gradbuf, fx) : run_fused(h, b, h->gradbuf, fx);
    case Route::twopass: return run_twopass(h, b, h->gradbuf, fx);
  }
}

// ---- per-term gradients and their statistics (vn_balance.hip) -------------------------------
static int term_scratch(vn_engine* h, bool with_T) {
  hipError_t a = hipSuccess;
  if (!h->tg_part) a = hipMalloc((void**)&h->tg_part, (size_t)VN_BAL_MAX_BLOCKS * VN_BAL_ROW * sizeof(double));
  if (a == hipSuccess && !h->tg_out) a = hipMalloc((void**)&h->tg_out, (size_t)(VN_BAL_OUT + VN_TERM_N) * sizeof(double));
  if (a == hipSuccess && with_T && !h->tg_T) a = hipMalloc((void**)&h->tg_T, (size_t)VN_TERM_N * (size_t)h->net.P * sizeof(float));
  if (a != hipSuccess) {
    (void)hipGetLastError();
    return fail(VN_ENOMEM, "per-term gradient scratch: device allocation failed: %s", hipGetErrorString(a));
  }
  return VN_OK;
}

int vn_term_stats(vn_engine* h, const float* T_dev, int32_t K, int64_t n, double* stats, double* gram) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (K < 1 || K > VN_TERM_N) return fail(VN_EINVAL, "vn_term_stats: K = %d is outside 1..%d", K, VN_TERM_N);
  if (n < 1) return fail(VN_EINVAL, "vn_term_stats: n = %lld must be at least 1", (long long)n);
  if (!T_dev || !stats || !gram) return fail(VN_EINVAL, "vn_term_stats: null argument");
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = term_scratch(h, false)) return rc;
  HIPCHK(vn_balance_stats_launch(T_dev, K, n, h->tg_part, h->tg_out, h->stream));
  double out[VN_BAL_OUT];
  const size_t nv = (size_t)(3 * K + K * K);
  HIPCHK(hipMemcpyAsync(out, h->tg_out, nv * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::memcpy(stats, out, (size_t)(3 * K) * sizeof(double));
  std::memcpy(gram, out + 3 * K, (size_t)(K * K) * sizeof(double));
  return VN_OK;
}

int vn_term_grads(vn_engine* h, const int32_t* batches, int32_t n, uint32_t term_mask, double* stats, double* gram, double* value,
                  float* G_dev) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (is_lbfgs(h)) return fail(VN_EUNSUPPORTED, "vn_term_grads on an L-BFGS engine: the evaluations would disturb the optimizer's (f_k, g_k)");
  if (h->comm) return fail(VN_EUNSUPPORTED, "vn_term_grads under a communicator: each term's gradient would need its own all-reduce, which is not built");
  if (!batches || n < 1) return fail(VN_EINVAL, "vn_term_grads: the batch list is null or empty");
  if (!stats || !gram || !value) return fail(VN_EINVAL, "vn_term_grads: null output argument");
  if (term_mask == 0 || (term_mask >> VN_TERM_N) != 0)
    return fail(VN_EINVAL, "vn_term_grads: term_mask = 0x%x must have at least one bit and none at or above bit %d", term_mask, VN_TERM_N);
  for (int32_t i = 0; i < n; ++i)
    if (batches[i] < 0 || batches[i] >= (int)h->batches.size() || !h->batches[batches[i]].set)
      return fail(VN_EINVAL, "vn_term_grads: batches[%d] = %d names no registered batch", i, batches[i]);
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = term_scratch(h, true)) return rc;
  const size_t P = (size_t)h->net.P;
  // a term without rows is skipped: its mean is an empty one (vn_reduce_kernel), and so is its gradient
  const bool rows[VN_TERM_N] = {h->bDof > 0 || h->es[VN_EDGE_FLUX].count > 0 || h->es[VN_EDGE_PERIODIC].count > 0, h->nB - h->bDof > 0,
                                true, h->es[VN_EDGE_OBS].count > 0};
  bool on[VN_TERM_N];
  for (int k = 0; k < VN_TERM_N; ++k) on[k] = rows[k] && ((term_mask >> k) & 1u);
  const double w_user[3] = {h->w[0], h->w[1], h->w[2]}, lambda_user = h->olambda;
  double* const val = h->tg_out + VN_BAL_OUT;
  int rc = VN_OK;
  hipError_t e = hipMemsetAsync(val, 0, VN_TERM_N * sizeof(double), h->stream);
  for (int k = 0; k < VN_TERM_N && rc == VN_OK && e == hipSuccess; ++k) {
    float* Tk = h->tg_T + (size_t)k * P;
    if (!on[k]) { e = hipMemsetAsync(Tk, 0, P * sizeof(float), h->stream); continue; }
    for (int j = 0; j < 3; ++j) h->w[j] = j == k ? 1.0 : 0.0;
    h->olambda = k == VN_TERM_OBS ? 1.0 : 0.0;
    for (int32_t i = 0; i < n && rc == VN_OK && e == hipSuccess; ++i) {
      h->ad_quiet = true;       // a probe: committed state, pending state and pending flag of adaptive weights stay as they are
      rc = vn_grad(h, batches[i]);
      h->ad_quiet = false;
      if (rc == VN_OK)
        e = vn_balance_accum_launch(Tk, h->gradbuf, h->net.P, i == 0, val + k, k == VN_TERM_OBS ? nullptr : h->gradbuf + P + 1 + k,
                                    k == VN_TERM_OBS ? h->omisfit : nullptr, h->stream);
    }
  }
  h->w[0] = w_user[0]; h->w[1] = w_user[1]; h->w[2] = w_user[2];
  h->olambda = lambda_user;
  if (rc != VN_OK) { (void)hipStreamSynchronize(h->stream); return rc; }
  HIPCHK(e);
  HIPCHK(vn_balance_stats_launch(h->tg_T, VN_TERM_N, h->net.P, h->tg_part, h->tg_out, h->stream));
  if (G_dev) HIPCHK(hipMemcpyAsync(G_dev, h->tg_T, VN_TERM_N * P * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  double out[VN_BAL_OUT + VN_TERM_N];
  HIPCHK(hipMemcpyAsync(out, h->tg_out, sizeof(out), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  // (a skipped term's row of zeros would still carry a NaN of another term into the Gram matrix: 0 * NaN)
  for (int a = 0; a < VN_TERM_N; ++a) {
    for (int c = 0; c < 3; ++c) stats[a * 3 + c] = on[a] ? out[a * 3 + c] : 0.0;
    for (int b = 0; b < VN_TERM_N; ++b) gram[a * VN_TERM_N + b] = on[a] && on[b] ? out[3 * VN_TERM_N + a * VN_TERM_N + b] : 0.0;
    value[a] = on[a] ? out[VN_BAL_OUT + a] : 0.0;
  }
  return VN_OK;
}

static int apply_impl(vn_engine* h, float* loss_acc) {
  (void)hipGetLastError();   // a stale last-error of another library on this thread is not ours to report
  HIPCHK(hipSetDevice(h->cfg.device));
  // the step counter moves only when the update was launched (a failed call leaves the optimizer state as it found it)
  if (h->cfg.optimizer == VN_OPT_RMSPROP) {
    HIPCHK(vn_rmsprop_launch(h->theta, h->m, h->v, h->gradbuf, h->net.P, (float)h->cfg.lr, 0.9f, 0.0f, 1e-10f, loss_acc,
                             h->stream));
    adapt_commit(h);
    h->step += 1;
    return VN_OK;
  }
  const double t = (double)(h->step + 1);
  const double lr_t = h->cfg.lr * std::sqrt(1.0 - std::pow(h->cfg.beta2, t)) / (1.0 - std::pow(h->cfg.beta1, t));
  if (reparam_on(h)) {         // the joint step on (V, s) and the rebuild of theta_eff, in place of the plain step on theta
    VnReparamArgs a = h->rp.lay;
    a.g = h->gradbuf;
    a.lr_t = (float)lr_t;
    a.lr_s_t = (float)(h->rp.lr * std::sqrt(1.0 - std::pow(h->cfg.beta2, t)) / (1.0 - std::pow(h->cfg.beta1, t)));
    a.b1 = (float)h->cfg.beta1; a.b2 = (float)h->cfg.beta2; a.eps = (float)h->cfg.eps;
    a.loss_acc = loss_acc;
    HIPCHK(vn_reparam_step_launch(a, h->stream));
  } else {
    HIPCHK(vn_adam_launch(h->theta, h->m, h->v, h->gradbuf, h->net.P, (float)lr_t, (float)h->cfg.beta1,
                          (float)h->cfg.beta2, (float)h->cfg.eps, loss_acc, h->stream));
  }
  for (int id = 0; id < LV_N; ++id)
    if (h->lv[id].on)
      if (int rc = learnt_finish(h, id, false, true, t)) return rc;
  adapt_commit(h);              // self-adaptive weights: the pending states of the gradient evaluations this step applies
  h->step += 1;
  return VN_OK;
}

int vn_apply(vn_engine* h) {
  if (!h) return fail(VN_EINVAL, "null handle");
  NOT_LBFGS("vn_apply");
  return apply_impl(h, nullptr);
}

// gradient + optimizer step with the update folded into the gradient reduction (no collective in between)
static int step_fused(vn_engine* h, int32_t batch, float* loss_acc) {
  if (h->comm) {
    // towers: gradient -> SUM over ranks -> update, all on the engine stream, no host round trip.
    // One-rank failure (include/varnet_hip.h, "Failure under a communicator"): this rank returns its error WITHOUT entering
    // the collective and with its optimizer state untouched; its peers' ncclAllReduce for this step never completes, so the
    // caller must end the job -- varnet_amd/launch.py ends the peers of a rank that exits non-zero by PID, within its poll
    // interval, and reports the failing rank's last stage (VNEngine._ck leaves `engine_error: ...` there).
    if (int rc = vn_grad(h, batch)) return rc;
    if (int rc = vn_allreduce_grad(h)) return rc;
    return apply_impl(h, loss_acc);
  }
  if (reparam_on(h)) {          // learnt weight scales: the update is not folded into the reduction (fuse kind -1); the stage follows it
    if (int rc = vn_grad(h, batch)) return rc;
    return apply_impl(h, loss_acc);
  }
  h->step += 1;
  VnOptArgs o;
  o.kind = h->cfg.optimizer; o.theta = h->theta; o.m = h->m; o.v = h->v; o.loss_acc = loss_acc;
  if (h->cfg.optimizer == VN_OPT_RMSPROP) {
    o.lr = (float)h->cfg.lr; o.b1 = 0.9f; o.b2 = 0.0f; o.eps = 1e-10f;          // decay, momentum, epsilon
  } else {
    const double t = (double)h->step;
    o.lr = (float)(h->cfg.lr * std::sqrt(1.0 - std::pow(h->cfg.beta2, t)) / (1.0 - std::pow(h->cfg.beta1, t)));
    o.b1 = (float)h->cfg.beta1; o.b2 = (float)h->cfg.beta2; o.eps = (float)h->cfg.eps;
  }
  h->fuse = o;
  const int rc = vn_grad(h, batch);
  h->fuse = VnOptArgs();
  if (rc) { h->step -= 1; adapt_drop_pending(h); }
  else adapt_commit(h);
  return rc;
}

int vn_train_epoch(vn_engine* h, const int32_t* batches, int32_t n, float* loss_acc_dev) {
  if (!h || (n > 0 && !batches)) return fail(VN_EINVAL, "null argument");
  NOT_LBFGS("vn_train_epoch");
  for (int32_t i = 0; i < n; ++i)
    if (int rc = step_fused(h, batches[i], loss_acc_dev)) return rc;
  return VN_OK;
}

int vn_train_step(vn_engine* h, int32_t batch, float* loss_out_dev) {
  if (!h) return fail(VN_EINVAL, "null handle");
  NOT_LBFGS("vn_train_step");
  if (int rc = step_fused(h, batch, nullptr)) return rc;
  if (loss_out_dev)
    HIPCHK(hipMemcpyAsync(loss_out_dev, h->gradbuf + h->net.P, sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  return VN_OK;
}

// ---- L-BFGS (VN_OPT_LBFGS): one iteration above vn_grad -------------------------------------
static int lbfgs_alloc(vn_engine* h) {
  if (h->lb_alloc) return VN_OK;
  const size_t P = (size_t)h->net.P;
  VnLbfgsBufs& b = h->lb;
  hipError_t a = hipMalloc((void**)&b.ring, 2 * (size_t)VN_LBFGS_SLOTS * P * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&b.theta_k, P * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&b.g_k, (P + 4) * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&b.d, P * sizeof(float));
  if (a == hipSuccess) a = hipMalloc((void**)&b.part, (size_t)VN_LBFGS_MAXBLK * VN_LBFGS_NACC * sizeof(double));
  if (a == hipSuccess) a = hipMalloc((void**)&b.G, (size_t)VN_LBFGS_NB * VN_LBFGS_NB * sizeof(double));
  if (a == hipSuccess) a = hipMalloc((void**)&b.coef, (VN_LBFGS_NB + 1) * sizeof(double));
  if (a == hipSuccess) a = hipMalloc((void**)&b.meta, sizeof(VnLbfgsMeta));
  // host memory the one-wave kernel stores its scalars to, and the landing place of a trial's loss scalars
  if (a == hipSuccess) a = hipHostMalloc((void**)&b.out, sizeof(VnLbfgsOut) + 4 * sizeof(float), hipHostMallocDefault);
  if (a == hipSuccess) a = hipMemsetAsync(b.G, 0, (size_t)VN_LBFGS_NB * VN_LBFGS_NB * sizeof(double), h->stream);
  if (a == hipSuccess) a = hipMemsetAsync(b.meta, 0, sizeof(VnLbfgsMeta), h->stream);
  if (a != hipSuccess) {
    (void)hipGetLastError();
    void* ptrs[] = {b.ring, b.theta_k, b.g_k, b.d, b.part, b.G, b.coef, b.meta};
    for (void* p : ptrs)
      if (p) (void)hipFree(p);
    if (b.out) (void)hipHostFree(b.out);
    b = VnLbfgsBufs{};
    return fail(VN_ENOMEM, "L-BFGS state (%d vectors of %zu parameters) does not fit: %s", 2 * VN_LBFGS_SLOTS + 3, P,
                hipGetErrorString(a));
  }
  memset(b.out, 0, sizeof(VnLbfgsOut) + 4 * sizeof(float));
  h->lb_lossh = (float*)(b.out + 1);
  h->lb_alloc = true;
  return VN_OK;
}

int vn_lbfgs_step(vn_engine* h, int32_t batch, int32_t max_trials, double info[10]) {
  if (!h || !info) return fail(VN_EINVAL, "null argument");
  if (!is_lbfgs(h))
    return fail(VN_ESTATE, "vn_lbfgs_step needs an engine created with optimizer = VN_OPT_LBFGS (this one runs %s)",
                h->cfg.optimizer == VN_OPT_RMSPROP ? "RMSProp" : "Adam");
  if (h->comm)
    return fail(VN_EUNSUPPORTED, "vn_lbfgs_step under a communicator: every rank would have to take the same accept decision "
                                 "from an all-reduced loss, which is not built");
  if (max_trials < 1) return fail(VN_EINVAL, "max_trials must be at least 1");
  (void)hipGetLastError();
  if (int rc = check_batch(h, batch)) return rc;
  if (h->batches[batch].wt.S > 0)
    return fail(VN_EUNSUPPORTED, "vn_lbfgs_step on batch %d, which has a causal registration (vn_set_causal): its weights move with "
                                 "the parameters but are held constant for the gradient, so the search direction is not the gradient "
                                 "of the reported loss and an Armijo test on it means nothing; static weights (vn_set_tf_weights) work",
                batch);
  if (h->batches[batch].ad)
    return fail(VN_EUNSUPPORTED, "vn_lbfgs_step on batch %d, which has an adaptive registration (vn_set_tf_adapt): its weights move from "
                                 "step to step but are held constant for the gradient, so an Armijo test across steps means nothing; "
                                 "static weights (vn_set_tf_weights) work", batch);
  for (const Adapt* ad : h->bw)
    if (ad && ad->rule != VN_ADAPT_NONE)
      return fail(VN_EUNSUPPORTED, "vn_lbfgs_step next to an adaptive registration on the BC/IC rows (vn_set_bic_adapt): its weights move "
                                   "from step to step but are held constant for the gradient, so an Armijo test across steps means "
                                   "nothing; static weights (vn_set_bic_weights) work");
  if (h->lb_loss64 && has_ansatz(h->batches[batch]))
    return fail(VN_EUNSUPPORTED, "vn_lbfgs_step with vn_lbfgs_loss64 on batch %d, which has a hard-constraint ansatz (vn_set_ansatz): the "
                                 "fp64 objective does not carry the ansatz stage", batch);
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = lbfgs_alloc(h)) return rc;
  const long P = h->net.P;
  const VnLbfgsBufs& b = h->lb;
  const size_t nb4 = 4 * sizeof(float);
  if (batch != h->lb_batch) { lbfgs_invalidate(h); h->lb_batch = batch; }
  // weights: what counts is the objective this call sees (train()'s monitors set unit weights and put the run's back)
  if (h->w[0] != h->lb_w[0] || h->w[1] != h->lb_w[1] || h->w[2] != h->lb_w[2]) lbfgs_invalidate(h);
  if (!h->lb_valid) {                       // an evaluation, not a trial
    if (int rc = vn_grad(h, batch)) return rc;
    HIPCHK(vn_lbfgs_commit_launch(b, h->theta, h->gradbuf, P, 1, h->stream));
    HIPCHK(hipMemcpyAsync(h->lb_lossh, h->gradbuf + P, nb4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < 4; ++i) h->lb_f[i] = (double)h->lb_lossh[i];
    if (h->lb_loss64)
      if (int rc = vn_objective_f64(h, batch, nullptr, nullptr, nullptr, h->lb_f)) return rc;
    for (int i = 0; i < 3; ++i) h->lb_w[i] = h->w[i];
    h->lb_valid = true;
    h->lb_reset = true;
  }
  const int reset = h->lb_reset ? 1 : 0;
  HIPCHK(vn_lbfgs_gram_launch(b, P, reset, h->stream));
  HIPCHK(vn_lbfgs_twoloop_launch(b, P, reset, h->stream));
  h->lb_reset = false;
  const double fk = h->lb_f[0];
  double scale = 1.0, t = 0.0, f[4] = {0, 0, 0, 0};
  int used = 0;
  bool accepted = false;
  for (int j = 0; j < max_trials && !accepted; ++j, scale *= 0.5) {
    HIPCHK(vn_lbfgs_trial_launch(b, h->theta, P, scale, j == 0, h->stream));
    int rc = vn_grad(h, batch);
    if (rc == VN_OK) {
      hipError_t e = hipMemcpyAsync(h->lb_lossh, h->gradbuf + P, nb4, hipMemcpyDeviceToHost, h->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
      if (e != hipSuccess) rc = fail(VN_EHIP, "vn_lbfgs_step: %s", hipGetErrorString(e));
    }
    double f64[4] = {0, 0, 0, 0};
    if (rc == VN_OK && h->lb_loss64) rc = vn_objective_f64(h, batch, nullptr, nullptr, nullptr, f64);   // at the trial point
    if (rc != VN_OK) {                      // theta goes back to theta_k; the message is the failed call's
      (void)hipMemcpyAsync(h->theta, b.theta_k, (size_t)P * sizeof(float), hipMemcpyDeviceToDevice, h->stream);
      (void)hipStreamSynchronize(h->stream);
      return rc;
    }
    used = j + 1;
    t = b.out->t0 * scale;
    for (int i = 0; i < 4; ++i) f[i] = h->lb_loss64 ? f64[i] : (double)h->lb_lossh[i];
    accepted = std::isfinite(f[0]) && f[0] <= fk + 1e-4 * t * b.out->gd;
  }
  const double pairs = b.out->pairs;
  info[1] = fk; info[7] = (double)used; info[8] = b.out->gd; info[9] = pairs;
  if (accepted) {
    HIPCHK(vn_lbfgs_commit_launch(b, h->theta, h->gradbuf, P, 0, h->stream));
    h->step += 1;
    for (int i = 0; i < 4; ++i) h->lb_f[i] = f[i];
    info[0] = 0.0; info[2] = f[0]; info[3] = f[1]; info[4] = f[2]; info[5] = f[3]; info[6] = t;
    return VN_OK;
  }
  // no trial accepted: theta_k back bit for bit; with pairs the next call is a steepest-descent iteration, without: stalled
  HIPCHK(hipMemcpyAsync(h->theta, b.theta_k, (size_t)P * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  if (pairs > 0.0) h->lb_reset = true;
  info[0] = pairs > 0.0 ? 1.0 : 2.0;
  info[2] = fk; info[3] = h->lb_f[1]; info[4] = h->lb_f[2]; info[5] = h->lb_f[3]; info[6] = 0.0;
  return VN_OK;
}

int vn_lbfgs_loss64(vn_engine* h, int on) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (!is_lbfgs(h))
    return fail(VN_ESTATE, "vn_lbfgs_loss64 needs an engine created with optimizer = VN_OPT_LBFGS (this one runs %s)",
                h->cfg.optimizer == VN_OPT_RMSPROP ? "RMSProp" : "Adam");
  if (on && !vn_obj64_supported(h->net))
    return fail(VN_EUNSUPPORTED, "vn_lbfgs_loss64: the fp64 objective (vn_objective_f64) does not serve this network (%d layers, "
                "widest %d, %d inputs, dim %d%s): it is outside the range of the hand-written kernels", h->net.L, h->net.hmax,
                h->net.d_in, h->net.dim, h->net.act == VN_ACT_PER_LAYER ? ", mixed activations" : "");
  const bool want = on != 0;
  if (want != h->lb_loss64) lbfgs_invalidate(h);     // f_k was measured in the other precision
  h->lb_loss64 = want;
  return VN_OK;
}

int vn_eval_loss(vn_engine* h, int32_t batch, double out[4], float* lossVec_dev) {
  if (!h || !out) return fail(VN_EINVAL, "null argument");
  (void)hipGetLastError();   // a stale last-error of another library on this thread is not ours to report
  if (int rc = check_batch(h, batch)) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = ansatz_check_eval(h, h->batches[batch], batch)) return rc;
  if (bicw_on(h))
    if (int rc = bicw_check(h, "weights on the BC/IC rows (vn_set_bic_weights / vn_set_bic_adapt)")) return rc;
  if (int rc = source_mix(h, h->batches[batch], batch)) return rc;
  if (int rc = field_mix(h, h->batches[batch], batch)) return rc;
  if (int rc = bic_mix(h, h->batches[batch], batch)) return rc;
  if (int rc = fluxbc_mix(h)) return rc;
  VnEdgeSums fx;
  if (int rc = edge_passes(h, false, &fx)) return rc;
  if (int rc = run_forward_and_seed(h, h->batches[batch], false, lossVec_dev, h->lossbuf, fx)) return rc;
  float t[4];
  HIPCHK(hipMemcpyAsync(t, h->lossbuf, sizeof t, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < 4; ++i) out[i] = (double)t[i];
  return VN_OK;
}

int vn_objective_f64(vn_engine* h, int32_t batch, const double* theta_dev, double* grad_dev, double* lossVec_dev, double out[4]) {
  if (!h || !out) return fail(VN_EINVAL, "null argument");
  (void)hipGetLastError();   // a stale last-error of another library on this thread is not ours to report
  if (int rc = check_batch(h, batch)) return rc;
  if (!vn_obj64_supported(h->net))
    return fail(VN_EUNSUPPORTED, "vn_objective_f64 serves networks of the hand-written kernels (<= %d hidden layers, width <= %d, <= %d "
                "inputs, dim <= 3, one activation); this one (%d layers, widest %d, %d inputs, dim %d%s) is outside that range",
                VN_KMAX_LAYERS, VN_KMAX_WIDTH, VN_KMAX_DIN, h->net.L, h->net.hmax, h->net.d_in, h->net.dim,
                h->net.act == VN_ACT_PER_LAYER ? ", mixed activations" : "");
  if (has_ansatz(h->batches[batch]) || h->az_bic.B || h->az_edge[0].B || h->az_edge[1].B || h->az_edge[2].B)
    return fail(VN_EUNSUPPORTED, "vn_objective_f64 on batch %d next to a hard-constraint ansatz (vn_set_ansatz, vn_set_ansatz_rows): the "
                                 "fp64 objective does not carry the ansatz stage", batch);
  if (bicw_on(h))
    if (int rc = bicw_check(h, "weights on the BC/IC rows (vn_set_bic_weights / vn_set_bic_adapt)")) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (!theta_dev) {
    if (int rc = refresh_theta64(h)) return rc;
    theta_dev = h->theta64;
  }
  const Batch& b = h->batches[batch];
  if (int rc = source_mix(h, b, batch)) return rc;     // source identification: the mixed fp32 stream, widened exactly
  if (int rc = field_mix(h, b, batch)) return rc;      // field identification: likewise the mixed direction
  if (int rc = bic_mix(h, b, batch)) return rc;        // boundary data identification: likewise the mixed labels
  if (int rc = fluxbc_mix(h)) return rc;               // flux boundary identification: likewise the flux rows' datum and coefficient
  VnObj64Problem p{};
  p.net = h->net; p.theta = theta_dev;
  p.X = b.Input; p.G = batch_gcoef(h, b); p.src = batch_src(h, b);
  p.feN = h->feN; p.fedNt = h->fedNt; p.feW = fe_w(h);
  p.Nrow = b.Nrow; p.dNtrow = b.dNtrow; p.detJv = b.detJv; p.detJ = b.detJ;
  p.n_k = b.n_k; p.q = h->cfg.integ_num; p.td = h->cfg.time_dependent;
  p.Xb = bi_x(h, b); p.label = bi_y(h, b); p.nB = h->nB; p.bDof = h->bDof; p.biDimVal = h->biDimVal;
  const EdgeSet &ef = h->es[VN_EDGE_FLUX], &ep = h->es[VN_EDGE_PERIODIC], &eo = h->es[VN_EDGE_OBS];
  p.Xf = ef.X; p.Nf = ef.G; p.fcoef = flux_coef(h); p.flabel = flux_label(h); p.nF = ef.count; p.fbiDimVal = h->fbiDimVal;
  p.Xp = ep.X; p.Dp = ep.G; p.nP = ep.count; p.pgamma = h->pgamma; p.pbiDimVal = h->pbiDimVal;
  p.Xo = eo.X; p.Qo = h->oQ; p.Do = eo.G; p.orowptr = h->orowptr; p.ovalue = h->oval; p.owgt = h->owgt;
  p.on = eo.rows; p.nO = eo.count; p.olambda = h->olambda; p.omisfit = h->omisfit;
  p.w[0] = h->w[0]; p.w[1] = h->w[1]; p.w[2] = h->w[2];
  p.react = b.react.on ? 1 : 0; p.rate = b.react.stream; std::copy(b.react.c, b.react.c + 3, p.coef);
  p.nlflux = b.nlflux.on ? 1 : 0; p.phi = b.nlflux.stream; std::copy(b.nlflux.c, b.nlflux.c + 3, p.fcoef3);
  p.nldiff = b.nldiff.on ? 1 : 0; p.psi = b.nldiff.stream; std::copy(b.nldiff.c, b.nldiff.c + 3, p.dcoef3);
  if (h->lv[LV_COEF].on) {   // inverse mode: at the current device coefficients, widened exactly
    float c[VN_COEF_N];
    HIPCHK(hipMemcpyAsync(c, h->lv[LV_COEF].state, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < 3; ++i) { p.coef[i] = c[i]; p.fcoef3[i] = c[3 + i]; p.dcoef3[i] = c[6 + i]; }
  }
  p.wt = b.wt;
  for (int s = 0; s < 2; ++s)   // weights on the BC/IC rows: the committed omega, widened exactly (a probe: nothing moves)
    p.bic_omega[s] = h->bw[s] ? adapt_state(*h->bw[s], h->bw[s]->cur).omega : nullptr;
  hipError_t e = vn_obj64_run(h->o64, p, grad_dev, lossVec_dev, out, h->ncu, h->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(h->stream);
    return fail(e == hipErrorOutOfMemory ? VN_ENOMEM : VN_EHIP, "vn_objective_f64: %s", hipGetErrorString(e));
  }
  return VN_OK;
}

int vn_forward(vn_engine* h, const float* X, int64_t n, float* u) {
  if (!h || (n > 0 && (!X || !u))) return fail(VN_EINVAL, "null argument");
  (void)hipGetLastError();   // a stale last-error of another library on this thread is not ours to report
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->route == Route::layered) {
    VnRows sl{};
    sl.X = X; sl.G = nullptr; sl.u = u; sl.ud = nullptr; sl.n = n;
    LAYCHK(vn_layered_forward(h->layered, h->theta, sl, h->stream, lerr_, sizeof lerr_));
    return VN_OK;
  }
  // networks of the 8-wave family (7-8 hidden layers included): the value-only sweep of the point kernels (F_pt per point;
  // the fused kernel's forward-only mode would carry a tangent stream of zeros through every layer)
  if (on_8wave(h)) {
    HIPCHK(point_pass(h, X, n, u, nullptr, nullptr));
    return VN_OK;
  }
  VnRows s0{}, s1{};
  s0.X = X; s0.G = nullptr; s0.u = u; s0.ud = nullptr; s0.n = n;
  HIPCHK(vn_generic_forward(h->net, h->theta, s0, s1, h->fwd_grid, h->stream));
  return VN_OK;
}

int vn_forward_grad(vn_engine* h, const float* X, int64_t n, float* u, float* g) {
  if (!h || (n > 0 && (!X || !u || !g))) return fail(VN_EINVAL, "null argument");
  (void)hipGetLastError();   // a stale last-error of another library on this thread is not ours to report
  if (!on_8wave(h)) return fail(VN_EUNSUPPORTED, "vn_forward_grad needs a network of the 8-wave fused kernel");
  if (h->cfg.dim > 3) return fail(VN_EUNSUPPORTED, "vn_forward_grad supports dim <= 3");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(point_pass(h, X, n, u, g, nullptr));
  return VN_OK;
}

int vn_forward_f64(vn_engine* h, const double* X, int64_t n, double* u) {
  if (!h || (n > 0 && (!X || !u))) return fail(VN_EINVAL, "null argument");
  (void)hipGetLastError();   // a stale last-error of another library on this thread is not ours to report
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = refresh_theta64(h)) return rc;
  if (h->route == Route::layered) {
    LAYCHK(vn_layered_forward_f64(h->layered, h->theta64, X, n, u, h->stream, lerr_, sizeof lerr_));
    return VN_OK;
  }
  if (use_taylor16d(h)) {
    HIPCHK(vn_taylor16d_launch(h->net, h->theta64, X, nullptr, nullptr, nullptr, nullptr, h->cfg.time_dependent, n, u, nullptr, h->ncu, h->stream));
    return VN_OK;
  }
  HIPCHK(vn_pointwise_forward_f64(h->net, h->theta64, X, n, u, h->stream));
  return VN_OK;
}

int vn_residual(vn_engine* h, const float* X, const float* diff, const float* vel, const float* src,
                const float* ddx, int64_t n, float* u, float* res) {
  if (!h || (n > 0 && (!X || !diff || !vel || !res))) return fail(VN_EINVAL, "null argument");
  if (h->cfg.dim > 3) return fail(VN_EUNSUPPORTED, "residual supports dim <= 3");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->route == Route::layered) {
    LAYCHK(vn_layered_residual_f32(h->layered, h->theta, X, diff, vel, src, ddx, h->cfg.time_dependent, n, u, res, h->stream,
                                   lerr_, sizeof lerr_));
    return VN_OK;
  }
  HIPCHK(residual_f32(h, X, diff, vel, src, ddx, n, u, res));
  return VN_OK;
}

int vn_residual_f64(vn_engine* h, const double* X, const double* diff, const double* vel, const double* src,
                    const double* ddx, int64_t n, double* u, double* res) {
  if (!h || (n > 0 && (!X || !diff || !vel || !res))) return fail(VN_EINVAL, "null argument");
  if (h->cfg.dim > 3) return fail(VN_EUNSUPPORTED, "residual supports dim <= 3");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = refresh_theta64(h)) return rc;
  if (h->route == Route::layered) {
    LAYCHK(vn_layered_residual_f64(h->layered, h->theta64, X, diff, vel, src, ddx, h->cfg.time_dependent, n, u, res, h->stream,
                                   lerr_, sizeof lerr_));
    return VN_OK;
  }
  if (use_taylor16d(h)) {
    HIPCHK(vn_taylor16d_launch(h->net, h->theta64, X, diff, vel, src, ddx, h->cfg.time_dependent, n, u, res, h->ncu, h->stream));
    return VN_OK;
  }
  HIPCHK(vn_pointwise_residual_f64(h->net, h->theta64, X, diff, vel, src, ddx, h->cfg.time_dependent, n, u, res,
                                   h->stream));
  return VN_OK;
}


// ---- tower gradient SUM over RCCL (TFModel.py:342-377) ------------------------------------
int vn_comm_available(void) { return load_rccl(); }

int vn_comm_version(int32_t* version_out) {
  if (!version_out) return fail(VN_EINVAL, "null argument");
  if (int rc = load_rccl()) return rc;
  int v = 0;
  RCCLCHK(g_rccl.GetVersion(&v));
  *version_out = v;
  return VN_OK;
}

int vn_comm_unique_id(void* id_out) {
  if (!id_out) return fail(VN_EINVAL, "null argument");
  if (int rc = load_rccl()) return rc;
  static_assert(sizeof(ncclUniqueId) == VN_COMM_ID_BYTES, "RCCL unique id size");
  ncclUniqueId id;
  RCCLCHK(g_rccl.GetUniqueId(&id));
  memcpy(id_out, &id, sizeof id);
  return VN_OK;
}

int vn_comm_init(vn_engine* h, int32_t rank, int32_t world, const void* unique_id) {
  if (!h || !unique_id) return fail(VN_EINVAL, "null argument");
  if (world < 1 || rank < 0 || rank >= world) return fail(VN_EINVAL, "need 0 <= rank < world (got %d of %d)", rank, world);
  {
    std::lock_guard<std::mutex> lk(h->comm_mu);
    if (h->comm_abandoned) return fail(VN_ESTATE, "this engine's communicator was abandoned (vn_comm_abandon): it takes no other");
    if (h->comm) return fail(VN_ESTATE, "communicator already initialised (call vn_comm_destroy first)");
  }
  for (size_t i = 0; i < h->batches.size(); ++i)
    if (h->batches[i].wt.S > 0)
      return fail(VN_EUNSUPPORTED, "vn_comm_init: batch %d has a causal registration (vn_set_causal); a rank's slab means would cover "
                                   "only its shard, so the ranks together would train another objective than one rank", (int)i);
  for (size_t i = 0; i < h->batches.size(); ++i)
    if (h->batches[i].ad)
      return fail(VN_EUNSUPPORTED, "vn_comm_init: batch %d has an adaptive registration (vn_set_tf_adapt); a rank's max, mean and Z would "
                                   "cover only its shard, so the ranks together would train another objective than one rank", (int)i);
  if (bicw_on(h))
    return fail(VN_EUNSUPPORTED, "vn_comm_init next to weights on the BC/IC rows (vn_set_bic_weights / vn_set_bic_adapt): a rank's max, mean "
                                 "and Z would follow its own shard's steps, so the ranks together would train another objective than one rank");
  for (int id = LV_N - 1; id >= 0; --id)       // (the field amplitudes are reported first)
    if (h->lv[id].on)
      return fail(VN_EUNSUPPORTED, "vn_comm_init while %s are learnt (%s): %s are not in the all-reduced buffer, so every rank would "
                                   "follow its own shard's", kLearnt[id].what, kLearnt[id].setter, kLearnt[id].grads);
  if (reparam_on(h))
    return fail(VN_EUNSUPPORTED, "vn_comm_init while weight scales are learnt (vn_set_reparam): the scales' gradient is formed from each "
                                 "rank's own V after the all-reduce, a route that is not built");
  if (int rc = load_rccl()) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  ncclUniqueId id;
  memcpy(&id, unique_id, sizeof id);
  ncclComm_t c = nullptr;
  RCCLCHK(g_rccl.CommInitRank(&c, world, id, rank));
  int cnt = 0;
  RCCLCHK(g_rccl.CommCount(c, &cnt));
  if (cnt != world) { (void)g_rccl.CommDestroy(c); return fail(VN_ECOMM, "RCCL reports %d ranks, expected %d", cnt, world); }
  std::lock_guard<std::mutex> lk(h->comm_mu);
  if (h->comm_abandoned) {       // the caller gave up on this call while it sat in ncclCommInitRank: the engine must not start using it
    h->comm_orphan = c;
    return fail(VN_ESTATE, "ncclCommInitRank returned after the communicator was abandoned (vn_comm_abandon)");
  }
  h->comm = c; h->comm_world = world; h->comm_rank = rank;
  return VN_OK;
}

int vn_comm_abandon(vn_engine* h) {
  if (!h) return fail(VN_EINVAL, "null handle");
  std::lock_guard<std::mutex> lk(h->comm_mu);
  h->comm_abandoned = true;
  if (h->comm) { h->comm_orphan = h->comm; h->comm = nullptr; h->comm_world = 1; h->comm_rank = 0; }
  return VN_OK;
}

int vn_comm_size(const vn_engine* h, int32_t* world, int32_t* rank) {
  if (!h || !world) return fail(VN_EINVAL, "null argument");
  int cnt = 1;
  if (h->comm) RCCLCHK(g_rccl.CommCount(h->comm, &cnt));
  *world = cnt;
  if (rank) *rank = h->comm ? h->comm_rank : 0;
  return VN_OK;
}

int vn_comm_destroy(vn_engine* h) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (!h->comm) return VN_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  ncclComm_t c = h->comm;
  h->comm = nullptr; h->comm_world = 1; h->comm_rank = 0;
  RCCLCHK(g_rccl.CommDestroy(c));
  return VN_OK;
}

int vn_allreduce_grad(vn_engine* h) {
  if (!h) return fail(VN_EINVAL, "null handle");
  if (!h->comm) return fail(VN_ESTATE, "no communicator (call vn_comm_init first)");
  HIPCHK(hipSetDevice(h->cfg.device));
  // one collective per step: P gradient floats + (loss, BC, IC, var), in place, on the engine stream
  const bool rec = h->prof_on && h->cprof_n < PROF_CAP;
  if (rec) {
    if (!h->cev0[h->cprof_n]) { HIPCHK(hipEventCreate(&h->cev0[h->cprof_n])); HIPCHK(hipEventCreate(&h->cev1[h->cprof_n])); }
    HIPCHK(hipEventRecord(h->cev0[h->cprof_n], h->stream));
  }
  RCCLCHK(g_rccl.AllReduce(h->gradbuf, h->gradbuf, (size_t)h->net.P + 4, ncclFloat32, ncclSum, h->comm, h->stream));
  if (rec) { HIPCHK(hipEventRecord(h->cev1[h->cprof_n], h->stream)); h->cprof_n++; }
  return VN_OK;
}

int vn_get_step(const vn_engine* h, int64_t* step) {
  if (!h || !step) return fail(VN_EINVAL, "null argument");
  *step = h->step;
  return VN_OK;
}

int vn_profile_comm(vn_engine* h, double* mean_ms, int64_t* calls) {
  if (!h) return fail(VN_EINVAL, "null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  double tot = 0.0;
  for (int i = 0; i < h->cprof_n; ++i) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->cev0[i], h->cev1[i]));
    tot += ms;
  }
  if (mean_ms) *mean_ms = h->cprof_n ? tot / h->cprof_n : 0.0;
  if (calls) *calls = h->cprof_n;
  return VN_OK;
}

int vn_kernel_path(const vn_engine* h, int32_t* kernel, int32_t* two_pass) {
  if (!h || !kernel) return fail(VN_EINVAL, "null argument");
  switch (h->route) {
    case Route::layered: *kernel = VN_KERNEL_LAYERED; break;
    case Route::generic: *kernel = VN_KERNEL_GENERIC; break;
    case Route::fused4: *kernel = VN_KERNEL_FUSED; break;
    case Route::fused8:
    case Route::twopass: *kernel = VN_KERNEL_FUSED16; break;
  }
  if (two_pass) *two_pass = h->route == Route::twopass ? 1 : 0;
  return VN_OK;
}

int vn_debug_calibrate(vn_engine* h, double out[5]) {
  if (!h || !out) return fail(VN_EINVAL, "null argument");
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(vn_calibrate(h->ncu, h->stream, out));
  return VN_OK;
}

int vn_debug_calibrate_f64(vn_engine* h, double ghz, double out[3]) {
  if (!h || !out) return fail(VN_EINVAL, "null argument");
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(vn_calibrate_f64(h->ncu, h->stream, ghz, out));
  return VN_OK;
}

int vn_debug_point_route(vn_engine* h, int32_t per_thread) {
  if (!h) return fail(VN_EINVAL, "null handle");
  h->no_gtable = (per_thread & 4) != 0;
  h->eval_rowwise = (per_thread & 8) != 0;
  per_thread &= 3;
  if (per_thread == 2 && !kWithF32Point)
    return fail(VN_EUNSUPPORTED, "route 2 (f32-MFMA point kernels for the networks the bf16-piece kernels serve) exists in the tests' "
                                 "cross-check build only: libvarnet_hip_xcheck.so (make -C varnet_amd/csrc xcheck)");
  h->point_route = per_thread == 1 ? PointRoute::per_thread : per_thread == 2 ? PointRoute::f32_mfma : PointRoute::automatic;
  return VN_OK;
}

int vn_debug_stamps(vn_engine* h, unsigned long long out[8]) {
  if (!h || !out) return fail(VN_EINVAL, "null argument");
  if (!h->stamps) { memset(out, 0, 8 * sizeof(unsigned long long)); return VN_OK; }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(out, h->stamps, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return VN_OK;
}

int vn_profile_begin(vn_engine* h) {
  if (!h) return fail(VN_EINVAL, "null handle");
  h->prof_on = true;
  h->prof_n = 0;
  h->cprof_n = 0;
  return VN_OK;
}

int vn_profile_end(vn_engine* h, double* mean_ms, int64_t* launches, char* name, int32_t name_len) {
  if (!h) return fail(VN_EINVAL, "null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  double tot = 0.0;
  for (int i = 0; i < h->prof_n; ++i) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev0[i], h->ev1[i]));
    tot += ms;
  }
  if (mean_ms) *mean_ms = h->prof_n ? tot / h->prof_n : 0.0;
  if (launches) *launches = h->prof_n;
  if (name && name_len > 0) {
    strncpy(name, h->prof_name.c_str(), name_len - 1);
    name[name_len - 1] = 0;
  }
  h->prof_on = false;
  return VN_OK;
}

}  // extern "C"
