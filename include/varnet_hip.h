/*
 * varnet_hip.h -- C ABI of libvarnet_hip.so, the MI355X (gfx950) engine behind the VarNet
 * variational-loss training loop.
 *
 * The reference has no FFI layer: its device boundary is the `TFNN` object that
 * `VarNet` / `ManageTrainData` drive through `sess.run(feed_dict)`.  Every entry point below
 * replaces one of those call sites (cited as /root/reference/<file>:<line>).  All functions
 * are `extern "C"`, take plain pointers and sizes, return 0 on success and a non-zero
 * VN_E* code on failure (message via vn_last_error()).
 *
 * Conventions
 *   - "dev" pointers are device (HBM) addresses owned by the caller; they must stay valid
 *     while registered.  "host" pointers are ordinary host memory.
 *   - Rows of the interior arrays are grouped by test function: row r = k*integ_num + p
 *     (test function k, quadrature point p), exactly the reference's `Input` layout
 *     (VarNet.py:576-588, VarNetUtility.py:820).
 *   - Flat parameter order: W_1[d_in,H_1] row-major, b_1[H_1], ..., w_o[H_L,1], b_o[1]
 *     (Keras kernel is [in,out]; TFModel.py:208-242).
 *   - All work is enqueued on the stream given to vn_set_stream (default: the null stream);
 *     no entry point synchronises with the host unless its comment says so.
 *   - A handle is not thread-safe; use one handle per GPU / per process.
 */
#ifndef VARNET_HIP_H
#define VARNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* What a vn_config may describe (the reference takes any layerWidth list, TFModel.py:208-221).  The hand-written
 * kernels cover the VN_K* range; anything beyond it runs on the layer-by-layer route (VN_KERNEL_LAYERED). */
#define VN_MAX_LAYERS 16    /* hidden layers                                   */
#define VN_MAX_WIDTH  2048  /* hidden width                                    */
#define VN_MAX_DIN    32    /* network inputs: dim + time + MOR parameters     */
#define VN_KMAX_LAYERS 6    /* ... covered by the fused / generic kernels      */
#define VN_KMAX_WIDTH  64
#define VN_KMAX_DIN    8

enum {
  VN_OK = 0,
  VN_EINVAL = 1,   /* bad argument                                             */
  VN_EHIP = 2,     /* a HIP runtime call failed                                */
  VN_ESTATE = 3,   /* call order violated (e.g. step before data registered)   */
  VN_ENOMEM = 4,
  VN_EUNSUPPORTED = 5,
  VN_ECOMM = 6     /* an RCCL call failed                                      */
};

/* activationFun options of the constructor (VarNet.py:97).  VN_ACT_PER_LAYER: vn_config.layer_act holds one of the two
 * per hidden layer (the reference accepts a list, TFModel.py:113-119); a list with different entries runs on the
 * layer-by-layer route, the kernels take one activation for all hidden layers. */
enum { VN_ACT_SIGMOID = 0, VN_ACT_TANH = 1, VN_ACT_PER_LAYER = 2 };
enum { VN_OPT_ADAM = 0, VN_OPT_RMSPROP = 1,     /* tf.train.AdamOptimizer / RMSPropOptimizer (TFModel.py:183-186) */
       VN_OPT_LBFGS = 2 };                      /* no reference counterpart: device-resident L-BFGS, advanced by vn_lbfgs_step */
#define VN_LBFGS_HISTORY 10                     /* (s, y) pairs the L-BFGS ring keeps */
/* Kernel families.  AUTO picks the 8-wave fused kernel where it is instantiated: uniform or ragged hidden widths
 * <= 50 with 1..8 layers, <= 64 with 1..6 layers, d_in <= 8, sigmoid or tanh; integ_num <= 128 in one launch, larger
 * through the two-pass route.  The generic kernels serve VN_KERNEL_GENERIC requests (the independent cross-check of the
 * tests); networks beyond VN_KMAX_* run on the layer-by-layer route. */
enum { VN_KERNEL_AUTO = 0, VN_KERNEL_GENERIC = 1, VN_KERNEL_FUSED = 2 /* 4 waves, 32x32x2 */,
       VN_KERNEL_FUSED16 = 3 /* 8 waves, 16x16x4 */,
       /* Layer-by-layer route for networks outside the kernels' range (more than 6 hidden layers, widths above 64,
        * more than 8 inputs).  Hidden widths <= 256: tile
        * kernels that carry 32 points through all layers with the activations in LDS and keep (a, ad) of every layer
        * in HBM for the reverse kernel (6 F_pt per point).  Otherwise: activations of a chunk of rows live in HBM,
        * every layer is one GEMM over the stacked (value, tangent) rows -- the hand-written MFMA products of vn_gemm.hip --
        * plus hand-written elementwise kernels (6 F_pt when a step's activations fit in HBM, else 8).  Same results
        * contract as the other routes. */
       VN_KERNEL_LAYERED = 4 };

typedef struct vn_engine vn_engine;

/* Replaces the arguments of TFNN.__init__ (TFModel.py:85-191) + lossOpt (VarNet.py:182-185). */
typedef struct vn_config {
  int32_t dim;                      /* spatial dimension                                   */
  int32_t d_in;                     /* network inputs (VarNet.py:174-180)                  */
  int32_t n_layers;                 /* hidden layers L                                     */
  int32_t widths[VN_MAX_LAYERS];    /* layerWidth                                          */
  int32_t activation;               /* VN_ACT_SIGMOID | VN_ACT_TANH for all hidden layers, or VN_ACT_PER_LAYER */
  int32_t integ_num;                /* quadrature points per test function (FiniteElement.py:416) */
  int32_t time_dependent;           /* TFModel.py:537,646,655                              */
  int32_t has_source;               /* lossOpt['isSource']  (TFModel.py:656)               */
  int32_t has_integw;               /* lossOpt['integWflag'] (TFModel.py:660)              */
  int32_t device;                   /* HIP device ordinal                                  */
  int32_t optimizer;                /* VN_OPT_ADAM | VN_OPT_RMSPROP (TFModel.py:183-186) | VN_OPT_LBFGS */
  int32_t kernel;                   /* VN_KERNEL_*                                         */
  double  lr, beta1, beta2, eps;    /* taken literally, NO defaulting (TF-1's own defaults are 1e-3, .9, .999, 1e-8).  lr >= 0
                                     * (lr = 0 is legal TF: TFModel.py:130).  With VN_OPT_ADAM: 0 <= beta1, beta2 < 1 and
                                     * eps > 0, else vn_create returns VN_EINVAL -- a zero-initialised struct (eps = 0 turns a
                                     * zero gradient into 0/0 = NaN in the update) is rejected, not trained.  RMSProp ignores
                                     * beta1, beta2, eps (TF-1 constants: decay 0.9, momentum 0, epsilon 1e-10); L-BFGS ignores
                                     * all four.                                                                          */
  int32_t layer_act[VN_MAX_LAYERS]; /* with VN_ACT_PER_LAYER: VN_ACT_SIGMOID | VN_ACT_TANH of hidden layer i */
} vn_config;

const char* vn_last_error(void);
int  vn_abi_version(void);   /* 2: towers (vn_comm_*), tanh, empty feeds, vn_kernel_path, vn_profile_comm;
                                * 3: vn_config.widths holds VN_MAX_LAYERS = 16 entries, layer_act, VN_KERNEL_LAYERED;
                                * 4: vn_comm_available, Adam hyper-parameters validated (no silent NaN from a zeroed config);
                                * 5: vn_comm_version;
                                * 6: vn_forward_grad, vn_debug_calibrate
                                * 7: vn_comm_abandon, vn_debug_point_route, vn_debug_calibrate_f64, vn_state_snapshot / vn_state_rollback */
#define VN_ABI_VERSION 7     /* what this header describes: a binding must refuse a library that reports another number */

/* TFNN.__init__ / graph + session construction (TFModel.py:85-191, 293-338). */
int vn_create(const vn_config* cfg, vn_engine** out);
int vn_destroy(vn_engine* h);
/* Stream all later work is enqueued on (pass torch.cuda.current_stream().cuda_stream). */
int vn_set_stream(vn_engine* h, void* hip_stream);

/* Number of trainable scalars P. */
int vn_param_count(const vn_engine* h, int64_t* n);
/* sess.run(global_variables_initializer()) (TFModel.py:326, VarNet.py:1412): glorot-uniform
 * kernels, zero biases, zero Adam slots, step 0.  Deterministic in `seed`. */
int vn_params_init(vn_engine* h, uint64_t seed);
/* saver.save / restore of the trainable variables, saveNNparam (VarNet.py:1362,1498,2231).
 * Host buffers of P floats.  These two synchronise the stream. */
int vn_params_get(vn_engine* h, float* host, int64_t n);
int vn_params_set(vn_engine* h, const float* host, int64_t n);
/* Full optimiser state {theta, m, v, step}: what tf.train.Saver writes (TFModel.py:307).
 * Layout: int64 step, then 3*P floats.  Synchronises. */
int vn_state_size(const vn_engine* h, int64_t* bytes);
int vn_state_export(vn_engine* h, void* host, int64_t bytes);
int vn_state_import(vn_engine* h, const void* host, int64_t bytes);
/* Device-side snapshot of the same state (parameters, both optimizer slots, step counter) in the engine's one snapshot slot, and
 * the way back to it; on the engine stream, no host copy, no synchronisation (ABI 7).  VarNet.train stands its `lossLag` blocks on
 * it: k epochs are enqueued before ONE read-back of their losses (the reference reads one loss per epoch, VarNetUtility.py:1044);
 * when the stopping test `loss < tol` (VarNet.py:1378) fires inside a block, the state is rolled back to the block's start and the
 * epochs up to the one that met the tolerance are replayed -- the steps are bitwise reproducible -- so the run ends in exactly the
 * state the one-read-back-per-epoch loop ends in.  vn_state_rollback without a snapshot is VN_ESTATE. */
int vn_state_snapshot(vn_engine* h);
int vn_state_rollback(vn_engine* h);

/* Feed of tower.N / tower.dNt / tower.integW (VarNetUtility.py:845-852) for the uniform case,
 * where those nT-row arrays are period-integ_num tables (FiniteElement.py:426-432).
 * Host pointers, integ_num floats each; integW may be NULL (all ones). */
int vn_set_fe_table(vn_engine* h, const float* N, const float* dNt, const float* integW);

/* Feed of tower.Input / gcoef / source / intShape / detJ for one (mini-|MOR-)batch
 * (VarNetUtility.py:840-854).  Device pointers: Input [n_k*integ_num, d_in], gcoef
 * [n_k*integ_num, dim], source [n_k*integ_num] or NULL.  detJ_dev: per-test-function
 * determinants [n_k] (the reference's detJvec=True case) or NULL to use the scalar `detJ`.
 * N_rows/dNt_rows: per-row basis arrays [n_k*integ_num] (non-uniform supports) or NULL to use
 * the table of vn_set_fe_table.  n_k == 0 registers an empty tower feed (the reference slices past the end
 * of the set when batchLen*towers > nt, VarNetUtility.py:830-838): the pointers may then be NULL, only the
 * BC/IC rows contribute and the rank still joins the gradient SUM. */
int vn_set_interior(vn_engine* h, int32_t batch, const float* Input_dev, const float* gcoef_dev,
                    const float* source_dev, int64_t n_k, const float* detJ_dev, double detJ,
                    const float* N_rows_dev, const float* dNt_rows_dev);
/* OPTIONAL, no reference counterpart: de-duplicated formulation for `batch`.  On uniform grids every
 * quadrature point is shared by the 2^feDim hat functions around it, so the reference evaluates the
 * network 2^feDim times per point (VarNet.py:576-588).  Given the unique points Xu [U, d_in], the map
 * uid [n_k*integ_num] row -> unique point and its CSR inverse (rowptr [U+1], rowidx [n_k*integ_num]),
 * vn_grad evaluates value and input gradient once per unique point and assembles the same loss and
 * gradient (same math, different rounding).  All device pointers.  Xu == NULL switches it off.
 * The map is validated on the device at this call (which therefore synchronises): an inconsistent one returns VN_EINVAL
 * (ranges, rowptr a partition of [0, n_k*integ_num), uid[rowidx[e]] = the point whose segment holds e, the rows of a point in
 * increasing order -- hence rowidx a permutation).  The array LENGTHS are the caller's contract (the ABI carries pointers only).
 * A call replaces the batch's previous registration even when it fails: after an error the batch is row-wise.
 * A batch without interior rows (n_k == 0) is VN_EINVAL.
 * Requires a network of the 8-wave fused kernel (integ_num <= 256: the two-pass route's 216 included) and uniform supports.
 * The batch's gcoef is READ at this call (the engine keeps a copy
 * in CSR order for its seed gather): register again after changing gcoef in place; vn_set_interior clears the registration. */
int vn_set_dedup(vn_engine* h, int32_t batch, const float* Xu_dev, int64_t U, const int32_t* uid_dev,
                 const int32_t* rowptr_dev, const int32_t* rowidx_dev);

/* Feed of tower.biInput / biLabel / bDof / biDimVal (VarNetUtility.py:841-849).
 * biInput [nB, d_in], biLabel [nB]; rows [0,bDof) are boundary, [bDof,nB) initial condition.  A steady engine
 * (time_dependent == 0) has no initial condition (TFModel.py:646-650: ICloss is the constant 0): it never evaluates the
 * rows [bDof,nB), and they enter neither the loss nor the gradient. */
int vn_set_bic(vn_engine* h, const float* biInput_dev, const float* biLabel_dev, int64_t nB,
               int64_t bDof, double biDimVal);
/* Optional per-batch copy of the BC/IC rows: the reference's shuffleTrainData feeds every (mini-batch, tower) its own
 * permutation of biInput / biLabel (VarNetUtility.py:988-996).  Same nB, bDof, biDimVal as vn_set_bic; NULL, NULL (or a
 * new vn_set_interior for the batch) returns to the shared set. */
int vn_set_batch_bic(vn_engine* h, int32_t batch, const float* biInput_dev, const float* biLabel_dev);
/* OPTIONAL, no reference counterpart: boundary-flux rows (Neumann / Robin), shared by all batches.  Device pointers:
 * X [nF, d_in], normal [nF, dim] (outward unit normals), coef [nF] (b/a), label [nF] (g/a).  nF == 0 or X == NULL clears.
 * The reference enforces Dirichlet edges only (the BC rows of vn_set_bic); a boundary a grad(c).n + b c = g with a != 0 enters
 * no term of its loss.  With flux rows registered, vn_grad / vn_train_step / vn_train_epoch / vn_eval_loss add per row the
 * residual r = n . grad_x u + (b/a) u - g/a (grad_x: the dim space inputs) to the BC component:
 *     BC = mean_D[biDimVal (u - g/beta)^2] + mean_F[biDimVal r^2]     (the first mean is 0 without Dirichlet rows)
 * weighted by w[0] like the Dirichlet mean; the gradient, the update fused into the reduction and a communicator's all-reduce
 * all see it.  The pass runs on the generic kernels (forward along the normals, residual seeds, reverse pass: three launches
 * per step) whatever route the interior term takes; networks outside VN_KMAX_* (the layer-by-layer route, 7-8 hidden layers,
 * mixed activations) get VN_EUNSUPPORTED.  Without flux rows no launch is added and every result is what it is without this
 * call.  The arrays are READ on every step: they must stay valid while registered.  A call replaces the previous
 * registration, also when it fails (after an error there is none). */
int vn_set_flux_bc(vn_engine* h, const float* X_dev, const float* normal_dev, const float* coef_dev,
                   const float* label_dev, int64_t nF, double biDimVal);
/* OPTIONAL, no reference counterpart: periodic boundary pairs, shared by all batches.  Device pointers: X [2 nP, d_in],
 * dir [2 nP, dim]; rows i and i + nP are the two images of one point (x_B = x_A + s, same time), and both carry the same unit
 * direction d (the outward normal of side A).  nP == 0 or X == NULL clears.  With pairs registered, vn_grad / vn_train_step /
 * vn_train_epoch / vn_eval_loss / vn_lbfgs_step / vn_objective_f64 add the jumps of value and derivative across each pair,
 *     r0 = u_i - u_{i+nP},     r1 = d . grad_x u_i - d . grad_x u_{i+nP}     (grad_x: the dim space inputs)
 * to the BC component:
 *     BC = mean_D[biDimVal (u - g/beta)^2] + mean_F[biDimVal r^2] + mean_P[biDimVal (r0^2 + gamma r1^2)]
 * weighted by w[0] like the other two means (each is 0 without its rows); the gradient, the update fused into the reduction and
 * a communicator's all-reduce all see it.  gamma >= 0 weights the derivative match; gamma == 0 matches values only (no tangent
 * stream is computed and no derivative seed produced); negative or non-finite: VN_EINVAL.  The pass runs on the generic kernels
 * (forward along the directions, pair seeds, reverse pass: three launches per step, beside the flux rows' three when both are
 * registered) whatever route the interior term takes; networks outside VN_KMAX_* (the layer-by-layer route, 7-8 hidden layers,
 * mixed activations) get VN_EUNSUPPORTED.  Without a registration nothing is launched, nothing is allocated and every result is
 * bit for bit what it is without this call.  The arrays are READ on every step: they must stay valid while registered.  A call
 * replaces the previous registration, also when it fails (after an error there is none), and invalidates the L-BFGS (f_k, g_k)
 * and ring, like vn_set_flux_bc. */
int vn_set_periodic(vn_engine* h, const float* X_dev, const float* dir_dev, int64_t nP, double gamma, double biDimVal);
/* OPTIONAL, no reference counterpart: observations (sensor data), shared by all batches.  Observation i is a linear functional of
 * the network over a segment of registered points, its measured value c_i and a weight wgt_i (1 / sigma_i^2):
 *     l_i(u) = sum_{j in seg i} [ q_j u(x_j) + dir_j . grad_x u(x_j) ]      (grad_x: the dim space inputs)
 *     r_i = l_i(u) - c_i,     O = (1/nO) sum_i wgt_i r_i^2,     loss = w0 BC + w1 IC + w2 var + lambda O
 * Device pointers: X [n, d_in]; q [n] or NULL (all 1); dir [n, dim] or NULL (no derivative part: no tangent stream is computed and
 * no derivative seed produced); rowptr [nO + 1] int32 or NULL (point sensors: segment i is the point i, n == nO); value [nO];
 * wgt [nO] or NULL (all 1).  A point sensor is a segment of one point with q = 1; an averaged sensor carries quadrature weights q_j;
 * a flux gauge has q = 0 and dir_j = the gauge direction times its coefficient.  nO == 0 clears.  BC, IC, var, lossVec and the
 * gradient buffer's slots P+1..P+3 are untouched by the term; slot P+0 (the loss) gains lambda O, the gradient its derivative, and
 * the unweighted O of the last evaluation (vn_grad, vn_train_step, vn_train_epoch, vn_eval_loss, vn_lbfgs_step, vn_objective_f64)
 * is read with vn_get_obs_misfit.  The update fused into the reduction and a communicator's all-reduce see the term: ranks that
 * register the same observations divide lambda by their number.  The pass runs on the generic kernels (forward along dir, the
 * observations' seed kernel, reverse pass: three launches per step, beside the flux rows' and the periodic pairs') whatever route
 * the interior term takes; networks outside VN_KMAX_* (the layer-by-layer route, 7-8 hidden layers, mixed activations) get
 * VN_EUNSUPPORTED.  The registration is validated on the device (the call may synchronise): rowptr[0] == 0, rowptr strictly
 * increasing (no empty segment), rowptr[nO] == n; value finite; wgt finite and >= 0; q and dir finite; else VN_EINVAL.  lambda
 * negative or non-finite: VN_EINVAL.  Without a registration nothing is launched, nothing is allocated and every result is bit
 * for bit what it is without this call.  The arrays are READ on every step: they must stay valid while registered.  A call
 * replaces the previous registration, also when it fails (after an error there is none), and invalidates the L-BFGS (f_k, g_k)
 * and ring, like vn_set_periodic. */
int vn_set_observations(vn_engine* h, const float* X_dev, const float* q_dev, const float* dir_dev, const int32_t* rowptr_dev,
                        const float* value_dev, const float* wgt_dev, int64_t n, int64_t nO, double lambda);
/* The weight lambda of the observation term, without re-registering (negative or non-finite: VN_EINVAL).  A change invalidates
 * the L-BFGS (f_k, g_k) and ring. */
int vn_set_obs_weight(vn_engine* h, double lambda);
/* The unweighted misfit O of the last evaluation (synchronises the engine's stream).  VN_ESTATE without a registration. */
int vn_get_obs_misfit(vn_engine* h, double* misfit);
/* OPTIONAL, no reference counterpart: a hard-constraint ansatz.  The solution is written as
 *     u(x,t) = A(x,t) + B(x,t) n(x,t)
 * with n the network output, A carrying the Dirichlet and initial data and B vanishing where they must hold (A = IC(x), B = t:
 * an exact initial state; A = g, B = 1 - x^2: exact Dirichlet walls).  The map is affine in n, so it is an elementwise stage
 * (vn_ansatz.hip) after every forward and before every reverse pass: with the engine's value n_r and tangent nd_r = grad_x n . G_r
 * of a row (G: gcoef, a normal, a pair direction, an observation direction)
 *     u_r = A_r + B_r n_r,   ud_r = a_r + b_r n_r + B_r nd_r,      a_r = grad_x A . G_r,  b_r = grad_x B . G_r
 * and everything in between (the row integrand, the polynomial terms, the loss weights, the seed kernels of every row set) sees
 * u and ud as it does without an ansatz.  The time derivative needs no A_t: it is integrated by parts onto the test function.
 * vn_set_ansatz registers the [n_k*integ_num] interior streams of `batch`, after vn_set_interior of that batch:
 *   A_dev, a_dev, b_dev   device floats or NULL (zero);   B_dev   required.   All four NULL clears the registration.
 * A new vn_set_interior clears it; the term, weight and map registrations keep it and it keeps them.  An unregistered batch:
 * VN_ESTATE; a batch without interior rows: VN_EINVAL; a non-finite entry (checked on the device: the call may synchronise):
 * VN_EINVAL.  The arrays are READ on every step: they must stay valid while registered.  A change invalidates the L-BFGS
 * (f_k, g_k) and ring of that batch.
 * An evaluation is ALL or NOTHING: when the batch has an ansatz, every registered row set (BC/IC rows, flux rows, pairs,
 * observations) must have one too (vn_set_ansatz_rows), and the other way round -- else vn_grad, vn_train_*, vn_lbfgs_step and
 * vn_eval_loss return VN_ESTATE and name what is missing: rows evaluated without the map would be a silent wrong answer.
 * Routes: the generic route carries the stage around its seed kernel; a batch of the single-launch 8-wave route runs the
 * two-pass sequence, and on both 8-wave sequences (two-pass, de-duplicated) the BC/IC rows leave the seeded reverse launch for
 * the generic kernels, their partials appended to the step's own.  Refused with VN_EUNSUPPORTED: VN_KERNEL_FUSED (the 4-wave
 * cross-check geometry), the layer-by-layer route and networks outside the generic kernels' range, vn_objective_f64 and
 * vn_lbfgs_loss64 on an ansatz batch, a per-batch BC/IC copy (vn_set_batch_bic) next to BC/IC ansatz streams, and any learnt
 * vector next to an ansatz (at vn_grad).  Without a registration nothing is launched, nothing is allocated and every result is
 * bit for bit what it is without this call. */
int vn_set_ansatz(vn_engine* h, int32_t batch, const float* A_dev, const float* B_dev, const float* a_dev, const float* b_dev);
/* ... at the U unique points of the batch's de-duplication map, after vn_set_dedup of that batch: A and B [U], their spatial
 * gradients [U, dim].  Au_dev, gAu_dev, gBu_dev may be NULL (zero); all four NULL clears the registration, and so does
 * vn_set_dedup.  A batch without a map: VN_ESTATE; non-finite entries: VN_EINVAL.  A step on a batch that has a map and an ansatz
 * but no point streams returns VN_ESTATE. */
int vn_set_ansatz_points(vn_engine* h, int32_t batch, const float* Au_dev, const float* Bu_dev, const float* gAu_dev,
                         const float* gBu_dev);
/* ... on the engine's other row sets.  The row counts are those of the set's registration: nB of vn_set_bic, nF of
 * vn_set_flux_bc, 2 nP of vn_set_periodic, n of vn_set_observations.  a_dev, b_dev are the derivatives of A and B along the
 * set's own direction (normal, pair direction, observation direction); passing them for a set without directions (the BC/IC
 * rows, pairs with gamma == 0, observations without dir) is VN_EINVAL.  All four NULL clears; registering the set again
 * (vn_set_bic, vn_set_flux_bc, ...) drops its streams.  A set that is not registered: VN_ESTATE. */
enum { VN_ANSATZ_BIC = 0, VN_ANSATZ_FLUX = 1, VN_ANSATZ_PERIODIC = 2, VN_ANSATZ_OBS = 3 };
int vn_set_ansatz_rows(vn_engine* h, int32_t set, const float* A_dev, const float* B_dev, const float* a_dev, const float* b_dev);
/* OPTIONAL, no reference counterpart: a polynomial reaction term for `batch`,
 *     c_t = div(kappa grad c) - v.grad c + s + rate(x,t) p(c),     p(c) = c1 c + c2 c^2 + c3 c^3
 * (first-order decay, Fisher-KPP, Allen-Cahn-type reactions).  The term sits on the source side: the row integrand of the weak
 * form (TFModel.py:653-657) becomes  sum_d u_{x_d} gcoef_d - u dNt - (s + rate p(u)) N,  everything after it is unchanged, and the
 * value seed of a row gains  -N rate p'(u)  times the row's tangent seed.
 *   rate_dev  [n_k*integ_num] device floats, one per interior row, or NULL: rate == 1.  READ on every step (it must stay valid
 *             while registered), like the flux rows.
 *   coef      {c1, c2, c3}; NULL or all zero clears the registration.  Non-finite: VN_EINVAL.
 * Per batch, called after vn_set_interior of that batch: a new vn_set_interior clears it (as it clears the de-duplication map),
 * vn_set_dedup keeps it, and this call keeps a registered map.  An unregistered batch: VN_ESTATE; a batch without interior rows
 * (n_k == 0): VN_EINVAL.  A change invalidates the L-BFGS (f_k, g_k) and ring of that batch, like vn_set_flux_bc.
 * With a reaction on the batch vn_grad / vn_train_step / vn_train_epoch (under a communicator as well), vn_eval_loss (lossVec
 * included), vn_lbfgs_step and vn_objective_f64 all see the term.  Routes: the generic, layer-by-layer and two-pass routes carry it
 * in their row-wise seed kernel; a batch of the single-launch 8-wave route runs the two-pass sequence instead (forward-only launch,
 * seed kernel, seeded reverse launch: 8 F_pt per row instead of 6) at any integ_num; the de-duplicated step adds two small kernels
 * (vn_terms.hip); the 4-wave cross-check geometry (VN_KERNEL_FUSED) returns VN_EUNSUPPORTED.  Without a registration nothing is
 * launched, nothing is allocated and every result is bit for bit what it is without this call. */
int vn_set_reaction(vn_engine* h, int32_t batch, const float* rate_dev, const double coef[3]);
/* OPTIONAL, no reference counterpart: a polynomial flux term (Burgers-type advection, scalar conservation laws) for `batch`,
 *     c_t = div(kappa grad c) - v.grad c - div( w(x,t) F(c) ) + s + rate p(c),     F(c) = f1 c + f2 c^2 + f3 c^3
 * (Burgers: w = 1, F = c^2 / 2; LWR traffic: F = c - c^2).  The flux is conservative, so the weak form integrates it by parts onto
 * the test function and only the network value enters: with  phi_r = sum_d w_d(x_r, t_r) dN_r/dx_d  the row integrand
 * (TFModel.py:653-657) becomes  sum_d u_{x_d} gcoef_d - u dNt - (s + rate p(u)) N - F(u) phi,  everything after it is unchanged, and
 * the value seed of a row gains  -phi F'(u)  times the row's tangent seed.  The test functions vanish on the edge of their supports
 * (as the diffusion and time terms assume): there is no boundary term.
 *   phi_dev   [n_k*integ_num] device floats, one per interior row.  READ on every step (it must stay valid while registered),
 *             like the flux rows.  NULL with non-zero coefficients: VN_EINVAL.
 *   coef      {f1, f2, f3}; NULL or all zero clears the registration.  Non-finite: VN_EINVAL.
 * Per batch, called after vn_set_interior of that batch: a new vn_set_interior clears it (as it clears the de-duplication map),
 * vn_set_dedup and vn_set_reaction keep it, and this call keeps a registered map and a registered reaction.  An unregistered
 * batch: VN_ESTATE; a batch without interior rows (n_k == 0): VN_EINVAL.  A change invalidates the L-BFGS (f_k, g_k) and ring of
 * that batch, like vn_set_flux_bc.
 * With a flux term on the batch vn_grad / vn_train_step / vn_train_epoch (under a communicator as well), vn_eval_loss (lossVec
 * included), vn_lbfgs_step and vn_objective_f64 all see the term, together with a reaction of the same batch.  Routes: the generic,
 * layer-by-layer and two-pass routes run two elementwise kernels around their row-wise seed kernel (vn_terms.hip); a batch of the
 * single-launch 8-wave route runs the two-pass sequence instead, at any integ_num; the de-duplicated step adds two small kernels
 * (they divide by the table entries N_p of vn_set_fe_table: a table with a zero entry is VN_EUNSUPPORTED for a batch that has both
 * a map and a flux term); the 4-wave cross-check geometry (VN_KERNEL_FUSED) returns VN_EUNSUPPORTED.  Without a registration
 * nothing is launched, nothing is allocated and every result is bit for bit what it is without this call. */
int vn_set_nlflux(vn_engine* h, int32_t batch, const float* phi_dev, const double coef[3]);
/* OPTIONAL, no reference counterpart: a solution-dependent diffusivity (quasilinear diffusion) for `batch`,
 *     c_t = div( kappa(x,t) D(c) grad c ) - v.grad c - div( w F(c) ) + s + rate p(c),     D(c) = d0 + d1 c + d2 c^2
 * (porous medium c_t = Lap(c^m): D = m c^(m-1); temperature-dependent conductivity; Richards-type moisture transport).
 * THE CALLER'S SIDE: the engine carries one tangent per row, along gcoef, and D(u) must scale the diffusion part only.  On a batch
 * with this term gcoef (vn_set_interior) is  kappa dN/dx  ALONE -- without the v N part -- and the advection comes on the value
 * side: int v.grad u N = -int u (v.grad N + N div v), the test functions vanishing on the edge of their supports, so with
 *     psi_r = sum_d v_d(x_r, t_r) dN_r/dx_d + N_r div v(x_r, t_r)        and       A_r = sum_d u_{x_d} gcoef_d
 * the row integrand (TFModel.py:653-657) becomes  D(u) A - u psi - u dNt - (s + rate p(u)) N - F(u) phi,  everything after it is
 * unchanged, the value seed of a row gains  (D'(u) A - psi)  times the row's tangent seed and the tangent seed is scaled by D(u).
 * Nothing divides by D(u): D(0) = 0 (the porous-medium case) is a regular point.
 *   psi_dev   [n_k*integ_num] device floats, one per interior row, or NULL when v is identically zero.  READ on every step (it
 *             must stay valid while registered), like phi_dev.
 *   coef      {d0, d1, d2}; NULL, or {1, 0, 0} together with psi_dev == NULL, clears the registration.  Non-finite: VN_EINVAL.
 * Per batch, called after vn_set_interior of that batch: a new vn_set_interior clears it, vn_set_dedup, vn_set_reaction and
 * vn_set_nlflux keep it, and this call keeps a registered map, reaction and flux term.  An unregistered batch: VN_ESTATE; a batch
 * without interior rows (n_k == 0): VN_EINVAL.  A change invalidates the L-BFGS (f_k, g_k) and ring of that batch.
 * vn_grad / vn_train_step / vn_train_epoch, vn_eval_loss (lossVec included), vn_lbfgs_step and vn_objective_f64 all see the term.
 * Routes: the generic, layer-by-layer and two-pass routes run two elementwise kernels (vn_terms.hip) around their row-wise seed
 * kernel and the flux term's pair, with A_r saved in an engine-owned [n_k*integ_num] buffer that the first registration allocates;
 * a batch of the single-launch 8-wave route runs the two-pass sequence instead; the de-duplicated step adds two small kernels (the
 * first divides by the table entries N_p of vn_set_fe_table: a zero entry is VN_EUNSUPPORTED for a batch that has both a map and
 * this term); the 4-wave cross-check geometry (VN_KERNEL_FUSED) returns VN_EUNSUPPORTED.  Without a registration nothing is
 * launched, nothing is allocated and every result is bit for bit what it is without this call. */
int vn_set_nldiff(vn_engine* h, int32_t batch, const float* psi_dev, const double coef[3]);
/* Per-test-function loss weights.  The variational loss of a batch is var = sum_k l_k, l_k = detJ_k R_k^2 (lossVec[k]); with
 * weights omega_k >= 0 it becomes  var = sum_k omega_k l_k,  loss = w0 BC + w1 IC + w2 var.  THE GRADIENT TREATS omega AS
 * CONSTANT: the seed of test function k becomes 2 w2 omega_k detJ_k R_k, and every per-row seed derived from it (time term,
 * reaction, flux and D(u) value seeds, the D(u) rescale) is linear in it.  lossVec stays UNWEIGHTED everywhere, in fp32 and
 * fp64: the causal weights are derived from it, and residual-driven sampling and the monitors read it.  BC / IC terms are not
 * weighted.
 *   omega_dev  [n_k] device floats.  READ on every step (it must stay valid while registered), like rate_dev.  NULL clears
 *              the registration.
 * Per batch, called after vn_set_interior of that batch: a new vn_set_interior clears it, vn_set_dedup, vn_set_reaction,
 * vn_set_nlflux and vn_set_nldiff keep it, and this call keeps theirs; it replaces a causal registration (vn_set_causal) of the
 * batch.  An unregistered batch: VN_ESTATE; a batch without interior rows (n_k == 0): VN_EINVAL; the 4-wave cross-check geometry
 * (VN_KERNEL_FUSED): VN_EUNSUPPORTED; clearing is always accepted.  A change invalidates the L-BFGS (f_k, g_k) and ring of that
 * batch.  vn_grad / vn_train_step / vn_train_epoch, vn_eval_loss (weighted var and loss, unweighted lossVec), vn_lbfgs_step and
 * vn_objective_f64 (weights widened exactly) all see the weights.  They work under a communicator.
 * Routes: the weights are applied in kernels of their own (vn_weights.hip) after the seed kernel and the terms' seed kernels:
 * the row-wise routes scale the rows' seeds in one elementwise pass, the de-duplicated step scales the n_k test-function seeds
 * before its gather; both replace the var loss partials by block sums of omega_k l_k in a fixed order.  A batch of the
 * single-launch 8-wave route runs the two-pass sequence instead.  When the caller passes no lossVec the engine uses an [n_k]
 * buffer of its own, allocated at the first registration.  Without a registration nothing is launched, nothing is allocated
 * and every result is bit for bit what it is without this call. */
int vn_set_tf_weights(vn_engine* h, int32_t batch, const float* omega_dev);
/* Causal time-slab weights (Wang, Sankaran, Perdikaris 2022), recomputed on the device at every step from that step's own loss
 * field.  Every test function has a slab id s_k in [0, n_slabs).  With L_s the mean of l_k over the batch's test functions of
 * slab s (an empty slab: 0) and C_s = sum_{s' < s} L_s':  omega_k = exp(-eps C_{s_k}), so omega = 1 on slab 0 and a late slab
 * counts only once the earlier ones have converged.  Accumulated in fp64 in a fixed order, no floating-point atomics: two calls
 * give the same bits (vn_state_rollback + replay relies on it).  Everything else as for vn_set_tf_weights, whose registration
 * on the same batch this call replaces, and vice versa.
 *   slab_dev   [n_k] device ints, VALIDATED on the device and COPIED at this call, which therefore synchronises (like
 *              vn_set_dedup); the caller's array need not outlive the call.  The engine keeps a CSR slab -> test functions in
 *              increasing k, so the slab sums have a fixed order.  NULL clears the registration.
 *   n_slabs    1 <= n_slabs <= 4096;   eps  >= 0 and finite;   ids in range.  Otherwise VN_EINVAL.
 * Refused: vn_lbfgs_step on a batch with a causal registration (VN_EUNSUPPORTED: with constant-for-the-gradient weights that
 * move with theta the search direction is not the gradient of the reported loss, so an Armijo test on it means nothing);
 * this call on a handle that has a communicator, and vn_comm_init on a handle that has a causal batch (VN_EUNSUPPORTED: a
 * rank's slab means would cover only its shard, so W ranks would train another objective than one rank). */
int vn_set_causal(vn_engine* h, int32_t batch, const int32_t* slab_dev, int32_t n_slabs, double eps);
/* omega_s of the batch's causal registration at the current parameters into omega_slab_host[n_slabs] (n_slabs as registered):
 * runs the batch's loss-only evaluation.  Synchronises; changes no engine state.  Without a causal registration: VN_ESTATE. */
int vn_causal_weights(vn_engine* h, int32_t batch, double* omega_slab_host, int32_t n_slabs);
/* Self-adaptive per-test-function weights: a state lambda_k >= 0 (fp32) per test function lives on the device and moves at every
 * gradient step from that step's own unweighted loss field l_k = lossVec[k].  The weights in use are a
 * function of the COMMITTED state only,
 *     omega_k = m(lambda_k) / Z,   m(x) = x^power (power 1 or 2),   Z = mean_j m(lambda_j) if normalize else 1,
 * constant for the gradient like every other weight, and the same in vn_grad / vn_train_step / vn_train_epoch, vn_eval_loss,
 * vn_term_grads and vn_objective_f64 (widened exactly): the loss vn_eval_loss reports is the loss the step trained on.  The update
 * is formed from the step's l_k at theta_t and takes effect from the NEXT step (omega lags one step, for both rules):
 *   rule 1, rba   lambda'_k = gamma lambda_k + eta sqrt(l_k) / max_j sqrt(l_j);  lambda <= max(init, eta / (1 - gamma)) throughout.
 *   rule 2, sa    Adam ascent on lambda with g_k = m'(lambda_k) l_k / mean_j l_j (fp64 mean in a fixed order), slots m1, m2, the
 *                 bias-corrected rate of update tau + 1, then clamped to [0, cap].
 *   rule 0        clears the registration (par and lambda_init_dev are not read).
 * If max_j l_j (rba) or mean_j l_j (sa) is zero or not finite the state does not move: lambda, slots and tau are kept.
 *   par[10]   [0], [1] = (gamma, eta) of rba or (lr, cap) of sa;  [2], [3], [4] = beta1, beta2, eps of sa (ignored by rba);
 *             [5] power;  [6] init;  [7] normalize (0 or 1);  [8] every (updates are enqueued only at gradient evaluations whose
 *             step index -- optimizer steps completed before them -- is a multiple of it; other steps cost a static-weights
 *             step);  [9] reserved.  VN_EINVAL for gamma outside [0, 1], eta < 0, lr < 0, cap <= 0, beta outside [0, 1),
 *             eps <= 0, power not 1 or 2, init < 0, normalize not 0 or 1, every not a whole number >= 1, any entry not finite.
 *   lambda_init_dev  [n_k] device floats, VALIDATED on the device (finite, >= 0; else VN_EINVAL) and COPIED at this call, which
 *             therefore synchronises; any alignment.  NULL: par[6] everywhere.  vn_params_init returns to this initial state.
 * Commit protocol (vn_train_step == vn_grad + vn_apply stays bit for bit): vn_grad of a registered batch applies omega(lambda)
 * and writes the PENDING state (lambda', slots', omega', Z', tau', statistics) into the second half of a double buffer;
 * vn_apply -- and the step vn_train_step / vn_train_epoch fold into the reduction -- commits every pending state by swapping
 * the halves, without a copy.  vn_grad twice without vn_apply recomputes the same pending bits.  vn_eval_loss, vn_term_grads,
 * vn_objective_f64 and every other loss-only call leave committed state, pending state and pending flag as they found them.
 * Three n_k-sized launches per updating step (vn_adapt.hip) over a static-weights step; fp64 folds in a fixed order on a grid
 * fixed by n_k alone, no floating-point atomics: two runs give the same bits on any card.
 * Registration as for vn_set_tf_weights: per batch, after vn_set_interior (a new one clears it); it and a static or causal
 * registration of the batch replace each other; VN_ESTATE / VN_EINVAL (n_k == 0) as there.  VN_EUNSUPPORTED: VN_KERNEL_FUSED;
 * a handle with a communicator, and vn_comm_init on a handle with an adaptive batch (a shard's max, mean and Z are not the
 * batch's); vn_lbfgs_step on an adaptive batch (the causal refusal, for the same reason); learnt vectors, as for every weight.
 * vn_state_snapshot / _rollback and vn_state_size / _export / _import carry (scalars incl. Z and tau, lambda, omega, slots) of
 * every registered batch in batch order after the optimizer state; with none registered their layout is unchanged.  The BC / IC
 * rows have weights of their own (vn_set_bic_weights, vn_set_bic_adapt). */
int vn_set_tf_adapt(vn_engine* h, int32_t batch, int32_t rule, const double par[10], const float* lambda_init_dev);
/* The committed state of the batch's adaptive registration: lambda_host [n_k], omega_host [n_k], slots_host [2 n_k] (m1 | m2; sa
 * only, VN_EINVAL for rba), stats[6] = min, max, mean omega, effective sample share (sum omega)^2 / (n_k sum omega^2), Z, tau
 * (updates that moved the state).  Any output pointer may be NULL.  Synchronises; changes no engine state.  Without an adaptive
 * registration: VN_ESTATE. */
int vn_get_tf_adapt(vn_engine* h, int32_t batch, float* lambda_host, float* omega_host, float* slots_host, double stats[6]);
/* Puts a state back (a checkpoint): lambda_host [n_k] (finite, >= 0), slots_host [2 n_k] (sa; NULL: zeros; VN_EINVAL for rba),
 * tau >= 0.  omega, Z and the statistics are rebuilt on the device, a pending state is dropped.  Synchronises. */
int vn_set_tf_adapt_state(vn_engine* h, int32_t batch, const float* lambda_host, const float* slots_host, int64_t tau);
/* Weights on the Dirichlet and initial rows of vn_set_bic.  The rows fall into two PARTS: bc = rows
 * [0, bDof) (part 0) and ic = rows [bDof, nB) (part 1; absent on a steady engine or when nB == bDof).  Per row e_i = u_i - label_i
 * and the unweighted loss field l_i = e_i^2; per row of a registered part a state lambda_i >= 0 (fp32), per part a normaliser Z_s
 * and an update counter tau_s.  With n_s the rows of part s the weights in use are
 *     omega_i = m(lambda_i) / Z_s,   m(x) = x^p (p 1 or 2),   Z_s = mean over the part of m(lambda) if normalize else 1
 * (all lambda zero under normalize: Z = 1, omega = 0), and they enter as
 *     BC = biDimVal (1 / bDof) sum_{i < bDof} omega_i e_i^2,   IC likewise over its part,
 *     value seed of row i = (the unweighted seed) * omega_i;
 * omega and Z are constants of the gradient.  A part without a registration has omega = 1.  Flux rows, periodic pairs and
 * observation rows stay as they are.
 * vn_set_bic_weights: STATIC weights, omega_dev [nB] device floats (nB as the engine counts them: bDof on a steady engine),
 * VALIDATED on the device (finite, >= 0; else VN_EINVAL) and COPIED, so the call synchronises; normalize (0 or 1) applies per
 * part.  It registers every part that has rows and replaces whatever they held.  NULL clears both parts.
 * vn_set_bic_adapt: ONE part follows rule 1 (rba) or 2 (sa) of vn_set_tf_adapt, with l_i in place of l_k and n_s in place of n_k:
 * its own max / mean, tau_s, Adam slots, Z_s and `every`; par[10] and lambda_init_dev [n_s] exactly as there.  Each part is run
 * independently and may have its own rule and parameters.  rule 0 clears that part.  A static and an adaptive registration of the
 * same part replace each other.  A maximum or a mean that is zero or not finite leaves that part's state, slots and tau_s alone.
 * Commit protocol: that of vn_set_tf_adapt, with the state belonging to the engine's row set, not to a batch -- a gradient
 * evaluation of ANY batch applies the committed omega and writes the pending half; vn_apply or the folded step of vn_train_step /
 * vn_train_epoch commits by a pointer swap; vn_grad twice recomputes the same pending bits; vn_eval_loss, vn_objective_f64 (omega
 * widened exactly), vn_term_grads and every loss-only call move nothing and see the committed omega; a failed folded step drops the pending state; vn_set_bic clears both
 * parts; vn_params_init returns to the registered initial state.
 * While a part is registered the BC/IC rows leave the step's main launch and run as a pass of their own (vn_bicadapt.hip): a
 * forward of the rows, one kernel for loss field, weighted seeds and weighted loss partials (fp64 sums in a fixed order, no
 * atomics), a reverse pass; an adaptive part adds the three launches of vn_adapt.hip on its own loss field.  Without a
 * registration nothing is launched or allocated and every result is bit for bit what it was.
 * vn_state_snapshot / _rollback carry the committed halves; vn_state_size / _export / _import append (scalars incl. Z and tau,
 * lambda, omega, slots) per registered part, bc first, after what vn_set_tf_adapt appends; nothing when none is registered.
 * VN_ESTATE: no rows (vn_set_bic first), a part without rows.  VN_EUNSUPPORTED, in either order of registration: BC/IC ansatz
 * streams (vn_set_ansatz_rows); learnt vectors; a communicator; a batch's own copy of the rows (vn_set_batch_bic); the
 * layer-by-layer route, a network outside the hand-written kernels' range and VN_KERNEL_FUSED; an adaptive part on an L-BFGS engine
 * (static weights work with vn_lbfgs_step, with and without vn_lbfgs_loss64). */
int vn_set_bic_weights(vn_engine* h, const float* omega_dev, int32_t normalize);
int vn_set_bic_adapt(vn_engine* h, int32_t part, int32_t rule, const double par[10], const float* lambda_init_dev);
/* The committed state of a registered part: lambda_host, omega_host [n_s], slots_host [2 n_s] (m1 | m2; sa only, else VN_EINVAL),
 * lossfield_host [n_s] the unweighted l_i of the last evaluation (zeros before the first), stats[6] as for vn_get_tf_adapt.  A
 * static part reports lambda = the weights as given.  Any output pointer may be NULL.  Synchronises; changes no engine state.
 * Without a registration of the part: VN_ESTATE. */
int vn_get_bic_adapt(vn_engine* h, int32_t part, float* lambda_host, float* omega_host, float* slots_host, float* lossfield_host,
                     double stats[6]);
/* Puts the state of an ADAPTIVE part back (a checkpoint), as vn_set_tf_adapt_state does; VN_ESTATE for a static part. */
int vn_set_bic_adapt_state(vn_engine* h, int32_t part, const float* lambda_host, const float* slots_host, int64_t tau);
/* Inverse mode: learn the nine polynomial coefficients next to the parameters.  Index 0..2 = (c1, c2, c3) of the reaction,
 * 3..5 = (f1, f2, f3) of the flux, 6..8 = (d0, d1, d2) of the diffusivity.  While learning is on the engine owns ONE device
 * vector of nine fp32 coefficients (`init`, rounded once), shared by every batch; every registered term of every batch reads its
 * three coefficients from it, and the `coef` a batch passes to vn_set_reaction / vn_set_nlflux / vn_set_nldiff only says that the
 * term is registered (values equal to an unregistered term's no longer clear a term that has a mask entry; NULL still does).
 * The vector outlives a re-registration of the batches.
 *   d loss / d c_m = - sum_r s_r N_p rate_r u_r^m,  d loss / d f_m = - sum_r s_r phi_r u_r^m,  d loss / d d_m = + sum_r s_r A_r u_r^m
 * (s_r: the tangent seed of row r before D(u) rescales it) is formed inside vn_grad / vn_train_step / vn_train_epoch for the
 * masked entries, in a fixed order without atomics (two evaluations: the same bits), per unique point on the de-duplicated step.
 * vn_apply and the fused train steps update the masked entries with the arithmetic of the parameters' Adam update (the engine's
 * beta1, beta2, eps, the shared step counter, the rate `lr`), then clamp them to [lo, hi] (+-inf: unbounded).  Unmasked entries
 * never change a bit.  On a batch that does not carry its term a masked coefficient's gradient reads 0, and the coefficient
 * follows the momentum in its slots from the batches before that did (Adam with g = 0); it stays where it is only while
 * its slots are zero, that is while no batch has carried the term since the registration.
 * vn_state_snapshot / vn_state_rollback carry coefficients and slots; vn_state_size / _export / _import keep their layout.
 *   mask   nine ints (non-zero: learnt), or NULL: learning off, everything freed, the batches' own coefficients count again and
 *          every result is bit for bit what it was before learning was switched on.
 *   init, lo, hi   nine doubles each.  Non-finite init, NaN bounds, lo > hi, lr not finite or <= 0: VN_EINVAL.
 * Refused with VN_EUNSUPPORTED: an RMSProp or L-BFGS engine (also vn_lbfgs_step while learning is on); a handle that has a
 * communicator (and vn_comm_init while learning is on): the nine gradients are not in the all-reduced buffer; a batch with
 * vn_set_tf_weights / vn_set_causal (here, in those calls and in the steps): the weights are applied after the seeds the
 * reduction reads.  The call invalidates the snapshot of vn_state_snapshot.
 * vn_objective_f64 evaluates at the current coefficients (widened exactly); a coefficient gradient in double is not built. */
int vn_set_coef_learn(vn_engine* h, const int32_t mask[9], const double init[9], const double lo[9], const double hi[9], double lr);
/* The nine coefficients now (synchronises) and, when grad is not NULL, the coefficient gradient of the last gradient evaluation
 * (zeros for unmasked entries and before the first one).  Learning off: VN_ESTATE. */
int vn_get_coefs(vn_engine* h, double coef[9], double grad[9]);
/* Overwrites all nine coefficients (rounded to fp32, NOT clamped); the Adam slots stay.  Non-finite: VN_EINVAL; learning off:
 * VN_ESTATE.  Invalidates the snapshot of vn_state_snapshot. */
int vn_set_coefs(vn_engine* h, const double coef[9]);
/* Source identification: the source of a batch is s0 + sum_j a_j phi_j over a basis of J per-row streams, and the amplitudes a_j
 * are learnt next to the parameters from the observations.
 * vn_set_source_basis registers the basis of one batch: phi_dev is [J, n_k * integ_num] fp32 on the device, stream-major (every
 * stream contiguous); the streams are read on every step and must stay valid while registered.  phi_dev == NULL or J == 0 clears
 * the registration, and so does vn_set_interior of that batch.  A call replaces the previous registration, also when it fails.
 * Needs cfg.has_source (VN_ESTATE otherwise; pass a zero source stream when the PDE has no source); J > VN_SRC_MAX: VN_EINVAL.
 * Without vn_set_source_learn a registered basis changes nothing: the batch's source is the stream of vn_set_interior. */
#define VN_SRC_MAX 64
int vn_set_source_basis(vn_engine* h, int32_t batch, const float* phi_dev, int32_t J);
/* The amplitudes are engine-wide, like the nine coefficients of vn_set_coef_learn: while learning is on the engine owns ONE device
 * vector of J fp32 amplitudes (`init`, rounded once), their two Adam slots and a snapshot copy of the three; it outlives a
 * re-registration of the batches.  Every evaluation of a batch with a basis (vn_grad, vn_train_step / _epoch, vn_eval_loss,
 * vn_objective_f64) first forms s_mix[r] = s0[r] + sum_j a_j phi_j[r] (fp32, j ascending, one fused multiply-add per stream) and
 * reads it in place of the batch's source; a batch whose basis has another J makes the step return VN_EINVAL.
 *   d loss / d a_j = - sum_r s_r N_p phi_j[r]   (s_r: the tangent seed of row r before D(u) rescales it)
 * is formed inside vn_grad / vn_train_step / vn_train_epoch for the masked entries, in a fixed order without atomics (two
 * evaluations: the same bits); the single-launch 8-wave route runs its two-pass sequence for such a batch.  vn_apply and the
 * fused train steps update the masked entries with the arithmetic of the parameters' Adam update (the engine's beta1, beta2, eps,
 * the shared step counter -- shared with vn_set_coef_learn too --, the rate `lr`), then clamp them to [lo, hi] (+-inf: unbounded).
 * Unmasked entries take part in the source at their init value and never change a bit.  On a batch without a basis the
 * amplitude gradient reads 0, and the masked amplitudes follow the momentum in their slots, as a coefficient without its term does.
 * vn_state_snapshot / vn_state_rollback carry amplitudes and slots; vn_state_size / _export / _import keep their layout.
 *   mask   J ints (non-zero: learnt), or NULL: learning off, everything freed, every result bit for bit what it was before.
 *   init, lo, hi   J doubles each.  Non-finite init, NaN bounds, lo > hi, lr not finite or <= 0, J outside 1..VN_SRC_MAX: VN_EINVAL.
 * Refused with VN_EUNSUPPORTED for the reasons of vn_set_coef_learn: an RMSProp or L-BFGS engine; a handle that has a communicator
 * (and vn_comm_init while learning is on); a batch with vn_set_tf_weights / vn_set_causal (here, in those calls and in the steps).
 * The call invalidates the snapshot of vn_state_snapshot and the L-BFGS (f_k, g_k). */
int vn_set_source_learn(vn_engine* h, int32_t J, const int32_t* mask, const double* init, const double* lo, const double* hi, double lr);
/* The J amplitudes now (synchronises) and, when grad is not NULL, the amplitude gradient of the last gradient evaluation (zeros for
 * unmasked entries and before the first one).  Learning off: VN_ESTATE; J not the engine's: VN_EINVAL. */
int vn_get_source_amps(vn_engine* h, double* amp, double* grad, int32_t J);
/* Overwrites all J amplitudes (rounded to fp32, NOT clamped); the Adam slots stay.  Non-finite: VN_EINVAL; learning off: VN_ESTATE.
 * Invalidates the snapshot of vn_state_snapshot. */
int vn_set_source_amps(vn_engine* h, const double* amp, int32_t J);
/* Field identification: the tangent direction of a batch is gcoef = g0 + sum_j b_j G_j over a basis of J per-row streams of dim
 * floats per row (G_j[r, d] = chi_j dN_r/dx_d for a diffusivity basis function chi_j, omega_{j,d} N_r for a velocity basis function
 * omega_j; the engine does not know which stream is which), and the amplitudes b_j are learnt next to the parameters from the
 * observations.
 * vn_set_field_basis registers the basis of one batch: G_dev is [J, n_k * integ_num, dim] fp32 on the device, stream-major (every
 * stream contiguous, rows as in gcoef); the streams are read on every step and must stay valid while registered.  G_dev == NULL or
 * J == 0 clears the registration, and so does vn_set_interior of that batch.  A call replaces the previous registration, also
 * when it fails.  J > VN_FLD_MAX: VN_EINVAL.  vn_set_dedup and vn_set_field_basis may come in either order.
 * Without vn_set_field_learn a registered basis is not read: the batch's direction is the gcoef of vn_set_interior. */
#define VN_FLD_MAX 32
int vn_set_field_basis(vn_engine* h, int32_t batch, const float* G_dev, int32_t J);
/* The amplitudes are engine-wide, like those of vn_set_source_learn: while learning is on the engine owns ONE device vector of J
 * fp32 amplitudes (`init`, rounded once), their two Adam slots and a snapshot copy of the three; it outlives a re-registration of
 * the batches.  Every evaluation of a batch with a basis (vn_grad, vn_train_step / _epoch, vn_eval_loss, vn_objective_f64) first
 * forms gmix[e] = g0[e] + sum_j b_j G_j[e] over the n_k * integ_num * dim entries (fp32, j ascending, one fused multiply-add per
 * stream) and reads it in place of the batch's gcoef; the de-duplicated step rebuilds its CSR-ordered copy from it and does not use
 * the periodic-table shortcut for such a batch.  A batch whose basis has another J makes the step return VN_EINVAL.
 *   d loss / d b_j = + sum_r s_r (grad u_r . G_j[r, :])   (s_r: the tangent seed of row r AFTER D(u) rescaled it, vn_set_nldiff)
 * is formed inside vn_grad / vn_train_step / vn_train_epoch for the masked entries, in a fixed order without atomics (two
 * evaluations: the same bits); grad u_r comes from one extra point pass over the batch's rows (row-wise routes; the de-duplicated
 * step has it per point), and the single-launch 8-wave route runs its two-pass sequence for such a batch.  vn_apply and the fused
 * train steps update the masked entries with the arithmetic of the parameters' Adam update (the engine's beta1, beta2, eps, the
 * shared step counter -- shared with vn_set_coef_learn and vn_set_source_learn too --, the rate `lr`), then clamp them to [lo, hi]
 * (+-inf: unbounded).  Unmasked entries take part in gcoef at their init value and never change a bit.  On a batch without a
 * basis the amplitude gradient reads 0, and the masked amplitudes follow the momentum in their slots.  The loss-only forms and
 * vn_objective_f64 run the mix only: no amplitude gradient is built in fp64.
 * vn_state_snapshot / vn_state_rollback carry amplitudes and slots; vn_state_size / _export / _import keep their layout.
 *   mask   J ints (non-zero: learnt), or NULL: learning off, everything freed, every result bit for bit what it was before.
 *   init, lo, hi   J doubles each.  Non-finite init, NaN bounds, lo > hi, lr not finite or <= 0, J outside 1..VN_FLD_MAX: VN_EINVAL.
 * Refused with VN_EUNSUPPORTED for the reasons of vn_set_source_learn: an RMSProp or L-BFGS engine; a handle that has a communicator
 * (and vn_comm_init while learning is on); a batch with vn_set_tf_weights / vn_set_causal (here, in those calls and in the steps).
 * Also with VN_EUNSUPPORTED: cfg.dim > 3 (the point pass carries three gradient components), the layer-by-layer route, the 4-wave
 * cross-check geometry (VN_KERNEL_FUSED), and a network of the generic kernels that the 8-wave point pass does not serve.
 * The call invalidates the snapshot of vn_state_snapshot and the L-BFGS (f_k, g_k). */
int vn_set_field_learn(vn_engine* h, int32_t J, const int32_t* mask, const double* init, const double* lo, const double* hi, double lr);
/* The J amplitudes now (synchronises) and, when grad is not NULL, the amplitude gradient of the last gradient evaluation (zeros for
 * unmasked entries and before the first one).  Learning off: VN_ESTATE; J not the engine's: VN_EINVAL. */
int vn_get_field_amps(vn_engine* h, double* amp, double* grad, int32_t J);
/* Overwrites all J amplitudes (rounded to fp32, NOT clamped); the Adam slots stay.  Non-finite: VN_EINVAL; learning off: VN_ESTATE.
 * Invalidates the snapshot of vn_state_snapshot. */
int vn_set_field_amps(vn_engine* h, const double* amp, int32_t J);
/* Boundary data identification: the labels of a BC/IC row set are label0 + sum_j a_j B_j over a basis of J per-row streams (a
 * Dirichlet basis function on its edge's rows and zero elsewhere, an initial-condition basis function on the initial rows; the
 * engine does not know which stream is which), and the amplitudes a_j are learnt next to the parameters from the observations.
 * vn_set_bic_basis registers the basis of one row set: B_dev is [J, nB] fp32 on the device, stream-major (every stream contiguous,
 * nB as passed to vn_set_bic, also on a steady engine, which reads the first bDof entries of a stream); the streams are read on
 * every step and must stay valid while registered.  batch = -1: the rows of vn_set_bic; batch >= 0: that batch's own copy, which
 * needs a vn_set_batch_bic on that batch (VN_ESTATE without one).  B_dev == NULL or J == 0 clears the registration; vn_set_bic clears
 * the shared one, vn_set_batch_bic and vn_set_interior the batch's.  A call replaces the previous registration, also when it fails.
 * J > VN_BIC_MAX: VN_EINVAL.  The call invalidates the snapshot of vn_state_snapshot and the L-BFGS (f_k, g_k).
 * Without vn_set_bic_learn a registered basis is not read: the labels are those of vn_set_bic / vn_set_batch_bic. */
#define VN_BIC_MAX 64
int vn_set_bic_basis(vn_engine* h, int32_t batch, const float* B_dev, int32_t J);
/* The amplitudes are engine-wide, like those of vn_set_source_learn: while learning is on the engine owns ONE device vector of J
 * fp32 amplitudes (`init`, rounded once), their two Adam slots and a snapshot copy of the three.  Every evaluation of a batch whose
 * BC/IC set has a basis (vn_grad, vn_train_step / _epoch, vn_eval_loss, vn_objective_f64) first forms label[k] = label0[k] +
 * sum_j a_j B_j[k] (fp32, j ascending, one fused multiply-add per stream) and every kernel reads it in place of the set's labels; a
 * set whose basis has another J makes the step and the evaluations return VN_EINVAL.
 *   d loss / d a_j = - sum_k ubar_b[k] B_j[k],  ubar_b[k] = (k < bDof ? 2 w0 biDimVal / bDof : 2 w1 biDimVal / (nB - bDof)) (u_b[k] - label[k])
 * (k < bDof only on a steady engine) is formed inside vn_grad / vn_train_step / vn_train_epoch for the masked entries, in a fixed
 * order without atomics (two evaluations: the same bits).  Every step keeps its route: the generic and the layer-by-layer route
 * have u_b from their forward; the single launch, the two-pass sequence and the de-duplicated step run one forward of the BC/IC
 * rows ahead of their own launches.  vn_apply and the fused train steps update the masked entries with the arithmetic of the
 * parameters' Adam update (the engine's beta1, beta2, eps, the shared step counter, the rate `lr`), then clamp them to [lo, hi]
 * (+-inf: unbounded).  Unmasked entries take part in the labels at their init value and never change a bit.  On a batch whose set
 * has no basis the amplitude gradient reads 0, and the masked amplitudes follow the momentum in their slots.  The loss-only forms
 * and vn_objective_f64 run the mix only: no amplitude gradient is built in fp64.
 * vn_state_snapshot / vn_state_rollback carry amplitudes and slots; vn_state_size / _export / _import keep their layout.
 *   mask   J ints (non-zero: learnt), or NULL: learning off, everything freed, every result bit for bit what it was before.
 *   init, lo, hi   J doubles each.  Non-finite init, NaN bounds, lo > hi, lr not finite or <= 0, J outside 1..VN_BIC_MAX: VN_EINVAL.
 * Refused with VN_EUNSUPPORTED for the reasons of vn_set_source_learn: an RMSProp or L-BFGS engine; a handle that has a communicator
 * (and vn_comm_init while learning is on); a batch with vn_set_tf_weights / vn_set_causal (here, in those calls and in the steps);
 * and the 4-wave cross-check geometry (VN_KERNEL_FUSED).
 * The call invalidates the snapshot of vn_state_snapshot and the L-BFGS (f_k, g_k). */
int vn_set_bic_learn(vn_engine* h, int32_t J, const int32_t* mask, const double* init, const double* lo, const double* hi, double lr);
/* The J amplitudes now (synchronises) and, when grad is not NULL, the amplitude gradient of the last gradient evaluation (zeros for
 * unmasked entries and before the first one).  Learning off: VN_ESTATE; J not the engine's: VN_EINVAL. */
int vn_get_bic_amps(vn_engine* h, double* amp, double* grad, int32_t J);
/* Overwrites all J amplitudes (rounded to fp32, NOT clamped); the Adam slots stay.  Non-finite: VN_EINVAL; learning off: VN_ESTATE.
 * Invalidates the snapshot of vn_state_snapshot. */
int vn_set_bic_amps(vn_engine* h, const double* amp, int32_t J);
/* Flux boundary identification: the flux rows of vn_set_flux_bc evaluate r_k = n . grad_x u + coef[k] u - label[k] with
 *   label[k] = label0[k] + sum_{j < J_flux} a_j S_j[k],    coef[k] = coef0[k] + sum_{j >= J_flux} a_j S_j[k]
 * over a basis of J = J_flux + J_robin per-row streams (a stream is its basis function on the rows of its own edge and zero
 * elsewhere), and the amplitudes a_j -- a wall flux, a transfer coefficient -- are learnt next to the parameters from the
 * observations.  vn_set_fluxbc_basis registers the basis: S_dev is [J_flux + J_robin, nF] fp32 on the device, stream-major (every
 * stream contiguous, nF as passed to vn_set_flux_bc), the J_flux streams of the flux datum first; the streams are read on every step
 * and must stay valid while registered.  S_dev == NULL or J_flux + J_robin == 0 clears the registration, and so does vn_set_flux_bc.
 * A call replaces the previous registration, also when it fails.  J_flux + J_robin > VN_FBC_MAX or a negative count: VN_EINVAL; no
 * flux rows registered: VN_ESTATE.  The call invalidates the snapshot of vn_state_snapshot and the L-BFGS (f_k, g_k).
 * Without vn_set_fluxbc_learn a registered basis is not read: coef and label are those of vn_set_flux_bc. */
#define VN_FBC_MAX 64
int vn_set_fluxbc_basis(vn_engine* h, const float* S_dev, int32_t J_flux, int32_t J_robin);
/* While learning is on the engine owns ONE device vector of J fp32 amplitudes (`init`, rounded once), their two Adam slots and a
 * snapshot copy of the three, like vn_set_bic_learn.  Every evaluation (vn_grad, vn_train_step / _epoch, vn_eval_loss,
 * vn_objective_f64) first forms label and coef as above (fp32, from label0 / coef0, j ascending, one fused multiply-add per stream;
 * a part without streams is the caller's array) and the flux rows read them in place of the arrays of vn_set_flux_bc; a basis with
 * another J_flux + J_robin makes the step and the evaluations return VN_EINVAL.  With udbar[k] = 2 w0 biDimVal r_k / nF,
 *   d loss / d a_j = - sum_k udbar[k] S_j[k]  (j < J_flux),    d loss / d a_j = + sum_k udbar[k] u[k] S_j[k]  (j >= J_flux)
 * is formed inside vn_grad / vn_train_step / vn_train_epoch for the masked entries right after the flux rows' own pass, whose
 * buffers it reads, on every route, in a fixed order without atomics (two evaluations: the same bits).  The update, the clamp, the
 * unmasked entries, snapshot / rollback and the state layout are those of vn_set_bic_learn.  Without a registered basis the
 * amplitude gradient reads 0 and the masked amplitudes follow the momentum in their slots.  The loss-only forms and
 * vn_objective_f64 run the mix only: no amplitude gradient is built in fp64.
 *   mask   J ints (non-zero: learnt), or NULL: learning off, everything freed, every result bit for bit what it was before.
 *   init, lo, hi   J doubles each.  Non-finite init, NaN bounds, lo > hi, lr not finite or <= 0, J outside 1..VN_FBC_MAX: VN_EINVAL.
 * Refused with VN_EUNSUPPORTED for the reasons of vn_set_source_learn: an RMSProp or L-BFGS engine; a handle that has a communicator
 * (and vn_comm_init while learning is on); a batch with vn_set_tf_weights / vn_set_causal (here, in those calls and in the steps).
 * No kernel family is refused: the flux rows run their own pass on every route that registers them.
 * The call invalidates the snapshot of vn_state_snapshot and the L-BFGS (f_k, g_k). */
int vn_set_fluxbc_learn(vn_engine* h, int32_t J, const int32_t* mask, const double* init, const double* lo, const double* hi, double lr);
/* The J amplitudes now (synchronises) and, when grad is not NULL, the amplitude gradient of the last gradient evaluation (zeros for
 * unmasked entries and before the first one).  Learning off: VN_ESTATE; J not the engine's: VN_EINVAL. */
int vn_get_fluxbc_amps(vn_engine* h, double* amp, double* grad, int32_t J);
/* Overwrites all J amplitudes (rounded to fp32, NOT clamped); the Adam slots stay.  Non-finite: VN_EINVAL; learning off: VN_ESTATE.
 * Invalidates the snapshot of vn_state_snapshot. */
int vn_set_fluxbc_amps(vn_engine* h, const double* amp, int32_t J);
/* Regularisation of a learnt vector a of length J (kind: one of VN_LEARNT_*, the order of the sections above), with learnt mask M.
 * Quadratic prior Q(a) = 1/2 weight d^T R d, d = a - mean: R [J*J] symmetric positive semi-definite (NULL: the identity), mean [J]
 * (NULL: zeros), both host fp64, copied.  weight (R d)_j is added in fp64 to the folded gradient of the masked entries inside
 * vn_grad / vn_train_step / vn_train_epoch, before the cast to fp32 that feeds Adam; unmasked entries keep gradient 0, but their
 * fixed values enter d; d is formed from the values the gradient evaluation read.  vn_get_*(..., grad) then returns data gradient
 * plus prior gradient, and a vn_apply after a vn_grad steps on that gradient as it stands (the prior is not added a second time).
 * L1 shrinkage: l1 [J] host weights lambda_j >= 0 (NULL: none); the step of a masked entry ends in the proximal map
 *   c <- copysign(max(|c| - lr_t lambda_j, 0), c)
 * in fp32 after Adam's move and before the clamp, lr_t the bias-corrected rate of that step; it is no part of the gradient.  The
 * zero it produces keeps the sign of c: an entry shrunk from below reads -0.0, which compares equal to 0.  An
 * entry with lambda_j == 0, and every entry without a prior, keeps its arithmetic bit for bit.
 * The losses that vn_train_step, vn_eval_loss, vn_objective_f64 and the L-BFGS calls report do NOT contain Q or the L1 term: read
 * them with vn_get_learnt_prior.  weight == 0 with l1 == NULL clears the prior; any vn_set_<kind>_learn call, also a refused one, drops it.  The prior
 * is static data: the call may be repeated between steps to re-weight, and touches neither the values, the Adam slots nor the
 * snapshot.  It adds no launch to a step.
 * The vector not learnt: VN_ESTATE.  VN_EINVAL: kind outside 0..4; J not the registered length; weight negative or not finite; an
 * entry of R not finite, or R[i*J+j] != R[j*J+i]; an entry of mean not finite; an entry of l1 negative or not finite.  (Whether R
 * is positive semi-definite is the caller's to check: an indefinite R makes Q unbounded below.) */
#define VN_LEARNT_COEF 0
#define VN_LEARNT_SOURCE 1
#define VN_LEARNT_FIELD 2
#define VN_LEARNT_BIC 3
#define VN_LEARNT_FLUXBC 4
int vn_set_learnt_prior(vn_engine* h, int32_t kind, int32_t J, double weight, const double* R, const double* mean, const double* l1);
/* out[0] = Q and out[1] = sum_j lambda_j |a_j| at the current values (one launch; synchronises; changes no state); (0, 0) without a
 * prior.  The vector not learnt: VN_ESTATE. */
int vn_get_learnt_prior(vn_engine* h, int32_t kind, double out[2]);
/* OPTIONAL, no reference counterpart: learnt weight scales.  The network every kernel evaluates becomes an EFFECTIVE parameter
 * vector theta_eff = f(s_group) * V: a raw vector V of P floats and a short vector s of S scales, one per group of entries; an
 * entry in no group is the ordinary parameter.  The optimizer steps (V, s) through the chain rule.
 *   VN_REPARAM_RWF    random weight factorization (Wang, Wang, Perdikaris 2022): f(s) = exp(s); one group per output neuron of
 *                     EVERY layer, the output layer included; a group is column j of W_l, weights only (biases are in no group);
 *                     S = sum_{l=1..L+1} H[l].  `granularity` and `n` are ignored.
 *   VN_REPARAM_SLOPE  adaptive activation slopes (Jagtap, Kawaguchi, Karniadakis 2020): f(s) = n s with a fixed n >= 1; hidden
 *                     layers only; a group covers weights AND bias: column j of W_l with b_l[j] (VN_REPARAM_PER_NEURON,
 *                     S = sum_{l<=L} H[l]) or all of W_l and b_l (VN_REPARAM_PER_LAYER, S = L).
 *   VN_REPARAM_NONE   clears: theta keeps its current effective values and the slots of V are the slots of theta again.
 * The scales are ordered by layer, then by neuron.  With g = d loss / d theta_eff (what vn_grad leaves in the gradient buffer)
 *   g_V[p] = f(s_group(p)) g[p],     g_s[group] = f'(s_group) sum_{p in group} V[p] g[p]
 * and one step (vn_apply, vn_train_step, vn_train_epoch) is Adam on V with g_V in the engine's two slots, Adam on s with g_s in
 * two slots of S floats -- the engine's beta1, beta2, eps and step counter, the rate `lr` in place of cfg.lr -- and then
 * theta_eff = fl32(f(s_new)) * V_new: g_V uses the scale of BEFORE the step, theta_eff is rebuilt from the values of AFTER it.
 * The stage is one launch after the gradient reduction (vn_reparam.hip; sums in fp64 in a fixed order, no atomics: two steps on
 * the same state give the same bits); vn_train_step does not fold the update into the reduction and equals vn_grad + vn_apply
 * bit for bit.  No compute kernel changes: they read theta_eff, and so do vn_params_get, vn_eval_loss, vn_forward, vn_residual
 * and vn_objective_f64, whose gradient is with respect to theta_eff.
 * The call factorises the CURRENT parameters with s_init (S host doubles, rounded once to fp32): V = theta / f(s_init) on
 * grouped entries, then theta_eff = f * V (within 2 ulp of what it was; bit-equal where f == 1); it zeroes the two scale slots,
 * keeps m, v and the step counter, and invalidates the snapshot of vn_state_snapshot.
 * With scales registered: vn_params_set stores theta_eff and re-factorises it with the current s; vn_params_init draws the same
 * parameters as without, factorises them with the registered s_init and zeroes all four slots; vn_state_export / _import keep
 * their layout (theta_eff, m, v) -- on import V is re-factorised from theta with the current s, and a full restore calls
 * vn_set_reparam_state afterwards; vn_state_snapshot / _rollback carry V, s and the scale slots.
 * VN_EINVAL: S not the mode's count; a non-finite s_init; slope with n < 1 (or not finite) or an s_init of 0; lr negative or not
 * finite; an unknown mode or granularity.  VN_EUNSUPPORTED: an RMSProp or L-BFGS engine (their state would live in theta_eff
 * space); a handle with a communicator (and vn_comm_init while scales are registered); the layer-by-layer route and any network
 * outside the fused / generic kernels' range (at most 8 hidden layers, widths <= 64, d_in <= 8).
 * Without a registration nothing is launched, nothing is allocated and every result is bit for bit what it is without this call. */
enum { VN_REPARAM_NONE = 0, VN_REPARAM_RWF = 1, VN_REPARAM_SLOPE = 2 };
enum { VN_REPARAM_PER_NEURON = 0, VN_REPARAM_PER_LAYER = 1 };
int vn_set_reparam(vn_engine* h, int32_t mode, int32_t granularity, double n, const double* s_init_host, int32_t S, double lr);
/* V [P], s [S], fl32(f(s)) [S] as last formed and the scale slots [2 S] (first moment, then second) into host floats; any pointer
 * may be NULL.  Synchronises.  No registration: VN_ESTATE. */
int vn_get_reparam(vn_engine* h, float* V_host, float* s_host, float* f_host, float* slots_host);
/* Overwrites V, s and the scale slots (any pointer may be NULL: that part stays), then rebuilds theta_eff = fl32(f(s)) * V.
 * Synchronises; invalidates the snapshot.  A non-finite s: VN_EINVAL; no registration: VN_ESTATE. */
int vn_set_reparam_state(vn_engine* h, const float* V_host, const float* s_host, const float* slots_host);
/* (g_V [P], g_s [S]) of the gradient buffer as it stands (after a vn_grad), by the stage's dry form: no state changes.  Either
 * pointer may be NULL.  Synchronises.  No registration: VN_ESTATE. */
int vn_reparam_grad(vn_engine* h, float* gV_host, float* gs_host);
/* updateDictFields('trainW') (VarNetUtility.py:921-922); the caller applies the
 * w[0:2] /= batchNum*puNum rule (VarNetUtility.py:900-901). */
int vn_set_weights(vn_engine* h, const double w[3]);

/* Optional externally owned gradient buffer of P+4 floats (gradient | loss, BC, IC, var) so
 * that the host can all-reduce it (tower gradient SUM, TFModel.py:342-377) between vn_grad
 * and vn_apply.  NULL restores the internal buffer. */
int vn_bind_grad_buffer(vn_engine* h, float* dev);

/* compute_gradients(loss) (TFModel.py:709): forward, weak-form loss, backward for `batch`;
 * leaves d loss/d theta and the 4 loss scalars in the gradient buffer. */
int vn_grad(vn_engine* h, int32_t batch);
/* OPTIONAL (the reference's updateWeights, VarNet.py:1373, cannot run): per-term gradients and their statistics, the input of an
 * adaptive loss-balancing rule (vn_balance.hip).  The objective of vn_grad is w0 BC + w1 IC + w2 var + lambda O, linear in the
 * weights, so the gradient of one term is what vn_grad leaves under a one-hot weight vector. */
#define VN_TERM_BC 0
#define VN_TERM_IC 1
#define VN_TERM_VAR 2
#define VN_TERM_OBS 3
#define VN_TERM_N 4
/* the statistics alone, on caller vectors: T_dev [K][n] fp32, 1 <= K <= VN_TERM_N, n >= 1.
 * stats [K][3] = {sumsq, sumabs, maxabs}, gram [K][K]; host doubles; synchronises.
 * All sums in fp64 from exact products, in an order that depends on n alone (no atomics; not on the card): two calls give the same
 * bits.  gram is symmetric and gram[a][a] is sumsq[a], the same bits.  A NaN entry makes the sums it enters NaN; maxabs ignores it.
 * VN_EINVAL: K outside 1..VN_TERM_N, n < 1, a null pointer.  VN_ENOMEM: the 150 KB of partials do not fit. */
int vn_term_stats(vn_engine* h, const float* T_dev, int32_t K, int64_t n, double* stats, double* gram);
/* per-term gradients of the objective of vn_grad over `batches[0..n)`, and their statistics.
 * G_k is the gradient buffer vn_grad(batch) leaves with the weights (1,0,0), (0,1,0), (0,0,1) and lambda = 0 for VN_TERM_BC,
 * VN_TERM_IC, VN_TERM_VAR, and with (0,0,0) and lambda = 1 for VN_TERM_OBS, summed over the listed batches in list order in fp32
 * (the first batch is copied, every later one added with one rounding).  value[k] is the matching unweighted scalar (BC, IC, var of
 * the gradient buffer's tail, O of the misfit slot) summed over the batches in double.  Flux rows and periodic pairs belong to
 * VN_TERM_BC, as they do in the loss.  Every evaluation is vn_grad's own (the learnt-vector mixes first, the batch's route, every
 * registered extension, no update folded in); with weight scales registered the gradient is with respect to theta_eff.
 * A term outside `term_mask` (bit k = term k) or without rows (no IC rows on a steady problem, no observations) is skipped: its
 * rows of stats, gram, value and G_dev are zeros.  stats, gram and value are host doubles, none may be NULL; G_dev (device,
 * [VN_TERM_N][P] floats) may be.
 * State: on return the weights and lambda are the caller's, bit for bit; theta, m, v, the step counter, a loss accumulator, the
 * learnt vectors and their slots, (V, s) and the scale slots and the snapshot are untouched.  CLOBBERED until the next vn_grad: the
 * gradient buffer (a bound one included), the loss scalars, the misfit slot and the learnt vectors' gradient read-outs, which are
 * left as the last evaluated term wrote them.  One synchronisation, at the end.
 * VN_EUNSUPPORTED: an L-BFGS engine (its (f_k, g_k) would be disturbed); a handle with a communicator (each term would need its
 * own all-reduce).  VN_EINVAL: a null or empty batch list, a batch id that names no registered batch, a term_mask with no bit
 * or a bit >= VN_TERM_N.  Whatever vn_grad refuses is refused with its code, the weights restored.  VN_ENOMEM: the
 * [VN_TERM_N][P] scratch, allocated at the first call and freed by vn_destroy, does not fit. */
int vn_term_grads(vn_engine* h, const int32_t* batches, int32_t n, uint32_t term_mask,
                  double* stats /*[VN_TERM_N][3]*/, double* gram /*[VN_TERM_N][VN_TERM_N]*/,
                  double* value /*[VN_TERM_N]*/, float* G_dev /*[VN_TERM_N][P] or NULL*/);
/* optimizer.apply_gradients (TFModel.py:313): TF-1 Adam (or RMSProp: decay 0.9, momentum 0, eps 1e-10,
 * mean-square slot initialised to ones) step from the gradient buffer. */
int vn_apply(vn_engine* h);
/* sess.run([optMinimize, loss]) (VarNetUtility.py:1044) = vn_grad + vn_apply.  If
 * loss_out_dev != NULL the pre-update loss is copied there (device scalar, async). */
int vn_train_step(vn_engine* h, int32_t batch, float* loss_out_dev);
/* ManageTrainData.optimIter (VarNetUtility.py:1021-1047) for one process: `n` consecutive steps
 * (vn_grad + vn_apply) over batches[0..n), the pre-update loss of each step ADDED to the device scalar
 * *loss_acc_dev (may be NULL).  One host call per epoch instead of four per mini-batch; no sync. */
int vn_train_epoch(vn_engine* h, const int32_t* batches, int32_t n, float* loss_acc_dev);

/* OPTIONAL, no reference counterpart: one L-BFGS iteration on the objective "vn_grad of `batch`" (whatever route, de-duplication
 * map and flux rows that batch has), for engines created with optimizer = VN_OPT_LBFGS; VN_ESTATE on Adam / RMSProp engines,
 * VN_EUNSUPPORTED on a handle with a communicator.  On such an engine vn_apply, vn_train_step, vn_train_epoch, vn_state_snapshot
 * and vn_state_rollback return VN_ESTATE.  Full-batch, deterministic objectives only: consecutive calls must see the same one.
 *   State (device, fp32 vectors of length P, allocated at the first call -- VN_ENOMEM if they do not fit): theta_k, the
 *   optimizer's own copy of g_k and of the loss scalars f_k (a caller's vn_grad between two calls does not disturb them), the
 *   direction, and a ring of up to m = VN_LBFGS_HISTORY pairs (s_i, y_i) in m + 1 slots per family (the spare slot takes the pair
 *   of an accepted step before its curvature test): (2 m + 5) P floats in all.
 *   1. (f_k, g_k) not valid: vn_grad(batch) at theta_k first (an evaluation, not a trial).
 *   2. Direction: the two-loop recursion over the stored pairs, newest first, gamma = s.y / y.y of the newest pair (1 without
 *      pairs), d = -H g_k; run in its Gram form on the coefficients of d in the basis [s_i, y_i, g_k], every inner product
 *      accumulated in fp64 in a fixed order (bitwise repeatable).  g_k.d >= 0: the ring is dropped and d = -g_k.
 *   3. Backtracking Armijo search: t0 = min(1, 1/|g_k|_1) with an empty ring, else 1; trial j runs vn_grad at
 *      fl32(theta_k + t d), t = t0 2^-j, j < max_trials; the first trial whose loss is finite and <= f_k + 1e-4 t g_k.d is
 *      accepted.  One 16-byte copy and one synchronisation per trial; the decision is the host's, in double.
 *   4. Accepted: theta_{k+1} is the trial point, s = fl32(theta_{k+1} - theta_k), y = fl32(g_{k+1} - g_k); the pair enters the
 *      ring (evicting the oldest) iff s.y > 1e-10 |s|_2 |y|_2 (decided on the device when the next direction is formed); the step
 *      counter moves by one; the gradient buffer holds g_{k+1} and the loss scalars of theta_{k+1}.
 *   5. No trial accepted: theta is restored to theta_k bit for bit, the step counter does not move; status 1 with pairs in the
 *      ring (they are dropped: the next call is a steepest-descent iteration), status 2 ("stalled") with an empty ring.  Both
 *      return VN_OK.
 * info = {status, f_k, f_{k+1}, BC, IC, var at theta_{k+1}, accepted t, trials used, g_k.d, pairs the direction was formed from}
 * (after a status != 0: f_{k+1} = f_k, the components of theta_k, t = 0).
 * vn_params_init, vn_params_set, vn_state_import, vn_set_bic, vn_set_flux_bc, vn_set_interior / vn_set_dedup /
 * vn_set_batch_bic / vn_set_reaction / vn_set_nlflux / vn_set_nldiff of that batch, a call with another `batch` than the previous one and vn_set_weights invalidate (f_k, g_k) and
 * drop the ring -- vn_set_weights when the call finds other weights than (f_k, g_k) were evaluated with (weights changed and put
 * back between two calls, as the monitors of VarNet.train do, leave the objective and therefore the optimizer alone).
 * vn_state_export writes the two slots as zeros and vn_state_import ignores them; the ring is not part of a checkpoint. */
int vn_lbfgs_step(vn_engine* h, int32_t batch, int32_t max_trials, double info[10]);
/* OPTIONAL, default off: with `on` != 0 vn_lbfgs_step takes f_k and each trial's loss (and the BC, IC, var it reports) from the
 * loss-only form of vn_objective_f64 at the trial point -- a 32-byte read-back of doubles instead of 16 bytes of floats -- so the
 * Armijo test is not limited by the resolution of an fp32 loss.  The gradient, the direction, the ring and every other rule above
 * are unchanged; with it off vn_lbfgs_step is bitwise what it is without this call.  A change of the flag invalidates (f_k, g_k).
 * VN_ESTATE on Adam / RMSProp engines; VN_EUNSUPPORTED where vn_objective_f64 is. */
int vn_lbfgs_loss64(vn_engine* h, int on);

/* ManageTrainData.splitLoss (VarNetUtility.py:1080-1088): out = {loss, BCloss, ICloss,
 * varLoss} (host doubles), lossVec_dev [n_k] or NULL.  Synchronises. */
int vn_eval_loss(vn_engine* h, int32_t batch, double out[4], float* lossVec_dev);

/* OPTIONAL, no reference counterpart: the objective of vn_grad(batch) in double precision.
 * Exactly the objective vn_grad / vn_eval_loss define for the batch as registered -- interior rows (per-row N_rows / dNt_rows,
 * per-test-function detJ_dev, n_k == 0 included), FE table, integW, source term, the BC/IC rows of vn_set_bic or the batch's own
 * vn_set_batch_bic copy, the flux rows of vn_set_flux_bc, the weights of vn_set_weights, steady or time-dependent -- with the
 * registered fp32 arrays widened exactly and everything after that in fp64: layer products (fp64 matrix pipe), exp / tanh and
 * the division, quadrature sums, squares and means, the reverse pass, and every reduction in a fixed order without
 * floating-point atomics (two calls return the same bits).  A de-duplication map on the batch is ignored: the row-wise sum is
 * evaluated (the two formulations are the same mathematics).
 *   theta_dev    P doubles on the device, or NULL: the engine's own fp32 parameters, widened
 *   grad_dev     P doubles, d loss / d theta, or NULL: loss only (no reverse launch is enqueued)
 *   lossVec_dev  n_k doubles, or NULL
 *   out          {loss, BC, IC, var} as host doubles
 * Synchronises, like vn_eval_loss.  Changes no engine state (parameters, optimizer slots, step counter, gradient buffer, the
 * L-BFGS validity flags, the communicator) and issues no collective.
 * Range: 1..6 hidden layers of width <= 64 (ragged widths included), d_in <= 8, dim <= 3, one activation (sigmoid or tanh), any
 * integ_num; networks outside VN_KMAX_* (the layer-by-layer route, 7-8 hidden layers, mixed activations): VN_EUNSUPPORTED.
 * An unregistered batch: VN_ESTATE; out == NULL: VN_EINVAL. */
int vn_objective_f64(vn_engine* h, int32_t batch, const double* theta_dev,
                     double* grad_dev, double* lossVec_dev, double out[4]);

/* runSession(['model']) (VarNetUtility.py:1123-1128,1142; VarNet.py:1930): u = model(X). */
int vn_forward(vn_engine* h, const float* X_dev, int64_t n, float* u_dev);
int vn_forward_f64(vn_engine* h, const double* X_dev, int64_t n, double* u_dev);
/* NNModel.modelGrad's tf.gradients(model(Input), Input) (TFModel.py:536-541): u = model(X) [n] and
 * g = d u / d X[:, :dim] [n, dim] in one pass (value forward + value-adjoint sweep to the inputs, 2 F_pt per point).
 * Networks the 8-wave fused kernel serves (vn_kernel_path == VN_KERNEL_FUSED16), dim <= 3; VN_EUNSUPPORTED otherwise. */
int vn_forward_grad(vn_engine* h, const float* X_dev, int64_t n, float* u_dev, float* g_dev);
/* runSession(['model','residual']) (VarNetUtility.py:1130-1142; TFModel.py:743-754):
 * res = -u_t + diff*Lap(u) - (vel - diff_dx).grad(u) + source.  diff [n], vel [n,dim],
 * source [n] or NULL, diff_dx [n,dim] or NULL.  fp32 and fp64 forms. */
int vn_residual(vn_engine* h, const float* X_dev, const float* diff_dev, const float* vel_dev,
                const float* source_dev, const float* diff_dx_dev, int64_t n, float* u_dev,
                float* res_dev);
int vn_residual_f64(vn_engine* h, const double* X_dev, const double* diff_dev,
                    const double* vel_dev, const double* source_dev, const double* diff_dx_dev,
                    int64_t n, double* u_dev, double* res_dev);

/* ---- towers: one process per GPU, gradient SUM over RCCL --------------------------------------------
 * Replaces TFNN.towerSetup / sum_grads (TFModel.py:253-289, 342-377): the reference builds one NNModel per
 * device in ONE process and reduces the per-tower gradients with tf.reduce_sum on a controller device.
 * Here every GPU has its own process and handle; the handles are joined into one RCCL communicator and the
 * only collective per step is a SUM all-reduce of the P+4 floats of the gradient buffer
 * (gradient | loss, BC, IC, var -- the tower loss sums of TFModel.py:315-319 ride along).
 *   rank 0:    vn_comm_unique_id(id)            -> 128 opaque bytes (ncclUniqueId), host memory
 *   host:      ship `id` to every rank (any side channel: MPI, a TCP store, torch.distributed ...)
 *   all ranks: vn_comm_init(h, rank, world, id) -> collective; returns when every rank has joined
 * With a communicator attached, vn_train_step / vn_train_epoch run gradient -> all-reduce -> optimizer on
 * the engine stream without a host round trip; vn_grad + vn_allreduce_grad + vn_apply is the same step in
 * three calls.  RCCL is loaded at run time (librccl.so.1 by SONAME, or $VN_RCCL_LIB); without it the vn_comm_* 
 * entry points return VN_EUNSUPPORTED and everything else works. */
#define VN_COMM_ID_BYTES 128
/* VN_OK if RCCL can be loaded in this process (no collective, no GPU work): lets every rank probe locally BEFORE any
 * rank enters the collective bootstrap, so that all ranks take the same route. */
int vn_comm_available(void);
/* Version of the RCCL library this process loaded, as ncclGetVersion reports it (e.g. 22205 = 2.22.5); VN_EUNSUPPORTED
 * when it cannot be loaded.  No collective, no GPU work: a first multi-GPU record can say which library summed the gradient. */
int vn_comm_version(int32_t* version_out);
int vn_comm_unique_id(void* id_out_host);
int vn_comm_init(vn_engine* h, int32_t rank, int32_t world, const void* unique_id_host);
/* Ranks RCCL reports for the attached communicator (1 if none); rank_out may be NULL. */
int vn_comm_size(const vn_engine* h, int32_t* world_out, int32_t* rank_out);
int vn_comm_destroy(vn_engine* h);
/* ncclCommInitRank has no timeout.  A caller that runs vn_comm_init on a helper thread and stops waiting for it (a peer is
 * wedged) calls vn_comm_abandon from the thread that drives the engine: from then on the engine has no communicator and
 * takes none -- a vn_comm_init that is still running leaves its communicator aside when it returns (VN_ESTATE), one that had
 * come up is withdrawn WITHOUT ncclCommDestroy (which could block on the wedged peer) -- so vn_train_step / vn_train_epoch
 * never enqueue a collective on it.  Idempotent.  After abandonment do not call vn_destroy while a vn_comm_init may still
 * be running (it writes into the handle): leave the handle to the process exit. */
int vn_comm_abandon(vn_engine* h);
/* Failure under a communicator.  vn_train_step / vn_train_epoch on a handle with a communicator are gradient -> all-reduce
 * -> update.  When the gradient fails on ONE rank (bad batch index, HIP error) that rank returns its error without entering
 * the collective and with parameters, optimizer slots and step counter untouched; the all-reduce its peers enqueued for
 * that step never completes.  A failed step under a communicator therefore ends the JOB: the failing process must exit
 * non-zero and its launcher must end the peers (varnet_amd/launch.py and torch.distributed.run both do; the former also
 * reports the failing rank's last stage).  Nothing in the library waits for a dead peer on the host: the peers' host
 * threads block at their next synchronisation, not inside vn_train_*.
 * In-place SUM all-reduce of the gradient buffer over the communicator, on the engine stream. */
int vn_allreduce_grad(vn_engine* h);

/* Adam step counter (global_step, TFModel.py:312). */
int vn_get_step(const vn_engine* h, int64_t* step);

/* Mean duration (ms, HIP events on the engine stream) of the vn_allreduce_grad calls recorded since
 * vn_profile_begin (call before vn_profile_end; synchronises). */
int vn_profile_comm(vn_engine* h, double* mean_ms, int64_t* calls);

/* Which kernel family VN_KERNEL_AUTO resolved to for this network (VN_KERNEL_GENERIC / _FUSED / _FUSED16);
 * *two_pass = 1 when integ_num > 128 runs the fused kernel twice around the row-wise epilogue. */
int vn_kernel_path(const vn_engine* h, int32_t* kernel_out, int32_t* two_pass_out);

/* Name / mean duration (ms, HIP events on the engine's stream) of the dominant kernel of the
 * last `vn_profile_begin` .. `vn_profile_end` window: used by bench.py for the roofline
 * object.  vn_profile_end synchronises. */
int vn_profile_begin(vn_engine* h);
int vn_profile_end(vn_engine* h, double* mean_ms, int64_t* launches, char* name, int32_t name_len);

/* Measurement aid (bench.py `roofline.peak_measured`, `issue_model`), ~30 ms, synchronises: what this GPU sustains on
 * the two instruction streams the fused kernels are priced against, two waves per SIMD on every SIMD.
 * out[0] fp32 MFMA TFLOP/s (v_mfma_f32_16x16x4_f32 loop; datasheet 157.3), out[1] ms of that launch,
 * out[2] cycles per independent v_fma_f32 per SIMD (at the clock out[3]), out[3] GHz implied by 32 cycles per MFMA,
 * out[4] ms of the vector launch. */
int vn_debug_calibrate(vn_engine* h, double out[5]);

/* The same for the fp64 matrix pipe (vn_forward_f64 / vn_residual_f64 run on v_mfma_f64_16x16x4_f64): out[0] fp64 MFMA
 * TFLOP/s of a loop of independent MFMAs, out[1] ms of that launch, out[2] cycles one MFMA occupies a SIMD at the clock
 * `ghz` (vn_debug_calibrate's out[3]; 0 = not asked). */
int vn_debug_calibrate_f64(vn_engine* h, double ghz, double out[3]);

/* Test aid: route = 1 sends vn_residual, vn_residual_f64 and vn_forward_f64 of THIS engine to the per-thread kernels of
 * vn_pointwise.hip (the independent implementation the matrix-pipe kernels are checked against); route = 2 keeps vn_forward and
 * vn_residual on the f32-MFMA kernels (vn_pgrad16 / vn_taylor16) where the bf16-piece kernels of vn_split16.hip would run
 * (A/B and cross-check of the two matrix-pipe forms; exists in the tests' cross-check library only); 0 restores the automatic choice;
 * | 4: vn_set_dedup keeps the CSR-ordered copy of gcoef although it found it periodic in integ_num (the general path of the two
 * assembly kernels, cross-checked bit for bit against the table path); | 8: vn_eval_loss of a batch that carries a de-duplication map
 * runs the row-wise forward anyway (cross-check of the loss-only form of the de-duplicated assembly).  (Round 5: an environment variable
 * read on every call.) */
int vn_debug_point_route(vn_engine* h, int32_t route);

/* Diagnostic builds (-DVN_STAMPS) only: per-phase s_memtime cycle sums of workgroup 0 of the last
 * fused launch (zeros otherwise).  Never part of a timed or shipped build. */
int vn_debug_stamps(vn_engine* h, unsigned long long out[8]);

#ifdef __cplusplus
}
#endif
#endif /* VARNET_HIP_H */
