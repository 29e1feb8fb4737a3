"""
Host-side tables of the value-regime parity suite (tests/test_values_host.py, tests/test_values_gpu.py): the nets, the value
transforms, their seeded inputs and parameters, the fp64 / fp32 oracle evaluations of them (each computed once and shared:
every evaluation is lru_cached and must not be modified by a caller), and a NumPy float32 restatement of the loss and its
gradient with the kernels' activation formula.  Plain module: no GPU, no pytest marks.

Every other parity suite draws its numbers from one box (inputs U(-1, 1), coefficients N(0, 1), parameters Glorot + 0.05 N(0, 1),
theta scaled by at most 2.5).  The transforms below move a case out of that box, one direction at a time:

    plain        nothing: the control case
    planted      in every hidden layer of width wd the biases of units 0, 1, wd-2, wd-1 become +100, -100, -200, +200: these
                 units sit at |c z| > 128 (c = -log2 e for the sigmoid, -2 log2 e for tanh), where exp2 is +inf, zero or a
                 denormal and the stored activation is exactly 0, 1 or +-1; at width 50 the last two are the folded edge
                 features 48 and 49 of the 8-wave kernels
    planted800   the same with +-800 / +-1600: exp overflows in double (the fp64 entry points only)
    steep4       theta x 4: broad moderate saturation
    offset100    Input and biInput + 100 in every column, b1 -= 100 sum_i W1[i, :] in fp32: the fp64 function is the plain one
                 (up to the fp32 rounding of b1), the first layer cancels terms ~100 x its result
    scaled_down  gcoef, source, biLabel x 1e-4
    scaled_up    the same x 1e4
    mixed        gcoef x 1e-3, source x 1e3, loss weights [3e3, 2e-3, 5]
    shrunk       theta x 2^-10: every hidden pre-activation is tiny, the cancellation regime of tanh = 2 sigmoid(2z) - 1
    tiny         loss weights x 1e-8: |g| near Adam's eps (the optimizer-step tests only)

theta = glorot_init(seed 4) + 0.05 N(0, 1) from default_rng(6), in fp32.  The rows of every case share points (the map is
built as tests/fuzz_terms.case_inputs builds it), so that the de-duplicated step sees the same rows as every other route.

The GPU bars (tests/parity_cases.py: loss 1e-5, gradient and lossVec 1e-4) apply unwidened as long as the fp32 oracle stays
within a quarter of them of the fp64 oracle: tests/test_values_host.py asserts that for every (net, transform, activation)
of this module, on the loss, each of its components and every gradient block.  Five (net, transform) pairs break the condition
at the default scale, or hold it with no margin to spare, and run another transform scale instead (SCALE_OVERRIDE, with the
measured figures; offset 16 or 50 in place of 100 on three nets, theta x 2^-7 on 2x96, data x 1e-5 on 3x20): never a wider bar.
test_values_host.py scales its cancellation check with the offset (first-layer terms >= offset / 2 times their result).
"""
import functools

import numpy as np
import torch

from oracle import tf1_graph as og

NB, BDOF, BIDIMVAL = 50, 30, 2.0
ACTS = ('sigmoid', 'tanh')
TRANSFORMS = ('plain', 'planted', 'steep4', 'offset100', 'scaled_down', 'scaled_up', 'mixed', 'shrunk')
F64_TRANSFORMS = TRANSFORMS + ('planted800',)               # the fp64 entry points
STEP_TRANSFORMS = ('scaled_down', 'scaled_up', 'mixed', 'tiny')      # one optimizer step
POINT_TRANSFORMS = ('planted', 'steep4', 'offset100', 'shrunk')
PLANT = (100.0, -100.0, -200.0, 200.0)                      # units 0, 1, wd-2, wd-1
SCALE = {'steep4': 4.0, 'shrunk': 2.0 ** -10, 'offset100': 100.0, 'scaled_down': 1e-4, 'scaled_up': 1e4}
# (net name, transform) -> scale, where the default breaks the quarter-bar condition (measured deviation of the fp32 oracle at the
# default scale | at the override, as a fraction of the quarter bar)
SCALE_OVERRIDE = {
    ('5x50', 'offset100'): 16.0,               # tanh varLoss 5.6e-6 (2.2) | 3.4e-7 (0.14)
    ('2x96', 'offset100'): 50.0,               # tanh varLoss 2.4e-6 (0.95: no margin) | 2.1e-7 (0.08)
    ('3x50_q216', 'offset100'): 50.0,          # tanh varLoss 2.0e-6 (0.80: no margin) | 9.0e-7 (0.36)
    ('2x96', 'shrunk'): 2.0 ** -7,             # sigmoid W2 1.3e-4 (5.0) | 1.1e-5 (0.44); max |z| stays at 1.2e-2
    ('3x20', 'scaled_down'): 1e-5,             # tanh bo 2.4e-5 (0.96: no margin) | 1.5e-5 (0.60)
}

# name -> d_in, dim, widths, integNum, n_k, time dependent; the smallest shapes that reach each kernel class
NETS = {
    '3x20':      (3, 2, [20] * 3,       16,  40, True),     # f32 MFMA fused kernel
    '2x32':      (3, 2, [32, 32],       16,  40, True),     # KS = 8, thin_bias
    '5x50':      (3, 2, [50] * 5,       64,  9,  True),     # bf16 sweeps with both folded edge features
    '40_50_34':  (3, 2, [40, 50, 34],   16,  30, True),     # bf16 sweeps, mixed fold content
    '4x60':      (3, 2, [60] * 4,       64,  9,  True),     # KS = 16
    '2x64':      (3, 2, [64, 64],       64,  6,  True),     # 64 wide
    '3x50_q216': (3, 2, [50] * 3,       216, 7,  True),     # two-pass route
    '2x96':      (3, 2, [96, 96],       16,  20, True),     # vn_wide tile kernels
    '272_260':   (3, 2, [272, 260],     16,  8,  True),     # GEMM form
    '4x50_mor':  (6, 2, [50] * 4,       16,  30, True),     # MOR-shaped fused net
    '5x50_steady': (1, 1, [50] * 5,     6,   77, False),    # steady branch
}
POINT_NETS = {'3x20': (3, 2, [20] * 3), '5x50': (3, 2, [50] * 5), '2x64': (3, 2, [64, 64]), '4x60': (3, 2, [60] * 4)}
POINT_N = (17, 128, 1000)


def scale(net, transform):
    return SCALE_OVERRIDE.get((net, transform), SCALE[transform])


def act_const(act):
    """c of the kernels' activation  rcp(1 + exp2(c z))."""
    return -2.8853900817779268 if act == 'tanh' else -1.4426950408889634


def planted_units(wd):
    return (0, 1, wd - 2, wd - 1)


def bias_slices(d_in, widths):
    """Slices of the hidden layers' bias vectors in the flat layout [W1, b1, W2, b2, ..., wo, bo]."""
    out, off = [], 0
    for i, o in og.layer_dims(d_in, widths)[:-1]:
        off += i * o
        out.append(slice(off, off + o))
        off += o
    return out


def base_theta(d_in, widths):
    flat = og.glorot_init(d_in, widths, 4)
    return (flat + 0.05 * np.random.default_rng(6).standard_normal(flat.size).astype(np.float32)).astype(np.float32)


def transform_theta(flat, d_in, widths, transform, net=None):
    """The transform's share on the parameters (fp32 in, fp32 out)."""
    flat = np.array(flat, dtype=np.float32)
    if transform in ('planted', 'planted800'):
        k = np.float32(8.0 if transform == 'planted800' else 1.0)
        for s, wd in zip(bias_slices(d_in, widths), widths):
            for u, b in zip(planted_units(wd), PLANT):
                flat[s.start + u] = k * np.float32(b)
    elif transform in ('steep4', 'shrunk'):
        flat = (np.float32(scale(net, transform)) * flat).astype(np.float32)
    elif transform == 'offset100':
        W1 = flat[:d_in * widths[0]].reshape(d_in, widths[0])
        s = bias_slices(d_in, widths)[0]
        flat[s] = flat[s] - np.float32(scale(net, transform)) * W1.sum(axis=0, dtype=np.float32)
    return flat


def synth(seed, d_in, dim, integNum, n_k, source=True):
    """Inputs as tests/parity_cases.synth draws them (the same box), on NB boundary / initial rows."""
    rng = np.random.default_rng(seed)
    n = n_k * integNum
    d = dict(Input=rng.uniform(-1, 1, (n, d_in)).astype(np.float32), gcoef=rng.standard_normal((n, dim)).astype(np.float32),
             source=rng.standard_normal((n, 1)).astype(np.float32) if source else None,
             N1=rng.uniform(0, 1, integNum).astype(np.float32), dNt1=rng.standard_normal(integNum).astype(np.float32),
             integW=None, detJ=np.float32(0.137), biInput=rng.uniform(-1, 1, (NB, d_in)).astype(np.float32),
             biLabel=rng.standard_normal((NB, 1)).astype(np.float32), w=np.array([3.0, 2.0, 5.0]))
    d['N'] = np.tile(d['N1'], n_k).reshape(n, 1)
    d['dNt'] = np.tile(d['dNt1'], n_k).reshape(n, 1)
    return d


@functools.lru_cache(maxsize=None)
def inputs(net, transform):
    """(inputs dict, shared-point map (Xu, uid, rowptr, rowidx)) of a net under a transform."""
    d_in, dim, widths, q, n_k, td = NETS[net]
    idx = list(NETS).index(net)
    d = synth(300 + idx, d_in, dim, q, n_k)
    r5 = np.random.default_rng(5000 + idx)
    n = n_k * q
    U = max(1, n // int(r5.integers(1, 9)))
    uid = r5.integers(0, U, n).astype(np.int32)
    uid[:U] = np.arange(U)                      # every unique point is used
    r5.shuffle(uid)
    Xu = d['Input'][:U].copy()
    f32 = np.float32
    if transform == 'offset100':
        Xu = (Xu + f32(scale(net, transform))).astype(f32)
        d['biInput'] = (d['biInput'] + f32(scale(net, transform))).astype(f32)
    elif transform in ('scaled_down', 'scaled_up'):
        for k in ('gcoef', 'source', 'biLabel'):
            d[k] = (f32(scale(net, transform)) * d[k]).astype(f32)
    elif transform == 'mixed':
        d['gcoef'] = (f32(1e-3) * d['gcoef']).astype(f32)
        d['source'] = (f32(1e3) * d['source']).astype(f32)
        d['w'] = np.array([3e3, 2e-3, 5.0])
    elif transform == 'tiny':
        d['w'] = 1e-8 * d['w']
    d['Input'] = Xu[uid]
    rowptr = np.zeros(U + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(np.bincount(uid, minlength=U))
    return d, (Xu, uid, rowptr, np.argsort(uid, kind='stable').astype(np.int32))


@functools.lru_cache(maxsize=None)
def theta(net, transform):
    d_in, dim, widths, q, n_k, td = NETS[net]
    return transform_theta(base_theta(d_in, widths), d_in, widths, transform, net)


def _kw(net, d, f):
    d_in, dim, widths, q, n_k, td = NETS[net]
    cv = lambda a: None if a is None else np.asarray(a).astype(f)
    return dict(Input=cv(d['Input']), gcoef=cv(d['gcoef']), source=cv(d['source']), N=cv(d['N']), dNt=cv(d['dNt']), integW=None,
                intShape=[n_k, q], detJ=float(d['detJ']), detJvec=False, biInput=cv(d['biInput']), biLabel=cv(d['biLabel']),
                bDof=BDOF, biDimVal=BIDIMVAL, w=d['w'], dim=dim, time_dependent=td, is_source=True, integWflag=False)


@functools.lru_cache(maxsize=None)
def oracle(net, transform, act, fp64=True):
    """(result dict, gradient [P] float64) of the oracle in fp64, or in fp32 (the conditioning estimate)."""
    d_in, dim, widths, q, n_k, td = NETS[net]
    f, dtype = (np.float64, torch.float64) if fp64 else (np.float32, torch.float32)
    res, g = og.loss_and_grad(theta(net, transform).astype(f), d_in, widths, dtype, activation=act,
                              **_kw(net, inputs(net, transform)[0], f))
    return res, np.asarray(g, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def adam_step(net, transform, act):
    """One TF-1 Adam step in fp64 from theta: (parameters after it, oracle result at them)."""
    d_in, dim, widths, q, n_k, td = NETS[net]
    th0 = theta(net, transform).astype(np.float64)
    th1 = og.TF1Adam(th0.size, lr=1e-3, dtype=np.float64).step(th0, oracle(net, transform, act)[1])
    res, _ = og.loss_and_grad(th1, d_in, widths, torch.float64, activation=act, **_kw(net, inputs(net, transform)[0], np.float64))
    return th1, res


# -- the kernels' activation formula in float32 (test code: a yardstick for a miss, not an oracle) ---------------------------------

def kernel_act(z, act):
    """a = rcp(1 + exp2(c z)), tanh = 2a - 1, in float32; returns (a, act', act''/act'), the derivatives rebuilt from a."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(over='ignore'):
        s = (np.float32(1.0) / (np.float32(1.0) + np.exp2(np.float32(act_const(act)) * z))).astype(np.float32)
    if act == 'tanh':
        a = np.float32(2.0) * s - np.float32(1.0)
        return a, np.float32(1.0) - a * a, np.float32(-2.0) * a
    return s, s * (np.float32(1.0) - s), np.float32(1.0) - np.float32(2.0) * s


def exact_act(z, act):
    """The oracle's activation in the dtype of z, with the same derivative identities."""
    if act == 'tanh':
        a = np.tanh(z)
        return a, 1 - a * a, -2 * a
    with np.errstate(over='ignore'):
        a = 1 / (1 + np.exp(-z))
    return a, a * (1 - a), 1 - 2 * a


def _split(flat, d_in, widths):
    out, off = [], 0
    for i, o in og.layer_dims(d_in, widths):
        out.append((flat[off:off + i * o].reshape(i, o), flat[off + i * o:off + i * o + o]))
        off += i * o + o
    return out


def _fwd(params, X, G, actf, act):
    a, ad, cache = X, G, []
    for W, b in params[:-1]:
        z, zd = a @ W + b, ad @ W
        an, d1, d2r = actf(z, act)
        cache.append((a, ad, d1, d2r, zd, z))
        a, ad = an, d1 * zd
    W, b = params[-1]
    cache.append((a, ad))
    return (a @ W + b)[:, 0], (ad @ W)[:, 0], cache


def _bwd(params, cache, ubar, udbar):
    grads = [None] * len(params)
    a, ad = cache[-1]
    W = params[-1][0]
    grads[-1] = (a.T @ ubar[:, None] + ad.T @ udbar[:, None], ubar.sum(keepdims=True))
    abar, adbar = ubar[:, None] * W[:, 0][None, :], udbar[:, None] * W[:, 0][None, :]
    for l in range(len(params) - 2, -1, -1):
        ap, adp, d1, d2r, zd, _ = cache[l]
        zdbar = adbar * d1
        zbar = abar * d1 + adbar * (d1 * d2r) * zd
        grads[l] = (ap.T @ zbar + adp.T @ zdbar, zbar.sum(axis=0))
        abar, adbar = zbar @ params[l][0].T, zdbar @ params[l][0].T
    return grads


def formula_loss_and_grad(net, transform, act, dt=np.float32, actf=kernel_act):
    """The loss and its gradient by one forward tangent along gcoef and its reverse pass (the formulation of the kernels), every
    operation in `dt`, activation by `actf`.  Same contract as oracle()."""
    d_in, dim, widths, q, n_k, td = NETS[net]
    d = inputs(net, transform)[0]
    c = lambda a: np.asarray(a).astype(dt)
    params = _split(c(theta(net, transform)), d_in, widths)
    n = n_k * q
    G = np.zeros((n, d_in), dtype=dt)
    G[:, :dim] = c(d['gcoef'])
    u, ud, cache = _fwd(params, c(d['Input']), G, actf, act)
    dNt, w = c(d['dNt']).reshape(-1), [dt(x) for x in d['w']]
    int1 = ud - c(d['source']).reshape(-1) * c(d['N']).reshape(-1)
    if td:
        int1 = int1 - u * dNt
    R = int1.reshape(n_k, q).sum(axis=1)
    detJ = dt(d['detJ'])
    lossVec = detJ * R * R
    var = lossVec.sum()
    seed = np.repeat(dt(2.0) * w[2] * detJ * R, q)
    grads = _bwd(params, cache, -dNt * seed if td else np.zeros_like(seed), seed)
    ub, _, cb = _fwd(params, c(d['biInput']), np.zeros((NB, d_in), dtype=dt), actf, act)
    e = ub - c(d['biLabel']).reshape(-1)
    bv = dt(BIDIMVAL)
    bc = bv * np.mean(e[:BDOF] ** 2)
    coef = np.zeros(NB, dtype=dt)
    coef[:BDOF] = dt(2.0) * w[0] * bv / dt(BDOF)
    ic = dt(0.0)
    if td:
        ic = bv * np.mean(e[BDOF:] ** 2)
        coef[BDOF:] = dt(2.0) * w[1] * bv / dt(NB - BDOF)
    gb = _bwd(params, cb, coef * e, np.zeros(NB, dtype=dt))
    g = np.concatenate([np.concatenate([(a[0] + b_[0]).reshape(-1), (a[1] + b_[1]).reshape(-1)]) for a, b_ in zip(grads, gb)])
    res = dict(loss=float(w[0] * bc + w[1] * ic + w[2] * var), BCloss=float(bc), ICloss=float(ic), varLoss=float(var),
               lossVec=np.asarray(lossVec, dtype=np.float64))
    return res, np.asarray(g, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def kernel_formula(net, transform, act):
    return formula_loss_and_grad(net, transform, act)


def hidden_preacts(net, transform, act):
    """Per hidden layer, the fp32 pre-activations z [rows, width] and activations of the oracle's forward on the interior and
    the boundary / initial rows together."""
    d_in, dim, widths, q, n_k, td = NETS[net]
    d = inputs(net, transform)[0]
    a = torch.as_tensor(np.concatenate([d['Input'], d['biInput']]), dtype=torch.float32)
    out = []
    for W, b in og.unflatten(theta(net, transform), d_in, widths, torch.float32)[:-1]:
        z = a @ W + b
        a = og.ACTIVATION[act](z)
        out.append((z.numpy(), a.numpy()))
    return out


# -- point kernels ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def point_case(net, transform, act, n):
    """Points, coefficient fields, parameters and the fp64 references (u, grad u, residual) of a point-kernel case.  X holds
    fp32-representable values (at offset 100 the rounding of a double input would be the error measured)."""
    d_in, dim, widths = POINT_NETS[net]
    rng = np.random.default_rng(700 + 10 * list(POINT_NETS).index(net) + POINT_N.index(n))
    X32 = rng.uniform(-1.2, 1.2, (n, d_in)).astype(np.float32)
    diff = rng.uniform(0.05, 1, (n, 1)); vel = rng.standard_normal((n, dim))
    src = rng.standard_normal((n, 1)); ddx = rng.standard_normal((n, dim))
    if transform == 'offset100':
        X32 = (X32 + np.float32(SCALE['offset100'])).astype(np.float32)
    flat = transform_theta(base_theta(d_in, widths), d_in, widths, transform)
    X, f64 = X32.astype(np.float64), flat.astype(np.float64)
    uref, rref = og.residual(f64, d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, True, activation=act)
    Xt = torch.tensor(X, requires_grad=True)
    gref = og.model_grad(og.unflatten(f64, d_in, widths, torch.float64), Xt, dim, True, activation=act)[1].detach().numpy()
    return dict(X32=X32, X=X, diff=diff, vel=vel, src=src, ddx=ddx, flat=flat, uref=uref[:, 0], rref=rref[:, 0], gref=gref)


def point_formula(net, transform, act, n):
    """(u, grad u) at the case's points by the float32 restatement with the kernels' activation formula."""
    d_in, dim, widths = POINT_NETS[net]
    c = point_case(net, transform, act, n)
    params = _split(c['flat'], d_in, widths)
    g = np.zeros((n, dim), dtype=np.float32)
    for k in range(dim):
        G = np.zeros((n, d_in), dtype=np.float32)
        G[:, k] = 1.0
        u, g[:, k], _ = _fwd(params, c['X32'], G, kernel_act, act)
    return u, g


def point_grad32(net, transform, act, n):
    """grad u of the fp32 oracle (the per-column conditioning rule)."""
    d_in, dim, widths = POINT_NETS[net]
    c = point_case(net, transform, act, n)
    Xt = torch.tensor(c['X32'], requires_grad=True)
    return og.model_grad(og.unflatten(c['flat'], d_in, widths, torch.float32), Xt, dim, True, activation=act)[1].detach().numpy()
