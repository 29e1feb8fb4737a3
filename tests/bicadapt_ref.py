"""
NumPy restatement of the weights on the Dirichlet and initial rows (vn_set_bic_weights, vn_set_bic_adapt,
`VarNet(bicWeights=..., bicAdapt=...)`), in fp64.  The rows of biInput fall into two parts, bc = rows [0, bDof) and
ic = rows [bDof, nB) (absent on a steady problem or when nB == bDof).  With e_i = u_i - label_i and omega_i >= 0 a constant of
the gradient:

    BC = biDimVal (1 / bDof) sum_{i < bDof} omega_i e_i^2,        IC likewise over its part,
    d loss / d u_i = 2 w_s biDimVal omega_i e_i / n_s             (w_0, n_0 = bDof for bc; w_1, n_1 = nB - bDof for ic)

`loss_and_grad` is oracle/tangent_ref.loss_and_grad with its BC/IC block extended by omega_i and nothing else changed (the
oracle's own forward and reverse passes are called, not copied); with omega = 1 it gives the oracle's numbers exactly.  It also
returns the unweighted loss field l_i = e_i^2 per part, which is what the update rules read.

The rules and the normalisation per part are those of tests/adapt_ref.py (`update`, `weights`, `step`), applied to a part's
own field, state and counter: `part_step` below is that function under the part's name.

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np

from oracle import tangent_ref as tr
from tests import adapt_ref

PARTS = ('bc', 'ic')


def part_rows(nB, bDof, time_dependent=True):
    """(rows of bc, rows of ic) as the engine counts them."""
    return int(bDof), (int(nB) - int(bDof)) if time_dependent else 0


def split(v, bDof, time_dependent=True):
    """A per-row array -> (bc part, ic part)."""
    v = np.asarray(v).reshape(-1)
    return v[:bDof], (v[bDof:] if time_dependent else v[:0])


def bic_block(params, d_in, biInput, biLabel, bDof, biDimVal, w, time_dependent, omega, dt):
    """The BC/IC block of oracle/tangent_ref.loss_and_grad with omega_i: (BC, IC, per-layer gradients of w0 BC + w1 IC or None
    without rows, (l_i of bc, l_i of ic))."""
    nB = 0 if biInput is None else biInput.shape[0]
    bc = ic = dt.type(0.0)
    field = (np.zeros(0, dtype=dt), np.zeros(0, dtype=dt))
    if not nB:
        return bc, ic, None, field
    om = np.ones(nB, dtype=dt) if omega is None else np.asarray(omega, dtype=dt).reshape(-1)
    assert om.size == nB
    ub, _, cb = tr.forward_tangent(params, biInput.astype(dt), np.zeros((nB, d_in), dtype=dt))
    e = ub - biLabel.reshape(-1)
    bc = biDimVal * np.mean(om[:bDof] * e[:bDof] ** 2)
    coef = np.empty(nB, dtype=dt)
    coef[:bDof] = 2.0 * w[0] * biDimVal / bDof
    if time_dependent and nB > bDof:
        ic = biDimVal * np.mean(om[bDof:] * e[bDof:] ** 2)
        coef[bDof:] = 2.0 * w[1] * biDimVal / (nB - bDof)
    else:
        coef[bDof:] = 0.0
    gb = tr.backward(params, cb, coef * om * e, np.zeros(nB, dtype=dt))
    return bc, ic, gb, split(e * e, bDof, time_dependent)


def bic_delta(flat, d_in, widths, biInput, biLabel, bDof, biDimVal, w, time_dependent, omega):
    """What the weights add to an UNWEIGHTED reference of any problem on these rows (the loss is a sum of terms, so the rest of
    the problem -- polynomial terms, flux rows, observations -- cancels): dict(BCloss, ICloss, loss) and the flat gradient, each
    the weighted block minus the unweighted one; 'field' as in loss_and_grad."""
    dt = flat.dtype
    params = tr.split_params(flat, d_in, widths)
    flatg = lambda gb: np.concatenate([np.concatenate([gW.reshape(-1), gb_.reshape(-1)]) for gW, gb_ in gb])
    bc1, ic1, g1, field = bic_block(params, d_in, biInput, biLabel, bDof, biDimVal, w, time_dependent, omega, dt)
    bc0, ic0, g0, _ = bic_block(params, d_in, biInput, biLabel, bDof, biDimVal, w, time_dependent, None, dt)
    return dict(BCloss=bc1 - bc0, ICloss=ic1 - ic0, loss=w[0] * (bc1 - bc0) + w[1] * (ic1 - ic0), field=field), flatg(g1) - flatg(g0)


def loss_and_grad(flat, d_in, widths, dim, Input, gcoef, source, N, dNt, integW, n_k, integNum, detJ, biInput, biLabel, bDof,
                  biDimVal, w, time_dependent=True, omega=None):
    """oracle/tangent_ref.loss_and_grad with per-row weights omega [nB] (None: 1) on the BC/IC rows.  Returns (dict, flat
    gradient); the dict carries, beside the oracle's entries, 'field': (l_i of bc, l_i of ic), unweighted."""
    dt = flat.dtype
    params = tr.split_params(flat, d_in, widths)
    n = Input.shape[0]
    G = np.zeros((n, d_in), dtype=dt)
    G[:, :dim] = gcoef
    u, ud, cache = tr.forward_tangent(params, Input.astype(dt), G)
    int1 = ud.copy()
    if time_dependent:
        int1 -= u * dNt.reshape(-1)
    if source is not None:
        int1 -= source.reshape(-1) * N.reshape(-1)
    wq = np.ones(integNum, dtype=dt) if integW is None else integW.reshape(-1).astype(dt)
    int1 = int1.reshape(n_k, integNum) * wq[None, :]
    R = int1.sum(axis=1)
    detJk = np.broadcast_to(np.asarray(detJ, dtype=dt).reshape(-1), (n_k,)) if np.size(detJ) > 1 \
        else np.full(n_k, detJ, dtype=dt)
    lossVec = detJk * R * R
    varLoss = lossVec.sum()
    seed = (2.0 * w[2] * detJk * R)[:, None] * wq[None, :]
    seed = seed.reshape(-1)
    ubar = -dNt.reshape(-1) * seed if time_dependent else np.zeros_like(seed)
    grads = tr.backward(params, cache, ubar, seed)

    bc, ic, gb, field = bic_block(params, d_in, biInput, biLabel, bDof, biDimVal, w, time_dependent, omega, dt)
    if gb is not None:
        grads = [(a[0] + b_[0], a[1] + b_[1]) for a, b_ in zip(grads, gb)]
    loss = w[0] * bc + w[1] * ic + w[2] * varLoss
    g = np.concatenate([np.concatenate([gW.reshape(-1), gb_.reshape(-1)]) for gW, gb_ in grads])
    return dict(loss=loss, BCloss=bc, ICloss=ic, varLoss=varLoss, lossVec=lossVec, field=field), g


def static_weights(omega, bDof, normalize, time_dependent=True):
    """The weights in use of a static registration: omega as given, divided per part by its mean when normalize (an all-zero
    part: Z = 1, omega = 0).  fp64."""
    spec = dict(power=1, normalize=bool(normalize))
    parts = split(np.asarray(omega, dtype=np.float64), bDof, time_dependent)
    return np.concatenate([adapt_ref.weights(p, spec)[0] if p.size else p for p in parts])


def part_step(lam, slots, tau, field, spec, dtype=np.float64):
    """One committed update of a part from its own unweighted loss field: tests/adapt_ref.step with l_i in place of l_k and the
    part's rows in place of the test functions."""
    return adapt_ref.step(lam, slots, tau, field, spec, dtype)
