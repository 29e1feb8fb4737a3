"""
fp64 restatement of the weak-form loss WITH a hard-constraint ansatz (vn_set_ansatz, vn_set_ansatz_points, vn_set_ansatz_rows)
with torch autograd on the CPU.  The solution is u = A + B n with n the network output.  Every row set carries four streams:
A_r, B_r and the derivatives a_r = grad_x A . G_r, b_r = grad_x B . G_r along the row's own direction G_r (gcoef on the interior
rows, the normal of a flux row, the direction of a pair or of an observed point); with n_r and nd_r = grad_x n . G_r the network's
value and tangent

    u_r = A_r + B_r n_r,      ud_r = a_r + b_r n_r + B_r nd_r                                   (`fold`)

`loss_fun` is tests/nldiff_ref.loss_fun with Val <- u and (grad * gcoef).sum <- ud on the interior rows and biVal <- u on the BC/IC
rows; `flux_term`, `periodic_term`, `obs_term` are those of tests/flux_ref.py, tests/periodic_ref.py, tests/obs_ref.py with the
same substitution.  Everything after it is theirs.  With A = 0, B = 1, a = b = 0 each returns its model's result bit for bit
(tests/test_ansatz_host.py), which also pins it against direct autograd of a composite A(x,t) + B(x,t) net(x,t) and against
central differences of its own loss.

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og
from tests.nldiff_ref import ONE, dfun
from tests.reaction_ref import poly

KEYS = ('A', 'B', 'a', 'b')


def streams(z, dtype):
    """dict(A, B, a, b) of numpy columns (missing or None: zero; B required) -> dict of [rows] tensors."""
    B = torch.as_tensor(np.reshape(np.asarray(z['B']), -1), dtype=dtype)
    out = {'B': B}
    for k in ('A', 'a', 'b'):
        v = z.get(k)
        out[k] = torch.zeros_like(B) if v is None else torch.as_tensor(np.reshape(np.asarray(v), -1), dtype=dtype)
    return out


def fold(z, n, nd=None):
    """(u, ud) of the rows from the network's (n, nd), all [rows]; nd None: values only (ud None)."""
    u = z['A'] + z['B'] * n
    if nd is None:
        return u, None
    return u, z['a'] + z['b'] * n + z['B'] * nd


def loss_fun(params, Input, gcoef, source, N, dNt, integW, intShape, detJ, detJvec, biInput, biLabel, bDof, biDimVal, w, dim,
             time_dependent=True, is_source=False, integWflag=False, activation='sigmoid', rate=None, coef=(0.0, 0.0, 0.0),
             phi=None, fcoef=(0.0, 0.0, 0.0), psi=None, dcoef=ONE, ansatz=None, ansatz_bic=None):
    """tests/nldiff_ref.loss_fun with the ansatz on the interior rows (ansatz: tensors of `streams`) and on the BC/IC rows
    (ansatz_bic; a, b unused: the rows have no direction)."""
    dt = Input.dtype
    Inp = Input.detach().clone().requires_grad_(True)
    Val, grad, _, _ = og.model_grad(params, Inp, dim, time_dependent, activation=activation)
    gd = (grad * gcoef).sum(dim=-1, keepdim=True)
    if ansatz is not None:
        u, ud = fold(ansatz, Val[:, 0], gd[:, 0])
        Val, gd = u.reshape(-1, 1), ud.reshape(-1, 1)
    if biInput is not None and biInput.shape[0] > 0:
        biVal = og.model(params, biInput, activation)
        if ansatz_bic is not None:
            biVal = fold(ansatz_bic, biVal[:, 0])[0].reshape(-1, 1)
        biCs = biDimVal * (biVal - biLabel) ** 2                 # :643
        bCs = biCs[:bDof, 0:1].mean()                            # :644-645
        if time_dependent:
            iCs = biCs[bDof:, 0:1].mean()                        # :647-648
        else:
            iCs = torch.zeros((), dtype=dt)
    else:
        bCs = torch.zeros((), dtype=dt)
        iCs = torch.zeros((), dtype=dt)

    int1 = dfun(Val, dcoef) * gd                                 # :653-654 with kappa -> kappa D(u)
    if psi is not None:
        int1 = int1 - Val * psi
    if time_dependent:
        int1 = int1 - Val * dNt                                  # :655
    react = poly(Val, coef)
    if rate is not None:
        react = rate * react
    if is_source:
        int1 = int1 - (source + react) * N                       # :657 with s -> s + rate p(u)
    else:
        int1 = int1 - react * N
    if phi is not None:
        int1 = int1 - poly(Val, fcoef) * phi
    int1 = int1.reshape(intShape[0], intShape[1])                # :659
    if integWflag:
        int1 = integW * int1                                     # :660
    int1 = int1.sum(dim=-1, keepdim=True) ** 2                   # :661
    if detJvec:
        int2 = (detJ * int1).sum()                               # :663
    else:
        int2 = detJ * int1.sum()                                 # :664
    loss = w[0] * bCs + w[1] * iCs + w[2] * int2                 # :666
    lossVec = detJ * int1                                        # :668
    return dict(loss=loss, BCloss=bCs, ICloss=iCs, varLoss=int2, lossVec=lossVec)


def _rows(params, X, dirs, dim, activation, dtype, z):
    """(u, ud) of the rows X with directions dirs (None: ud None) under the ansatz z (None: the bare network)."""
    Xt = torch.as_tensor(np.asarray(X), dtype=dtype).clone().requires_grad_(True)
    n = og.model(params, Xt, activation)[:, 0]
    nd = None
    if dirs is not None:
        gx = torch.autograd.grad(n.sum(), Xt, create_graph=True)[0][:, :dim]
        nd = (gx * torch.as_tensor(np.asarray(dirs), dtype=dtype).reshape(-1, dim)).sum(dim=1)
    if z is None:
        return n, nd
    return fold(streams(z, dtype), n, nd)


def flux_term(params, dim, X, normal, coef, label, biDimVal, activation, dtype, z=None):
    """F = mean[biDimVal (n . grad_x u + coef u - label)^2] of tests/flux_ref.flux_term, as a tensor."""
    u, ud = _rows(params, X, normal, dim, activation, dtype, z)
    c = torch.as_tensor(np.reshape(coef, -1), dtype=dtype)
    lab = torch.as_tensor(np.reshape(label, -1), dtype=dtype)
    r = ud + c * u - lab
    return (biDimVal * r ** 2).mean()


def periodic_term(params, dim, X, dirs, gamma, biDimVal, activation, dtype, z=None):
    """P = mean[biDimVal (r0^2 + gamma r1^2)] of tests/periodic_ref.periodic_term, as a tensor."""
    nP = np.asarray(X).shape[0] // 2
    u, ud = _rows(params, X, dirs, dim, activation, dtype, z)
    r0 = u[:nP] - u[nP:]
    r1 = ud[:nP] - ud[nP:]
    return (biDimVal * (r0 ** 2 + gamma * r1 ** 2)).mean()


def obs_term(params, dim, X, value, q, dirs, rowptr, wgt, activation, dtype, z=None):
    """O = mean[wgt r^2] of tests/obs_ref.obs_term, as a tensor."""
    value = np.asarray(value).reshape(-1)
    nO = value.shape[0]
    rowptr = np.arange(nO + 1) if rowptr is None else np.asarray(rowptr, dtype=np.int64)
    u, ud = _rows(params, X, dirs, dim, activation, dtype, z)
    t = u if q is None else torch.as_tensor(np.asarray(q), dtype=dtype).reshape(-1) * u
    if ud is not None:
        t = t + ud
    seg = torch.as_tensor(np.repeat(np.arange(nO), np.diff(rowptr)))
    ell = torch.zeros(nO, dtype=dtype).index_add(0, seg, t)
    r = ell - torch.as_tensor(value, dtype=dtype)
    w = torch.ones(nO, dtype=dtype) if wgt is None else torch.as_tensor(np.asarray(wgt), dtype=dtype).reshape(-1)
    return (w * r ** 2).mean()


def loss_and_grad(flat, d_in, widths, ansatz, nldiff=None, nlflux=None, reaction=None, flux=None, periodic=None, obs=None,
                  dtype=torch.float64, **kw):
    """The loss of tests/nldiff_ref.loss_and_grad(flat, d_in, widths, nldiff, nlflux, reaction, dtype, **kw) plus the edge sets of
    tests/flux_ref.py (flux = dict(X, normal, coef, label)), tests/periodic_ref.py (periodic = dict(X, dir, gamma)) and
    tests/obs_ref.py (obs = dict(X, value, lam[, q, dir, rowptr, wgt])), all under the ansatz.
    ansatz = dict(int=z, bic=z, flux=z, periodic=z, obs=z), z = dict(A, B, a, b) of numpy arrays (a missing set: the bare
    network on its rows); ansatz None: none anywhere.  (result dict, flat gradient) as numpy; 'obs' carries the misfit."""
    ansatz = ansatz or {}
    psi, dcoef = (None, ONE) if nldiff is None else nldiff
    rate, coef = (None, (0.0, 0.0, 0.0)) if reaction is None else reaction
    phi, fcoef = (None, (0.0, 0.0, 0.0)) if nlflux is None else nlflux
    params = og.unflatten(np.asarray(flat), d_in, widths, dtype=dtype, requires_grad=True)
    tk = {}
    for k, v in kw.items():
        tk[k] = torch.as_tensor(v, dtype=dtype) if isinstance(v, np.ndarray) else v
    col = lambda a: None if a is None else torch.as_tensor(np.reshape(np.asarray(a), (-1, 1)), dtype=dtype)
    zt = lambda name: None if ansatz.get(name) is None else streams(ansatz[name], dtype)
    out = loss_fun(params, rate=col(rate), coef=coef, phi=col(phi), fcoef=fcoef, psi=col(psi), dcoef=dcoef,
                   ansatz=zt('int'), ansatz_bic=zt('bic'), **tk)
    w = np.asarray(kw['w'], dtype=float)
    act = kw.get('activation', 'sigmoid')
    if flux is not None:
        F = flux_term(params, kw['dim'], flux['X'], flux['normal'], flux['coef'], flux['label'], kw['biDimVal'], act, dtype,
                      ansatz.get('flux'))
        out['BCloss'] = out['BCloss'] + F
        out['loss'] = out['loss'] + w[0] * F
    if periodic is not None:
        Pm = periodic_term(params, kw['dim'], periodic['X'], periodic['dir'], float(periodic['gamma']), kw['biDimVal'], act, dtype,
                           ansatz.get('periodic'))
        out['BCloss'] = out['BCloss'] + Pm
        out['loss'] = out['loss'] + w[0] * Pm
    if obs is not None:
        O = obs_term(params, kw['dim'], obs['X'], obs['value'], obs.get('q'), obs.get('dir'), obs.get('rowptr'), obs.get('wgt'), act,
                     dtype, ansatz.get('obs'))
        out['obs'] = O
        out['loss'] = out['loss'] + float(obs['lam']) * O
    out['loss'].backward()
    g = og.flatten_grads(params).detach().numpy()
    res = {k: (v.detach().numpy() if v.ndim else float(v.detach())) for k, v in out.items()}
    return res, g
