"""
fp64 restatement of the periodic boundary term (vn_set_periodic, `ADPDE(..., periodic=[(A, B)])`) with torch autograd on the
CPU: the MLP is built from the flat parameter vector in the header's layout (oracle/tf1_graph.unflatten), and the term is added
to what oracle/tf1_graph.loss_and_grad gives for the other terms.  Rows i and i + nP of X are the two images of one point and
carry the same direction d:

    r0   = u_i - u_{i+nP}
    r1   = d . grad_x u_i - d . grad_x u_{i+nP}     (grad_x: the dim space inputs)
    P    = mean_P[biDimVal (r0^2 + gamma r1^2)]
    BC   = mean_D[biDimVal (u - g/beta)^2] + P,     loss = w0 BC + w1 IC + w2 var

A problem without Dirichlet rows (bDof == 0) has mean_D = 0, as the engine defines it (include/varnet_hip.h); the oracle's
mean over no rows is NaN, so for that case the oracle is given one stand-in boundary row under a zero BC weight, which enters
neither its loss nor its gradient.

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og


def periodic_term(flat, d_in, widths, dim, X, dirs, gamma, biDimVal, activation='sigmoid', dtype=torch.float64):
    """(P, dP/dtheta, r0, r1): the periodic mean, its gradient (flat, numpy) and the per-pair jumps."""
    X = np.asarray(X)
    nP = X.shape[0] // 2
    assert X.shape[0] == 2 * nP
    params = og.unflatten(np.asarray(flat), d_in, widths, dtype=dtype, requires_grad=True)
    Xt = torch.as_tensor(X, dtype=dtype).clone().requires_grad_(True)
    u = og.model(params, Xt, activation)
    gx = torch.autograd.grad(u.sum(), Xt, create_graph=True)[0][:, :dim]
    d = torch.as_tensor(np.asarray(dirs), dtype=dtype).reshape(-1, dim)
    ud = (gx * d).sum(dim=1)
    r0 = u[:nP, 0] - u[nP:, 0]
    r1 = ud[:nP] - ud[nP:]
    P = (biDimVal * (r0 ** 2 + gamma * r1 ** 2)).mean()
    P.backward()
    return (float(P.detach()), og.flatten_grads(params).detach().numpy().astype(np.float64), r0.detach().numpy(),
            r1.detach().numpy())


def loss_and_grad(flat, d_in, widths, periodic, dtype=torch.float64, **kw):
    """og.loss_and_grad(flat, d_in, widths, dtype, **kw) with the periodic term added.  periodic = dict(X, dir, gamma) or None;
    biDimVal, w, dim and activation (default sigmoid) are those of kw."""
    w = np.asarray(kw['w'], dtype=float)
    if kw['bDof'] == 0:
        # no Dirichlet rows: mean_D = 0.  One stand-in row under w0 = 0 keeps the oracle's mean finite and out of everything.
        kw = dict(kw)
        bi, lab = np.asarray(kw['biInput']), np.asarray(kw['biLabel'])
        kw['biInput'] = np.vstack([np.zeros((1, d_in), dtype=bi.dtype), bi.reshape(-1, d_in)])
        kw['biLabel'] = np.vstack([np.zeros((1, 1), dtype=lab.dtype), lab.reshape(-1, 1)])
        kw['bDof'] = 1
        kw['w'] = np.array([0.0, w[1], w[2]])
        res, g = og.loss_and_grad(flat, d_in, widths, dtype, **kw)
        res = dict(res)
        res['BCloss'] = 0.0
    else:
        res, g = og.loss_and_grad(flat, d_in, widths, dtype, **kw)
    if periodic is None or len(periodic['X']) == 0:
        return res, g
    P, gP, _, _ = periodic_term(flat, d_in, widths, kw['dim'], periodic['X'], periodic['dir'], float(periodic['gamma']),
                                kw['biDimVal'], kw.get('activation', 'sigmoid'), dtype)
    res = dict(res)
    res['BCloss'] = res['BCloss'] + P
    res['loss'] = res['loss'] + w[0] * P
    return res, g + w[0] * gP
