"""
fp64 restatement of the observation term (vn_set_observations, `VarNet(..., observations=...)`) with torch autograd on the CPU:
the MLP is built from the flat parameter vector in the header's layout (oracle/tf1_graph.unflatten), and the term is added to what
tests/periodic_ref.loss_and_grad (oracle/tf1_graph.loss_and_grad plus the bDof == 0 convention and, if given, periodic pairs) gives
for the other terms.  Observation i owns the points rowptr[i] .. rowptr[i+1]-1 of X (rowptr None: the point i):

    l_i  = sum_j [ q_j u(x_j) + dir_j . grad_x u(x_j) ]     (grad_x: the dim space inputs; q None: 1; dir None: no such part)
    r_i  = l_i - value_i
    O    = mean_i[ wgt_i r_i^2 ]                            (wgt None: 1)
    loss = w0 BC + w1 IC + w2 var + lambda O

BC, IC, var and lossVec are untouched.

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og
from tests import periodic_ref


def obs_term(flat, d_in, widths, dim, X, value, q=None, dirs=None, rowptr=None, wgt=None, activation='sigmoid',
             dtype=torch.float64):
    """(O, dO/dtheta, r): the unweighted misfit, its gradient (flat, numpy) and the per-observation residuals."""
    X = np.asarray(X)
    n = X.shape[0]
    value = np.asarray(value).reshape(-1)
    nO = value.shape[0]
    rowptr = np.arange(nO + 1) if rowptr is None else np.asarray(rowptr, dtype=np.int64)
    assert rowptr[0] == 0 and rowptr[-1] == n and np.all(np.diff(rowptr) > 0)
    params = og.unflatten(np.asarray(flat), d_in, widths, dtype=dtype, requires_grad=True)
    Xt = torch.as_tensor(X, dtype=dtype).clone().requires_grad_(True)
    u = og.model(params, Xt, activation)[:, 0]
    t = u if q is None else torch.as_tensor(np.asarray(q), dtype=dtype).reshape(-1) * u
    if dirs is not None:
        gx = torch.autograd.grad(u.sum(), Xt, create_graph=True)[0][:, :dim]
        t = t + (gx * torch.as_tensor(np.asarray(dirs), dtype=dtype).reshape(-1, dim)).sum(dim=1)
    seg = torch.as_tensor(np.repeat(np.arange(nO), np.diff(rowptr)))
    ell = torch.zeros(nO, dtype=dtype).index_add(0, seg, t)
    r = ell - torch.as_tensor(value, dtype=dtype)
    w = torch.ones(nO, dtype=dtype) if wgt is None else torch.as_tensor(np.asarray(wgt), dtype=dtype).reshape(-1)
    O = (w * r ** 2).mean()
    O.backward()
    return float(O.detach()), og.flatten_grads(params).detach().numpy().astype(np.float64), r.detach().numpy()


def loss_and_grad(flat, d_in, widths, obs, periodic=None, dtype=torch.float64, **kw):
    """periodic_ref.loss_and_grad(flat, d_in, widths, periodic, dtype, **kw) with the observation term added.
    obs = dict(X, value, lam[, q, dir, rowptr, wgt]) or None; dim and activation (default sigmoid) are those of kw.  The result
    carries the unweighted misfit under 'obs'."""
    res, g = periodic_ref.loss_and_grad(flat, d_in, widths, periodic, dtype=dtype, **kw)
    if obs is None:
        return res, g
    O, gO, _ = obs_term(flat, d_in, widths, kw['dim'], obs['X'], obs['value'], obs.get('q'), obs.get('dir'), obs.get('rowptr'),
                        obs.get('wgt'), kw.get('activation', 'sigmoid'), dtype)
    lam = float(obs['lam'])
    res = dict(res)
    res['obs'] = O
    res['loss'] = res['loss'] + lam * O
    return res, g + lam * gO
