"""
fp64 restatement of the weak-form loss WITH per-test-function weights (vn_set_tf_weights) and the causal time-slab mode
(vn_set_causal, `VarNet(causal=eps)`) with torch autograd on the CPU.  With l_k = detJ_k R_k^2 the loss field of the underlying
reference (tests/nldiff_ref.loss_fun, which is tests/nlflux_ref's, tests/reaction_ref's and the oracle's when the terms are
off, so the terms compose):

    var  = sum_k omega_k l_k            omega DETACHED: the gradient treats it as a constant
    loss = w0 BC + w1 IC + w2 var
    lossVec = l                         unweighted

    causal:  L_s = mean of l_k over the test functions of slab s (an empty slab: 0),  C_s = sum_{s' < s} L_s',
             omega_k = exp(-eps C_{slab[k]})          (`causal_weights`, fp64 numpy whatever the reference's precision)

With omega = 1, or eps = 0, every output equals the underlying reference bit for bit (tests/test_causal_host.py): for a scalar
detJ the weighted sum is formed as detJ * sum_k omega_k R_k^2, the underlying reference's own order of operations.

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og
from tests import nldiff_ref


def causal_weights(lossVec, slab, S, eps):
    """(omega_k [n_k], omega_s [S]) in fp64 numpy from a loss field, slab ids in [0, S) and eps."""
    lv = np.asarray(lossVec, dtype=np.float64).reshape(-1)
    slab = np.asarray(slab, dtype=np.int64).reshape(-1)
    assert lv.size == slab.size and slab.min() >= 0 and slab.max() < S
    cnt = np.bincount(slab, minlength=S)
    tot = np.bincount(slab, weights=lv, minlength=S)
    L = np.where(cnt > 0, tot / np.maximum(cnt, 1), 0.0)
    C = np.concatenate([[0.0], np.cumsum(L)[:-1]])
    om = np.exp(-float(eps) * C)
    return om[slab], om


def loss_and_grad(flat, d_in, widths, omega=None, causal=None, nldiff=None, nlflux=None, reaction=None, dtype=torch.float64,
                  **kw):
    """nldiff_ref.loss_and_grad(flat, d_in, widths, nldiff, nlflux, reaction, dtype, **kw) with weights.  omega: [n_k] static
    weights, or causal = (slab [n_k], S, eps): the weights of this evaluation's own loss field; neither: weights 1.
    The result also carries 'omega' [n_k] (fp64) and, in causal mode, 'omega_slab' [S]."""
    assert omega is None or causal is None
    rate, coef = (None, (0.0, 0.0, 0.0)) if reaction is None else reaction
    phi, fcoef = (None, (0.0, 0.0, 0.0)) if nlflux is None else nlflux
    psi, dcoef = (None, nldiff_ref.ONE) if nldiff is None else nldiff
    params = og.unflatten(flat, d_in, widths, dtype=dtype, requires_grad=True)
    tk = {}
    for k, v in kw.items():
        tk[k] = torch.as_tensor(v, dtype=dtype) if isinstance(v, np.ndarray) else v
    col = lambda a: None if a is None else torch.as_tensor(np.reshape(np.asarray(a), (-1, 1)), dtype=dtype)
    detJ, detJvec, w = tk['detJ'], tk['detJvec'], tk['w']
    if not detJvec:
        tk['detJ'] = 1.0                                             # lossVec of the call below is then R_k^2 itself
    out = nldiff_ref.loss_fun(params, rate=col(rate), coef=coef, phi=col(phi), fcoef=fcoef, psi=col(psi), dcoef=dcoef, **tk)
    r2 = out['lossVec']                                              # detJvec: detJ_k R_k^2; else R_k^2
    lossVec = r2 if detJvec else detJ * r2                           # :668
    n_k = r2.shape[0]
    om_slab = None
    if causal is not None:
        slab, S, eps = causal
        om, om_slab = causal_weights(lossVec.detach().numpy(), slab, S, eps)
    elif omega is not None:
        om = np.asarray(omega, dtype=np.float64).reshape(-1)
    else:
        om = np.ones(n_k)
    assert om.size == n_k
    om_t = torch.as_tensor(om.reshape(-1, 1), dtype=dtype)           # a constant of the graph
    if detJvec:
        var = (om_t * r2).sum()                                      # :663
    else:
        var = detJ * (om_t * r2).sum()                               # :664
    loss = w[0] * out['BCloss'] + w[1] * out['ICloss'] + w[2] * var  # :666
    loss.backward()
    g = og.flatten_grads(params).detach().numpy()
    res = dict(loss=float(loss.detach()), BCloss=float(out['BCloss'].detach()), ICloss=float(out['ICloss'].detach()),
               varLoss=float(var.detach()), lossVec=lossVec.detach().numpy(), omega=om)
    if om_slab is not None:
        res['omega_slab'] = om_slab
    return res, g
