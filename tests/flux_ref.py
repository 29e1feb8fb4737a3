"""
fp64 restatement of the boundary-flux term (vn_set_flux_bc, `VarNet(fluxBC=True)`) with torch autograd on the CPU: the MLP is
built from the flat parameter vector in the header's layout (oracle/tf1_graph.unflatten), and the term is added to what
oracle/tf1_graph.loss_and_grad gives for the other terms:

    r    = n . grad_x u + coef u - label            (grad_x: the dim space inputs)
    F    = mean_F[biDimVal r^2]
    BC   = mean_D[biDimVal (u - g/beta)^2] + F,     loss = w0 BC + w1 IC + w2 var

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og


def flux_term(flat, d_in, widths, dim, X, normal, coef, label, biDimVal, activation='sigmoid', dtype=torch.float64):
    """(F, dF/dtheta, r): the flux mean, its gradient (flat, numpy) and the per-row residual."""
    params = og.unflatten(np.asarray(flat), d_in, widths, dtype=dtype, requires_grad=True)
    Xt = torch.as_tensor(np.asarray(X), dtype=dtype).clone().requires_grad_(True)
    u = og.model(params, Xt, activation)
    gx = torch.autograd.grad(u.sum(), Xt, create_graph=True)[0][:, :dim]
    n = torch.as_tensor(np.asarray(normal), dtype=dtype).reshape(-1, dim)
    c = torch.as_tensor(np.reshape(coef, -1), dtype=dtype)
    lab = torch.as_tensor(np.reshape(label, -1), dtype=dtype)
    r = (gx * n).sum(dim=1) + c * u[:, 0] - lab
    F = (biDimVal * r ** 2).mean()
    F.backward()
    return float(F.detach()), og.flatten_grads(params).detach().numpy().astype(np.float64), r.detach().numpy()


def loss_and_grad(flat, d_in, widths, flux, dtype=torch.float64, **kw):
    """og.loss_and_grad(flat, d_in, widths, dtype, **kw) with the flux term added.  flux = dict(X, normal, coef, label) or None;
    biDimVal, w, dim and activation (default sigmoid) are those of kw."""
    res, g = og.loss_and_grad(flat, d_in, widths, dtype, **kw)
    if flux is None or len(flux['X']) == 0:
        return res, g
    w = np.asarray(kw['w'], dtype=float)
    F, gF, _ = flux_term(flat, d_in, widths, kw['dim'], flux['X'], flux['normal'], flux['coef'], flux['label'], kw['biDimVal'],
                         kw.get('activation', 'sigmoid'), dtype)
    res = dict(res)
    res['BCloss'] = res['BCloss'] + F
    res['loss'] = res['loss'] + w[0] * F
    return res, g + w[0] * gF
