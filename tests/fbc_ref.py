"""
fp64 restatement of flux boundary identification (vn_set_fluxbc_basis, vn_set_fluxbc_learn) with torch autograd on the CPU: the
boundary-flux term of tests/flux_ref.py evaluated at

    label = label0 + Gamma^T a[:Jl],    coef = coef0 + H^T a[Jl:]

with the amplitudes `a` a tensor with a gradient.  The flux mean F enters the loss as w0 F (it joins the BC component), so the
amplitude gradient is g_a = w0 dF/da, and S_j = sum_k |row k's contribution to g_a[j]| measures its conditioning:

    r_k = n_k . grad_x u_k + coef[k] u_k - label[k],    udbar[k] = 2 w0 biDimVal r_k / nF
    g_a[j] = - sum_k udbar[k] Gamma[j, k]   (j < Jl),    g_a[j] = + sum_k udbar[k] u_k H[j, k]   (j >= Jl)

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og


def evaluate(flat, d_in, widths, dim, X, normal, coef0, label0, S, Jl, amp, biDimVal, w0, activation='sigmoid', dtype=torch.float64):
    """(F, dF/dtheta [P], g_a [J], S_j [J]) at the amplitudes amp; S is [J, nF], the Jl flux-datum streams first."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    params = og.unflatten(np.asarray(flat), d_in, widths, dtype=dtype, requires_grad=True)
    Xt = t(X).clone().requires_grad_(True)
    u = og.model(params, Xt, activation)
    gx = torch.autograd.grad(u.sum(), Xt, create_graph=True)[0][:, :dim]
    ud = (gx * t(normal).reshape(-1, dim)).sum(dim=1)
    St = t(S)
    a = t(amp).clone().requires_grad_(True)
    label = t(np.reshape(label0, -1)) + a[:Jl] @ St[:Jl]
    coef = t(np.reshape(coef0, -1)) + a[Jl:] @ St[Jl:]
    r = ud + coef * u[:, 0] - label
    nF = r.shape[0]
    F = (biDimVal * r ** 2).mean()
    (w0 * F).backward()
    g_theta = og.flatten_grads(params).detach().numpy().astype(np.float64) / w0
    with torch.no_grad():
        udbar = 2.0 * w0 * biDimVal * r / nF
        wrow = torch.cat([(-udbar).expand(Jl, nF), (udbar * u[:, 0]).expand(St.shape[0] - Jl, nF)], dim=0)
        Ssum = (wrow * St).abs().sum(dim=1)
    return float(F.detach()), g_theta, a.grad.detach().numpy().astype(np.float64), Ssum.numpy().astype(np.float64)
