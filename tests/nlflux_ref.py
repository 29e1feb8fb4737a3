"""
fp64 restatement of the weak-form loss WITH the polynomial flux term (vn_set_nlflux, `ADPDE(nlflux=...)`) with torch autograd on
the CPU.  The PDE is

    c_t = div(kappa grad c) - v . grad c - div(w(x,t) F(c)) + s + rate(x,t) p(c),      F(c) = f1 c + f2 c^2 + f3 c^3

The flux is conservative: it integrates by parts onto the test function, so with phi_r = sum_d w_d dN_r/dx_d per row `loss_fun`
below is tests/reaction_ref.loss_fun plus one line,

    reaction_ref:   int1 = sum_d u_{x_d} gcoef_d - u dNt - (s + rate p(u)) N
    here:           int1 = sum_d u_{x_d} gcoef_d - u dNt - (s + rate p(u)) N - F(u) phi

Everything after it (integW, R_k, detJ R_k^2, lossVec, the weights) is the oracle's.  With all flux coefficients zero the result
is reaction_ref's (and, without a reaction, the oracle's) bit for bit (tests/test_nlflux_host.py).  `residual` is
reaction_ref.residual - (F'(u) w . grad u + F(u) div w).

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og
from tests import reaction_ref
from tests.reaction_ref import poly


def dpoly(u, coef):
    """F'(u) = f1 + 2 f2 u + 3 f3 u^2 (coef zero-padded to three entries)."""
    c = [float(x) for x in np.reshape(np.asarray(coef, dtype=np.float64), -1)]
    c = c + [0.0] * (3 - len(c))
    return c[0] + 2.0 * c[1] * u + 3.0 * c[2] * u ** 2


def loss_fun(params, Input, gcoef, source, N, dNt, integW, intShape, detJ, detJvec,
             biInput, biLabel, bDof, biDimVal, w, dim, time_dependent=True,
             is_source=False, integWflag=False, activation='sigmoid', rate=None, coef=(0.0, 0.0, 0.0),
             phi=None, fcoef=(0.0, 0.0, 0.0)):
    """tests/reaction_ref.loss_fun with the flux term: phi [nT,1] tensor, fcoef (f1, f2, f3); rate / coef: the reaction."""
    dt = Input.dtype
    Inp = Input.detach().clone().requires_grad_(True)
    Val, grad, _, _ = og.model_grad(params, Inp, dim, time_dependent, activation=activation)
    if biInput is not None and biInput.shape[0] > 0:
        biVal = og.model(params, biInput, activation)
        biCs = biDimVal * (biVal - biLabel) ** 2                 # :643
        bCs = biCs[:bDof, 0:1].mean()                            # :644-645
        if time_dependent:
            iCs = biCs[bDof:, 0:1].mean()                        # :647-648
        else:
            iCs = torch.zeros((), dtype=dt)
    else:
        bCs = torch.zeros((), dtype=dt)
        iCs = torch.zeros((), dtype=dt)

    int1 = (grad * gcoef).sum(dim=-1, keepdim=True)              # :653-654
    if time_dependent:
        int1 = int1 - Val * dNt                                  # :655
    react = poly(Val, coef)                                      # p(u) at every row
    if rate is not None:
        react = rate * react
    if is_source:
        int1 = int1 - (source + react) * N                       # :657 with s -> s + rate p(u)
    else:
        int1 = int1 - react * N
    int1 = int1 - poly(Val, fcoef) * phi                         # the flux term, integrated by parts: - F(u) phi
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


def loss_and_grad(flat, d_in, widths, nlflux, reaction=None, dtype=torch.float64, **kw):
    """reaction_ref.loss_and_grad(flat, d_in, widths, reaction, dtype, **kw) with the flux term.  nlflux = (phi, fcoef): phi a
    numpy column [nT,1], fcoef up to three numbers; nlflux None: reaction_ref itself."""
    if nlflux is None:
        return reaction_ref.loss_and_grad(flat, d_in, widths, reaction, dtype, **kw)
    phi, fcoef = nlflux
    rate, coef = (None, (0.0, 0.0, 0.0)) if reaction is None else reaction
    params = og.unflatten(flat, d_in, widths, dtype=dtype, requires_grad=True)
    tk = {}
    for k, v in kw.items():
        tk[k] = torch.as_tensor(v, dtype=dtype) if isinstance(v, np.ndarray) else v
    if rate is not None:
        rate = torch.as_tensor(np.reshape(np.asarray(rate), (-1, 1)), dtype=dtype)
    phi = torch.as_tensor(np.reshape(np.asarray(phi), (-1, 1)), dtype=dtype)
    out = loss_fun(params, rate=rate, coef=coef, phi=phi, fcoef=fcoef, **tk)
    out['loss'].backward()
    g = og.flatten_grads(params).detach().numpy()
    res = {k: (v.detach().numpy() if v.ndim else float(v.detach())) for k, v in out.items()}
    return res, g


def residual(flat, d_in, widths, dtype, Input, diff, vel, source, diff_dx, dim, nlflux, reaction=None, time_dependent=True,
             activation='sigmoid'):
    """reaction_ref.residual - (F'(u) w . grad u + F(u) div w): (model value [n,1], residual [n,1]) as numpy.
    nlflux = (w [n,dim] or `dim` numbers, fcoef, div_w [n,1] or None); grad u from oracle/tf1_graph.model_grad."""
    val, res = reaction_ref.residual(flat, d_in, widths, dtype, Input, diff, vel, source, diff_dx, dim, reaction, time_dependent,
                                     activation)
    if nlflux is None:
        return val, res
    w, fcoef, div_w = nlflux
    params = og.unflatten(flat, d_in, widths, dtype=dtype)
    Inp = torch.as_tensor(Input, dtype=dtype).clone().requires_grad_(True)
    _, grad, _, _ = og.model_grad(params, Inp, dim, time_dependent, activation=activation)
    w = np.reshape(np.asarray(w, dtype=val.dtype), (-1, dim))
    w_grad_u = (w * grad.detach().numpy()).sum(axis=-1, keepdims=True)
    out = res - dpoly(val, fcoef) * w_grad_u
    if div_w is not None:
        out = out - poly(val, fcoef) * np.reshape(np.asarray(div_w, dtype=val.dtype), (-1, 1))
    return val, out
