"""
fp64 restatement of the weak-form loss WITH the polynomial reaction term (vn_set_reaction, `ADPDE(reaction=...)`) with torch
autograd on the CPU.  The PDE is

    c_t = div(kappa grad c) - v . grad c + s + rate(x,t) p(c),      p(c) = c1 c + c2 c^2 + c3 c^3

with the reaction on the source side.  The loss is rebuilt from oracle/tf1_graph.unflatten / model / model_grad; `loss_fun`
below restates oracle/tf1_graph.loss_fun (TFModel.py:622-668) line by line, and the only line that differs is the row integrand:

    oracle:   int1 = sum_d u_{x_d} gcoef_d - u dNt - s N
    here:     int1 = sum_d u_{x_d} gcoef_d - u dNt - (s + rate p(u)) N

Everything after it (integW, R_k, detJ R_k^2, lossVec, the weights) is the oracle's.  With all coefficients zero the result is
the oracle's bit for bit (tests/test_reaction_host.py).  `residual` is oracle/tf1_graph.residual + rate p(u).

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og


def poly(u, coef):
    """p(u) = c1 u + c2 u^2 + c3 u^3 (coef zero-padded to three entries)."""
    c = [float(x) for x in np.reshape(np.asarray(coef, dtype=np.float64), -1)]
    c = c + [0.0] * (3 - len(c))
    return c[0] * u + c[1] * u ** 2 + c[2] * u ** 3


def loss_fun(params, Input, gcoef, source, N, dNt, integW, intShape, detJ, detJvec,
             biInput, biLabel, bDof, biDimVal, w, dim, time_dependent=True,
             is_source=False, integWflag=False, activation='sigmoid', rate=None, coef=(0.0, 0.0, 0.0)):
    """oracle/tf1_graph.loss_fun with the reaction term: rate [nT,1] tensor or None (rate = 1), coef (c1, c2, c3)."""
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


def loss_and_grad(flat, d_in, widths, reaction, dtype=torch.float64, **kw):
    """og.loss_and_grad(flat, d_in, widths, dtype, **kw) with the reaction term.  reaction = (rate, coef): rate a numpy column
    [nT,1] or None (rate = 1), coef up to three numbers; reaction None: the oracle itself."""
    if reaction is None:
        return og.loss_and_grad(flat, d_in, widths, dtype, **kw)
    rate, coef = reaction
    params = og.unflatten(flat, d_in, widths, dtype=dtype, requires_grad=True)
    tk = {}
    for k, v in kw.items():
        tk[k] = torch.as_tensor(v, dtype=dtype) if isinstance(v, np.ndarray) else v
    if rate is not None:
        rate = torch.as_tensor(np.reshape(np.asarray(rate), (-1, 1)), dtype=dtype)
    out = loss_fun(params, rate=rate, coef=coef, **tk)
    out['loss'].backward()
    g = og.flatten_grads(params).detach().numpy()
    res = {k: (v.detach().numpy() if v.ndim else float(v.detach())) for k, v in out.items()}
    return res, g


def residual(flat, d_in, widths, dtype, Input, diff, vel, source, diff_dx, dim, reaction, time_dependent=True,
             activation='sigmoid'):
    """oracle/tf1_graph.residual + rate p(u): (model value [n,1], residual [n,1]) as numpy."""
    val, res = og.residual(flat, d_in, widths, dtype, Input, diff, vel, source, diff_dx, dim, time_dependent, activation)
    if reaction is None:
        return val, res
    rate, coef = reaction
    term = poly(val, coef)
    if rate is not None:
        term = np.reshape(np.asarray(rate, dtype=val.dtype), (-1, 1)) * term
    return val, res + term
