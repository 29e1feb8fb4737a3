"""
fp64 restatement of the weak-form loss of tests/nldiff_ref.py with the NINE polynomial coefficients as torch tensors, so that
autograd also returns d loss / d coefficient (inverse mode: vn_set_coef_learn, `VarNet(learnCoef=...)`).  tests/nldiff_ref.py and
the helpers below it call float() on the coefficients, which cuts the graph; `loss_fun` here is nldiff_ref.loss_fun line by line
with tensors in their place.  Coefficient index: 0..2 = (c1, c2, c3) reaction, 3..5 = (f1, f2, f3) flux, 6..8 = (d0, d1, d2) D(u).

Besides the gradient g_m the reference returns, per component, the scale S_m = sum_r |row contribution|: the coefficient is
broadcast as a per-row tensor, and S_m is the sum of the absolute values of the gradient with respect to that tensor.  |g_m| / S_m
says how much cancellation the sum over rows carries, which is what an fp32 evaluation can lose.

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og

OFF = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0)           # the nine values of a PDE without any of the three terms


def nine(nldiff=None, nlflux=None, reaction=None):
    """The nine coefficients of (nldiff, nlflux, reaction) as tests/dedup_term_cases.terms_of returns them (None: term absent)."""
    c = list(OFF)
    pad = lambda v: ([float(x) for x in np.reshape(np.asarray(v, dtype=np.float64), -1)] + [0.0] * 3)[:3]
    if reaction is not None:
        c[0:3] = pad(reaction[1])
    if nlflux is not None:
        c[3:6] = pad(nlflux[1])
    if nldiff is not None:
        c[6:9] = pad(nldiff[1])
    return np.array(c, dtype=np.float64)


def loss_fun(params, coef, Input, gcoef, source, N, dNt, integW, intShape, detJ, detJvec, biInput, biLabel, bDof, biDimVal, w, dim,
             time_dependent=True, is_source=False, integWflag=False, activation='sigmoid', rate=None, phi=None, psi=None,
             has=(True, True, True)):
    """tests/nldiff_ref.loss_fun with coef [9] or [nT, 9] (per-row copies) a tensor.  has = (reaction, flux, D(u)) present:
    an absent term contributes nothing whatever its entries of coef say (the engine does not launch its kernels)."""
    dt = Input.dtype
    Inp = Input.detach().clone().requires_grad_(True)
    Val, grad, _, _ = og.model_grad(params, Inp, dim, time_dependent, activation=activation)
    if biInput is not None and biInput.shape[0] > 0:
        biVal = og.model(params, biInput, activation)
        biCs = biDimVal * (biVal - biLabel) ** 2
        bCs = biCs[:bDof, 0:1].mean()
        iCs = biCs[bDof:, 0:1].mean() if time_dependent else torch.zeros((), dtype=dt)
    else:
        bCs = torch.zeros((), dtype=dt)
        iCs = torch.zeros((), dtype=dt)
    c = (lambda i: coef[i]) if coef.ndim == 1 else (lambda i: coef[:, i:i + 1])
    A = (grad * gcoef).sum(dim=-1, keepdim=True)
    int1 = (c(6) + Val * (c(7) + Val * c(8))) * A if has[2] else A           # nldiff_ref.dfun: Horner
    if psi is not None:
        int1 = int1 - Val * psi
    if time_dependent:
        int1 = int1 - Val * dNt
    if has[0]:
        react = c(0) * Val + c(1) * Val ** 2 + c(2) * Val ** 3               # reaction_ref.poly
        if rate is not None:
            react = rate * react
    else:
        react = torch.zeros_like(Val)
    if is_source:
        int1 = int1 - (source + react) * N
    else:
        int1 = int1 - react * N
    if has[1] and phi is not None:
        int1 = int1 - (c(3) * Val + c(4) * Val ** 2 + c(5) * Val ** 3) * phi
    int1 = int1.reshape(intShape[0], intShape[1])
    if integWflag:
        int1 = integW * int1
    int1 = int1.sum(dim=-1, keepdim=True) ** 2
    int2 = (detJ * int1).sum() if detJvec else detJ * int1.sum()
    loss = w[0] * bCs + w[1] * iCs + w[2] * int2
    return dict(loss=loss, BCloss=bCs, ICloss=iCs, varLoss=int2, lossVec=detJ * int1)


def evaluate(flat, d_in, widths, coef, nldiff=None, nlflux=None, reaction=None, dtype=torch.float64, **kw):
    """(loss pieces, theta-gradient, coefficient gradient [9], scale S [9]) at coef [9].  nldiff = (psi or None, _), nlflux =
    (phi, _), reaction = (rate or None, _) name the streams and which terms are present (their coefficient entries are ignored:
    coef counts); **kw as for tests/nldiff_ref.loss_and_grad."""
    f = np.float64 if dtype == torch.float64 else np.float32
    tk = {k: (torch.as_tensor(v, dtype=dtype) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    col = lambda a: None if a is None else torch.as_tensor(np.reshape(np.asarray(a), (-1, 1)).astype(f), dtype=dtype)
    streams = dict(rate=col(reaction[0]) if reaction is not None else None, phi=col(nlflux[0]) if nlflux is not None else None,
                   psi=col(nldiff[0]) if nldiff is not None else None,
                   has=(reaction is not None, nlflux is not None, nldiff is not None))
    params = og.unflatten(np.asarray(flat).astype(f), d_in, widths, dtype=dtype, requires_grad=True)
    c = torch.tensor(np.asarray(coef, dtype=f), dtype=dtype, requires_grad=True)
    out = loss_fun(params, c, **streams, **tk)
    out['loss'].backward()
    g = og.flatten_grads(params).detach().numpy()
    gc = np.zeros(9) if c.grad is None else c.grad.detach().numpy().astype(np.float64)
    # the scale: the same loss with a per-row copy of every coefficient
    nT = tk['Input'].shape[0]
    params2 = og.unflatten(np.asarray(flat).astype(f), d_in, widths, dtype=dtype)
    crow = torch.tensor(np.tile(np.asarray(coef, dtype=f), (nT, 1)), dtype=dtype, requires_grad=True)
    loss_fun(params2, crow, **streams, **tk)['loss'].backward()
    S = np.zeros(9) if crow.grad is None else crow.grad.detach().abs().sum(dim=0).numpy().astype(np.float64)
    res = {k: (v.detach().numpy() if v.ndim else float(v.detach())) for k, v in out.items()}
    return res, g, gc, S
