"""
fp64 restatement of the weak-form loss WITH a solution-dependent diffusivity (vn_set_nldiff, `ADPDE(nldiff=[d0, d1, d2])`) with
torch autograd on the CPU.  The PDE is

    c_t = div(kappa D(c) grad c) - v . grad c - div(w F(c)) + s + rate p(c),      D(c) = d0 + d1 c + d2 c^2

On a batch with the term gcoef = kappa dN/dx ALONE and the advection is integrated by parts onto the test function: with
psi_r = sum_d v_d dN_r/dx_d + N_r div v per row `loss_fun` below is tests/nlflux_ref.loss_fun with its first line changed,

    nlflux_ref:   int1 =        sum_d u_{x_d} gcoef_d                     - u dNt - (s + rate p(u)) N - F(u) phi
    here:         int1 = D(u) * sum_d u_{x_d} gcoef_d   -   u psi         - u dNt - (s + rate p(u)) N - F(u) phi

Everything after it (integW, R_k, detJ R_k^2, lossVec, the weights) is the oracle's.  With D = (1, 0, 0) and psi = None the result
is nlflux_ref's bit for bit (tests/test_nldiff_host.py).  `residual` is the strong residual with div(kappa D(u) grad u) =
kappa D(u) Lap u + D(u) grad kappa . grad u + kappa D'(u) |grad u|^2; its advection term stays v . grad u.

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og
from tests import nlflux_ref
from tests.reaction_ref import poly

ONE = (1.0, 0.0, 0.0)


def _c3(coef):
    c = [float(x) for x in np.reshape(np.asarray(coef, dtype=np.float64), -1)]
    return c + [0.0] * (3 - len(c))


def dfun(u, coef):
    """D(u) = d0 + d1 u + d2 u^2 in Horner form (coef zero-padded to three entries)."""
    c = _c3(coef)
    return c[0] + u * (c[1] + u * c[2])


def ddfun(u, coef):
    """D'(u) = d1 + 2 d2 u."""
    c = _c3(coef)
    return c[1] + 2.0 * c[2] * u


def loss_fun(params, Input, gcoef, source, N, dNt, integW, intShape, detJ, detJvec,
             biInput, biLabel, bDof, biDimVal, w, dim, time_dependent=True,
             is_source=False, integWflag=False, activation='sigmoid', rate=None, coef=(0.0, 0.0, 0.0),
             phi=None, fcoef=(0.0, 0.0, 0.0), psi=None, dcoef=ONE):
    """tests/nlflux_ref.loss_fun with D(u) on the diffusion part and the advection as -u psi: psi [nT,1] tensor or None, dcoef
    (d0, d1, d2); phi / fcoef: the flux term (phi None: none); rate / coef: the reaction."""
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

    int1 = dfun(Val, dcoef) * (grad * gcoef).sum(dim=-1, keepdim=True)    # :653-654 with kappa -> kappa D(u)
    if psi is not None:
        int1 = int1 - Val * psi                                  # the advection, integrated by parts: - u psi
    if time_dependent:
        int1 = int1 - Val * dNt                                  # :655
    react = poly(Val, coef)                                      # p(u) at every row
    if rate is not None:
        react = rate * react
    if is_source:
        int1 = int1 - (source + react) * N                       # :657 with s -> s + rate p(u)
    else:
        int1 = int1 - react * N
    if phi is not None:
        int1 = int1 - poly(Val, fcoef) * phi                     # the flux term: - F(u) phi
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


def loss_and_grad(flat, d_in, widths, nldiff, nlflux=None, reaction=None, dtype=torch.float64, **kw):
    """nlflux_ref.loss_and_grad(flat, d_in, widths, nlflux, reaction, dtype, **kw) with the diffusivity.  nldiff = (psi, dcoef):
    psi a numpy column [nT,1] or None, dcoef up to three numbers; nldiff None: nlflux_ref itself."""
    if nldiff is None:
        return nlflux_ref.loss_and_grad(flat, d_in, widths, nlflux, reaction, dtype, **kw)
    psi, dcoef = nldiff
    rate, coef = (None, (0.0, 0.0, 0.0)) if reaction is None else reaction
    phi, fcoef = (None, (0.0, 0.0, 0.0)) if nlflux is None else nlflux
    params = og.unflatten(flat, d_in, widths, dtype=dtype, requires_grad=True)
    tk = {}
    for k, v in kw.items():
        tk[k] = torch.as_tensor(v, dtype=dtype) if isinstance(v, np.ndarray) else v
    col = lambda a: None if a is None else torch.as_tensor(np.reshape(np.asarray(a), (-1, 1)), dtype=dtype)
    out = loss_fun(params, rate=col(rate), coef=coef, phi=col(phi), fcoef=fcoef, psi=col(psi), dcoef=dcoef, **tk)
    out['loss'].backward()
    g = og.flatten_grads(params).detach().numpy()
    res = {k: (v.detach().numpy() if v.ndim else float(v.detach())) for k, v in out.items()}
    return res, g


def value_and_grad(flat, d_in, widths, dtype, Input, dim, time_dependent=True, activation='sigmoid'):
    """(u [n,1], grad_x u [n,dim]) as numpy, from oracle/tf1_graph.model_grad."""
    params = og.unflatten(flat, d_in, widths, dtype=dtype)
    Inp = torch.as_tensor(Input, dtype=dtype).clone().requires_grad_(True)
    Val, grad, _, _ = og.model_grad(params, Inp, dim, time_dependent, activation=activation)
    return Val.detach().numpy(), grad.detach().numpy()


def residual(flat, d_in, widths, dtype, Input, diff, vel, source, diff_dx, dim, nldiff, nlflux=None, reaction=None,
             time_dependent=True, activation='sigmoid'):
    """Strong residual with div(kappa D(u) grad u): nlflux_ref.residual evaluated with kappa -> kappa D(u) and grad kappa ->
    D(u) grad kappa, plus kappa D'(u) |grad u|^2.  nldiff = (d0, d1, d2) or None (nlflux_ref.residual itself).
    (model value [n,1], residual [n,1]) as numpy."""
    if nldiff is None:
        return nlflux_ref.residual(flat, d_in, widths, dtype, Input, diff, vel, source, diff_dx, dim, nlflux, reaction,
                                   time_dependent, activation)
    u, gu = value_and_grad(flat, d_in, widths, dtype, Input, dim, time_dependent, activation)
    diff = np.reshape(np.asarray(diff, dtype=u.dtype), (-1, 1))
    Du = dfun(u, nldiff)
    val, res = nlflux_ref.residual(flat, d_in, widths, dtype, Input, diff * Du, vel, source, np.asarray(diff_dx) * Du, dim, nlflux,
                                   reaction, time_dependent, activation)
    return val, res + ddfun(u, nldiff) * diff * (gu * gu).sum(axis=-1, keepdims=True)
