"""
fp64 restatement of the weak-form loss with the tangent direction gcoef = g0 + sum_j b_j G_j over a basis of J per-row streams of
dim floats per row and the amplitudes b as a torch tensor, so that autograd also returns d loss / d b_j (field identification:
vn_set_field_basis, vn_set_field_learn, `VarNet(learnField=...)`).  The loss itself is tests/inverse_ref.loss_fun, which takes
gcoef as a tensor and so carries the graph; the nine polynomial coefficients go in as a constant tensor.  At b = 0 it is
tests/inverse_ref.evaluate on g0 (tests/test_field_host.py checks that to 1e-13).

Besides the gradient g_j the reference returns, per component, the scale S_j = sum_r |row contribution|: the amplitude is broadcast
as a per-row tensor, and S_j is the sum of the absolute values of the gradient with respect to that tensor (the trick of
tests/inverse_ref.evaluate).  |g_j| / S_j says how much cancellation the sum over rows carries.

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og
from tests import inverse_ref


def evaluate(flat, d_in, widths, g0, G, amp, coef, nldiff=None, nlflux=None, reaction=None, dtype=torch.float64, **kw):
    """(loss pieces, theta-gradient, amplitude gradient [J], scale S [J]) at amp [J].  g0: [nT, dim]; G: [J, nT, dim] or None (no
    basis: amp is ignored, the two amplitude outputs are empty); coef: the nine polynomial coefficients; nldiff / nlflux / reaction
    name the streams and which terms are present, as for tests/inverse_ref.evaluate; **kw as for tests/nldiff_ref.loss_and_grad
    (its `gcoef` is replaced)."""
    f = np.float64 if dtype == torch.float64 else np.float32
    kw = dict(kw)
    kw.pop('gcoef', None)
    tk = {k: (torch.as_tensor(v, dtype=dtype) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    col = lambda a: None if a is None else torch.as_tensor(np.reshape(np.asarray(a), (-1, 1)).astype(f), dtype=dtype)
    streams = dict(rate=col(reaction[0]) if reaction is not None else None, phi=col(nlflux[0]) if nlflux is not None else None,
                   psi=col(nldiff[0]) if nldiff is not None else None,
                   has=(reaction is not None, nlflux is not None, nldiff is not None))
    base = torch.as_tensor(np.asarray(g0).astype(f), dtype=dtype)
    c = torch.tensor(np.asarray(coef, dtype=f), dtype=dtype)
    params = og.unflatten(np.asarray(flat).astype(f), d_in, widths, dtype=dtype, requires_grad=True)
    if G is None:
        out = inverse_ref.loss_fun(params, c, gcoef=base, **streams, **tk)
        out['loss'].backward()
        res = {k: (v.detach().numpy() if v.ndim else float(v.detach())) for k, v in out.items()}
        return res, og.flatten_grads(params).detach().numpy(), np.zeros(0), np.zeros(0)
    J, nT = G.shape[0], G.shape[1]
    B = torch.as_tensor(np.asarray(G).astype(f), dtype=dtype)
    b = torch.tensor(np.asarray(amp, dtype=f), dtype=dtype, requires_grad=True)
    out = inverse_ref.loss_fun(params, c, gcoef=base + (b.reshape(J, 1, 1) * B).sum(dim=0), **streams, **tk)
    out['loss'].backward()
    g = og.flatten_grads(params).detach().numpy()
    gb = b.grad.detach().numpy().astype(np.float64)
    # the scale: the same loss with a per-row copy of every amplitude
    params2 = og.unflatten(np.asarray(flat).astype(f), d_in, widths, dtype=dtype)
    brow = torch.tensor(np.tile(np.asarray(amp, dtype=f).reshape(J, 1), (1, nT)), dtype=dtype, requires_grad=True)
    inverse_ref.loss_fun(params2, c, gcoef=base + (brow.reshape(J, nT, 1) * B).sum(dim=0), **streams, **tk)['loss'].backward()
    S = brow.grad.detach().abs().sum(dim=1).numpy().astype(np.float64)
    res = {k: (v.detach().numpy() if v.ndim else float(v.detach())) for k, v in out.items()}
    return res, g, gb, S
