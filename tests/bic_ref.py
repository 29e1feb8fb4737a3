"""
fp64 restatement of the weak-form loss with the BC/IC labels label = label0 + B a over a basis of J per-row streams and the
amplitudes a as a torch tensor, so that autograd also returns d loss / d a_j (boundary data identification: vn_set_bic_basis,
vn_set_bic_learn, `VarNet(learnBic=...)`).  The loss itself is tests/inverse_ref.loss_fun, called with the mixed labels as its
biLabel tensor; the nine polynomial coefficients go in as a constant tensor.

Besides the gradient g_j the reference returns, per component, the scale S_j = sum_k |row contribution|: the amplitude is broadcast
as a per-row tensor, and S_j is the sum of the absolute values of the gradient with respect to that tensor (the trick of
tests/source_ref.py).  |g_j| / S_j says how much cancellation the sum over the BC/IC rows carries.

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og
from tests import inverse_ref


def evaluate(flat, d_in, widths, label0, B, amp, coef, nldiff=None, nlflux=None, reaction=None, dtype=torch.float64, **kw):
    """(loss pieces, theta-gradient, amplitude gradient [J], scale S [J]) at amp [J].  label0: [nb] or [nb, 1]; B: [nb, J], nb the
    rows the loss evaluates (a steady problem: the boundary rows only); coef: the nine polynomial coefficients; nldiff / nlflux /
    reaction name the streams and which terms are present, as for tests/inverse_ref.evaluate; **kw as for
    tests/nldiff_ref.loss_and_grad (its `biLabel` is replaced)."""
    f = np.float64 if dtype == torch.float64 else np.float32
    kw = dict(kw)
    kw.pop('biLabel', None)
    tk = {k: (torch.as_tensor(v, dtype=dtype) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    col = lambda a: None if a is None else torch.as_tensor(np.reshape(np.asarray(a), (-1, 1)).astype(f), dtype=dtype)
    streams = dict(rate=col(reaction[0]) if reaction is not None else None, phi=col(nlflux[0]) if nlflux is not None else None,
                   psi=col(nldiff[0]) if nldiff is not None else None,
                   has=(reaction is not None, nlflux is not None, nldiff is not None))
    nb, J = B.shape
    Bt = torch.as_tensor(np.asarray(B).astype(f), dtype=dtype)
    base = col(label0)
    c = torch.tensor(np.asarray(coef, dtype=f), dtype=dtype)
    params = og.unflatten(np.asarray(flat).astype(f), d_in, widths, dtype=dtype, requires_grad=True)
    a = torch.tensor(np.asarray(amp, dtype=f), dtype=dtype, requires_grad=True)
    out = inverse_ref.loss_fun(params, c, biLabel=base + Bt @ a.reshape(J, 1), **streams, **tk)
    out['loss'].backward()
    g = og.flatten_grads(params).detach().numpy()
    ga = a.grad.detach().numpy().astype(np.float64)
    # the scale: the same loss with a per-row copy of every amplitude
    params2 = og.unflatten(np.asarray(flat).astype(f), d_in, widths, dtype=dtype)
    arow = torch.tensor(np.tile(np.asarray(amp, dtype=f), (nb, 1)), dtype=dtype, requires_grad=True)
    inverse_ref.loss_fun(params2, c, biLabel=base + (Bt * arow).sum(dim=1, keepdim=True), **streams, **tk)['loss'].backward()
    S = arow.grad.detach().abs().sum(dim=0).numpy().astype(np.float64)
    res = {k: (v.detach().numpy() if v.ndim else float(v.detach())) for k, v in out.items()}
    return res, g, ga, S
