"""
fp64 restatement of the JOINT problem: the weak-form loss of tests/inverse_ref.loss_fun evaluated once with every learnt vector in
the graph -- the nine polynomial coefficients (vn_set_coef_learn), source = s0 + Phi a_s (tests/source_ref.py), gcoef = g0 + sum_j
b_j G_j (tests/field_ref.py), labels = label0 + B a_b (tests/bic_ref.py) -- plus the edge terms as their own modules add them: the
boundary-flux rows at label = label0 + Gamma^T a[:Jl], coef = coef0 + H^T a[Jl:] (tests/fbc_ref.py; tests/flux_ref.flux_term
without a basis) and the periodic pairs (tests/periodic_ref.periodic_term) joining BCloss under w0, the observations
(tests/obs_ref.obs_term) under lambda.  Optionally per-test-function weights, static or causal, formed as
tests/causal_ref.loss_and_grad forms them (the engine refuses weights next to a learnt vector, so the two never meet here either).
It composes the existing restatements and adds no mathematics of its own: with nothing learnt and no extra edge set it is
tests/fuzz_terms.reference bit for bit, with one vector the matching single-vector module (tests/test_fuzz_learnt_host.py).

The problems of the fuzz always carry Dirichlet rows (bDof >= 1), so the bDof == 0 convention of tests/periodic_ref.loss_and_grad
(mean_D = 0) is the plain mean here and is asserted, not restated.

Per learnt vector the reference returns the gradient g_j and the conditioning scale S_j = sum_rows |row contribution|: every
amplitude is broadcast as a per-row tensor in a second pass (all vectors at once), and S_j is the sum of the absolute values of the
gradient with respect to that tensor -- the trick of tests/inverse_ref.evaluate and tests/source_ref.evaluate.

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np
import torch

from oracle import tf1_graph as og
from tests import causal_ref, fbc_ref, flux_ref, inverse_ref, obs_ref, periodic_ref

VECTORS = ('coef', 'source', 'field', 'bic', 'fluxbc')


def _interior(params, c, streams, tk, src, fld, bic, per_row=False):
    """tests/inverse_ref.loss_fun at the mixed source, direction and labels.  src = (base [nT,1], Phi [nT,J], a), fld = (G
    [J,nT,dim], b), bic = (B [nB,J], a) or None; per_row: the amplitudes are per-row copies (a [nT,J], b [J,nT], a [nB,J])."""
    tk = dict(tk)
    if src is not None:
        base, P, a = src
        tk['source'] = base + ((P * a).sum(dim=1, keepdim=True) if per_row else P @ a.reshape(-1, 1))
        tk['is_source'] = True
    if fld is not None:
        G, b = fld
        J, nT = G.shape[0], G.shape[1]
        tk['gcoef'] = tk['gcoef'] + ((b.reshape(J, nT, 1) if per_row else b.reshape(J, 1, 1)) * G).sum(dim=0)
    if bic is not None:
        B, a = bic
        tk['biLabel'] = tk['biLabel'] + ((B * a).sum(dim=1, keepdim=True) if per_row else B @ a.reshape(-1, 1))
    return inverse_ref.loss_fun(params, c, **streams, **tk)


def evaluate(flat, d_in, widths, terms, kw, dtype=torch.float64, coef=None, learn_coef=False, source=None, field=None, bic=None,
             flux=None, periodic=None, obs=None, omega=None, causal=None, scales=True):
    """(loss pieces incl. lossVec and, with observations, 'obs'; theta-gradient [P]; {vector: (gradient, S)}).

    terms: {name: (stream or None, coefficients)} as tests/fuzz_terms.py draws them; coef: the nine values the terms are evaluated
    at (None: those of `terms`); learn_coef: return their gradient.  kw: the keywords of tests/nldiff_ref.loss_and_grad (numpy, any
    precision).  source = (s0 [nT,1] or None, Phi [J,nT], amp [J]); field = (G [J,nT,dim], amp); bic = (B [J,nB], amp) -- streams
    stream-major as the engine takes them; flux = dict(X, normal, coef, label[, S [J,nF], Jl, amp]); periodic = dict(X, dir, gamma);
    obs = dict(X, value, lam[, q, dir, rowptr, wgt]); omega [n_k] or causal = (slab, n_slabs, eps): only with no vector learnt."""
    f = np.float64 if dtype == torch.float64 else np.float32
    cv = lambda a: None if a is None else np.asarray(a).astype(f)
    t = lambda a: torch.as_tensor(cv(a), dtype=dtype)
    flat = np.asarray(flat).astype(f)
    weighted = omega is not None or causal is not None
    assert not (weighted and (learn_coef or source or field or bic or (flux is not None and 'S' in flux))), 'weights next to a learnt vector'
    assert kw['bDof'] >= 1
    tk = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    nldiff, nlflux, reaction = terms.get('nldiff'), terms.get('nlflux'), terms.get('reaction')
    col = lambda a: None if a is None else t(np.reshape(np.asarray(a), (-1, 1)))
    streams = dict(rate=col(reaction[0]) if reaction is not None else None, phi=col(nlflux[0]) if nlflux is not None else None,
                   psi=col(nldiff[0]) if nldiff is not None else None,
                   has=(reaction is not None, nlflux is not None, nldiff is not None))
    nine = inverse_ref.nine(nldiff, nlflux, reaction) if coef is None else np.asarray(coef, dtype=np.float64)
    nT = tk['Input'].shape[0]
    w = np.asarray(kw['w'], dtype=np.float64)

    def parts(per_row):
        """The tensors of one pass: (c, src, fld, bic, leaves by vector name)."""
        leaf = {}
        rep = lambda a, n: np.tile(np.asarray(a, dtype=f), (n, 1))
        if learn_coef:
            leaf['coef'] = torch.tensor(rep(nine, nT) if per_row else nine.astype(f), dtype=dtype, requires_grad=True)
        c = leaf.get('coef', torch.tensor(nine.astype(f), dtype=dtype))
        src = fld = bc = None
        if source is not None:
            s0, Phi, amp = source
            leaf['source'] = torch.tensor(rep(amp, nT) if per_row else np.asarray(amp, dtype=f), dtype=dtype, requires_grad=True)
            src = (torch.zeros((nT, 1), dtype=dtype) if s0 is None else col(s0), t(np.asarray(Phi).T), leaf['source'])
        if field is not None:
            G, amp = field
            J = len(amp)
            leaf['field'] = torch.tensor(np.tile(np.asarray(amp, dtype=f).reshape(J, 1), (1, nT)) if per_row else np.asarray(amp, dtype=f),
                                         dtype=dtype, requires_grad=True)
            fld = (t(G), leaf['field'])
        if bic is not None:
            B, amp = bic
            leaf['bic'] = torch.tensor(rep(amp, np.asarray(B).shape[1]) if per_row else np.asarray(amp, dtype=f), dtype=dtype,
                                       requires_grad=True)
            bc = (t(np.asarray(B).T), leaf['bic'])
        return c, src, fld, bc, leaf

    params = og.unflatten(flat, d_in, widths, dtype=dtype, requires_grad=True)
    c, src, fld, bc, leaf = parts(False)
    vec = {}
    if weighted:
        # tests/causal_ref.loss_and_grad on inverse_ref.loss_fun: lossVec unweighted, omega a constant of the graph
        detJ, detJvec = tk['detJ'], tk['detJvec']
        tkw = dict(tk, detJ=tk['detJ'] if detJvec else 1.0)
        out = _interior(params, c, streams, tkw, None, None, None)
        r2 = out['lossVec']
        lossVec = r2 if detJvec else detJ * r2
        if causal is not None:
            om, om_slab = causal_ref.causal_weights(lossVec.detach().numpy(), *causal)
        else:
            om, om_slab = np.asarray(omega, dtype=np.float64).reshape(-1), None
        assert om.size == r2.shape[0]
        om_t = torch.as_tensor(om.reshape(-1, 1), dtype=dtype)
        var = (om_t * r2).sum() if detJvec else detJ * (om_t * r2).sum()
        loss = tk['w'][0] * out['BCloss'] + tk['w'][1] * out['ICloss'] + tk['w'][2] * var
        loss.backward()
        res = dict(loss=float(loss.detach()), BCloss=float(out['BCloss'].detach()), ICloss=float(out['ICloss'].detach()),
                   varLoss=float(var.detach()), lossVec=lossVec.detach().numpy(), omega=om)
        if om_slab is not None:
            res['omega_slab'] = om_slab
    else:
        out = _interior(params, c, streams, tk, src, fld, bc)
        out['loss'].backward()
        res = {k: (v.detach().numpy() if v.ndim else float(v.detach())) for k, v in out.items()}
    g = np.asarray(og.flatten_grads(params).detach().numpy(), dtype=np.float64)
    grads = {k: (np.zeros(v.shape) if v.grad is None else v.grad.detach().numpy().astype(np.float64)) for k, v in leaf.items()}
    if leaf:
        S = {}
        if scales:
            params2 = og.unflatten(flat, d_in, widths, dtype=dtype)
            c2, src2, fld2, bc2, leaf2 = parts(True)
            _interior(params2, c2, streams, tk, src2, fld2, bc2, per_row=True)['loss'].backward()
            for k, v in leaf2.items():
                a = torch.zeros_like(v) if v.grad is None else v.grad.detach().abs()
                S[k] = a.sum(dim=1 if k == 'field' else 0).numpy().astype(np.float64)
        for k in leaf:
            vec[k] = (grads[k], S.get(k))
    # ---- edge terms, as their modules add them
    act = kw.get('activation', 'sigmoid')
    dim, bdv = kw['dim'], kw['biDimVal']
    res = dict(res)
    if flux is not None:
        if 'S' in flux:
            F, gF, ga, Sa = fbc_ref.evaluate(flat, d_in, widths, dim, cv(flux['X']), cv(flux['normal']), cv(flux['coef']),
                                             cv(flux['label']), cv(flux['S']), int(flux['Jl']), cv(flux['amp']), bdv, float(w[0]), act, dtype)
            vec['fluxbc'] = (ga, Sa)
        else:
            F, gF, _ = flux_ref.flux_term(flat, d_in, widths, dim, cv(flux['X']), cv(flux['normal']), cv(flux['coef']),
                                          cv(flux['label']), bdv, act, dtype)
        res['BCloss'] = res['BCloss'] + F
        res['loss'] = res['loss'] + w[0] * F
        g = g + w[0] * gF
    if periodic is not None:
        P, gP, _, _ = periodic_ref.periodic_term(flat, d_in, widths, dim, cv(periodic['X']), cv(periodic['dir']), float(periodic['gamma']),
                                                 bdv, act, dtype)
        res['BCloss'] = res['BCloss'] + P
        res['loss'] = res['loss'] + w[0] * P
        g = g + w[0] * gP
    if obs is not None:
        O, gO, _ = obs_ref.obs_term(flat, d_in, widths, dim, cv(obs['X']), cv(obs['value']), cv(obs.get('q')), cv(obs.get('dir')),
                                    obs.get('rowptr'), cv(obs.get('wgt')), act, dtype)
        lam = float(obs['lam'])
        res['obs'] = O
        res['loss'] = res['loss'] + lam * O
        g = g + lam * gO
    return res, g, vec
