"""
Reference of the adaptive loss balancing (vn_balance.hip, varnet_amd/balance.py), written from the equations and not from either
implementation: the statistics of K fp32 vectors with exactly rounded sums (math.fsum of exact double products), and the two update
rules as plain loops over the terms.
"""
import math

import numpy as np

VAR = 2


def stats(T):
    """T [K, n] float32 -> (stats [K, 3] = (sumsq, sumabs, maxabs), gram [K, K], absgram [K, K] = sum |a_p b_p|), each sum the
    exactly rounded one of its exact terms.  maxabs ignores NaN entries (fmax)."""
    T = np.asarray(T)
    assert T.dtype == np.float32 and T.ndim == 2
    D = T.astype(np.float64)
    K = D.shape[0]
    st = np.zeros((K, 3))
    gram, absgram = np.zeros((K, K)), np.zeros((K, K))
    with np.errstate(all='ignore'):
        for a in range(K):
            ab = np.abs(D[a])
            st[a, 1] = _fsum(ab)
            finite = ab[~np.isnan(ab)]
            st[a, 2] = finite.max() if finite.size else 0.0
            for b in range(a, K):
                prod = D[a] * D[b]                       # exact: two 24-bit significands
                gram[a, b] = gram[b, a] = _fsum(prod)
                absgram[a, b] = absgram[b, a] = _fsum(np.abs(prod))
            st[a, 0] = gram[a, a]
    return st, gram, absgram


def _fsum(x):
    if not np.all(np.isfinite(x)):
        return float(np.sum(x))
    return math.fsum(x.tolist())


def sum_bar(n):
    """Relative bar of a sum of n non-negative exact terms accumulated in double in any order: at most n - 1 adds of relative
    2^-53 each; twice that first-order bound."""
    return n * 2.0 ** -52


def rule(name, w, w0, rho, active, norm, max_abs, mean_abs, L, alpha, cap, keep_loss):
    """One probe, term by term.  Returns (weights, skipped)."""
    K = len(w)
    act = [k for k in range(K) if active[k]]
    for k in act:
        if not (math.isfinite(norm[k]) and norm[k] > 0.0):
            return list(w), True
    hat = list(w)
    if name == 'gradnorm':
        tot = sum(norm[j] for j in act)
        for k in act:
            hat[k] = rho[k] * tot / norm[k]
    elif name == 'maxmean':
        for k in act:
            if k != VAR:
                hat[k] = rho[k] * w[VAR] * max_abs[VAR] / mean_abs[k]
    else:
        raise ValueError(name)
    new = list(w)
    for k in act:
        x = alpha * w[k] + (1.0 - alpha) * hat[k]
        new[k] = min(max(x, w0[k] / cap), w0[k] * cap)
    if keep_loss:
        c = sum(w[k] * L[k] for k in act) / sum(new[k] * L[k] for k in act)
        new = [x * c for x in new]
    return new, False
