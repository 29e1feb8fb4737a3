"""
Adaptive loss balancing from per-term gradient norms: the two update rules, on the host, in NumPy (no engine).

The objective of an epoch is  w_bc BC + w_ic IC + w_var var + w_obs O  on the scale of the TRAIN weights (what `trainWeight`
produced).  Every `freq` epochs the engine measures the gradient of each term at unit weight (vn_term_grads): its 2-norm n_k, its
largest and its mean absolute entry mx_k, mean_k -- after the caller has scaled the BC, IC and observation figures by
1 / (batchNum * puNum), the factor `towerWeights` puts on those weights, so that they are the figures of the terms of the epoch
objective.  With A the active terms (train weight > 0 and rows) and rho_k = weight_k / weight_var the user's stated preference:

    'gradnorm'  (Wang, Sankaran, Wang, Perdikaris 2023)   w^_k = rho_k * (sum_{j in A} n_j) / n_k
    'maxmean'   (Wang, Teng, Perdikaris 2021)             w^_var = w_var;   w^_k = rho_k * w_var * mx_var / mean_k   (k != var)

then, in this order:  w_k <- alpha w_k + (1 - alpha) w^_k;  w_k / w0_k clamped to [1 / cap, cap] (w0: what trainWeight produced);
with keepLoss every weight times c = sum w_old L / sum w_new L, which keeps the weighted loss continuous at the probe (the
reference's `alpha`; `tol` and `min_loss` stay meaningful, and Adam does not see the scale).  A zero or non-finite squared norm of
an active term leaves the weights alone, and the record says so.
"""
import numpy as np

TERMS = ('bc', 'ic', 'var', 'obs')
VAR = 2
RULES = ('gradnorm', 'maxmean')
DEFAULTS = {'rule': None, 'freq': 1000, 'alpha': 0.9, 'cap': 1e4, 'keepLoss': True}


def parse_balance(balance):
    """The `balance` option of VarNet.train as a full dict, or None: None | 'gradnorm' | 'maxmean' | {'rule', 'freq': 1000,
    'alpha': 0.9, 'cap': 1e4, 'keepLoss': True}; anything else is a ValueError."""
    if balance is None:
        return None
    if isinstance(balance, str):
        balance = {'rule': balance}
    if not isinstance(balance, dict):
        raise ValueError("balance must be None, 'gradnorm', 'maxmean' or a dict with the key 'rule' (got %r)" % (balance,))
    unknown = sorted(set(balance) - set(DEFAULTS))
    if unknown:
        raise ValueError('balance: unknown key %r (the keys are %s)' % (unknown[0], ', '.join(sorted(DEFAULTS))))
    cfg = dict(DEFAULTS)
    cfg.update(balance)
    if cfg['rule'] not in RULES:
        raise ValueError("balance: the rule must be 'gradnorm' or 'maxmean' (got %r)" % (cfg['rule'],))
    f = cfg['freq']
    if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or f < 1:
        raise ValueError('balance: freq must be an integer >= 1 (got %r)' % (f,))
    a = cfg['alpha']
    if isinstance(a, bool) or not isinstance(a, (int, float, np.floating)) or not (0.0 <= float(a) < 1.0):
        raise ValueError('balance: alpha must be in [0, 1) (got %r)' % (a,))
    c = cfg['cap']
    if isinstance(c, bool) or not isinstance(c, (int, float, np.floating)) or not (float(c) >= 1.0) or not np.isfinite(c):
        raise ValueError('balance: cap must be a finite number >= 1 (got %r)' % (c,))
    cfg.update(freq=int(f), alpha=float(a), cap=float(c), keepLoss=bool(cfg['keepLoss']))
    return cfg


def targets(rule, w, rho, active, norm, max_abs, mean_abs):
    """The rule's target weights w^ (inactive terms keep w)."""
    w = np.array(w, dtype=float)
    what = w.copy()
    A = np.flatnonzero(active)
    if rule == 'gradnorm':
        total = float(np.sum(np.asarray(norm, dtype=float)[A]))
        for k in A:
            what[k] = rho[k] * total / norm[k]
    elif rule == 'maxmean':
        for k in A:
            if k != VAR:
                what[k] = rho[k] * w[VAR] * max_abs[VAR] / mean_abs[k]
    else:
        raise ValueError("balance: the rule must be 'gradnorm' or 'maxmean' (got %r)" % (rule,))
    return what


def update(rule, w, w0, rho, active, sumsq, max_abs, mean_abs, L, alpha=0.9, cap=1e4, keepLoss=True):
    """One probe.  All vectors are over TERMS at train scale (figures already scaled by the caller); `active` is a boolean mask.
    Returns (w_new, skipped): skipped is True, and w_new is w, when an active squared norm is zero or not finite."""
    w = np.array(w, dtype=float)
    active = np.asarray(active, dtype=bool)
    sumsq = np.asarray(sumsq, dtype=float)
    ss = sumsq[active]
    if ss.size == 0 or not np.all(np.isfinite(ss)) or np.any(ss <= 0.0):
        return w, True
    if rule == 'maxmean' and not np.all(np.asarray(mean_abs, dtype=float)[active] > 0.0):
        return w, True
    norm = np.sqrt(np.where(active, sumsq, 0.0))
    what = targets(rule, w, np.asarray(rho, dtype=float), active, norm, np.asarray(max_abs, dtype=float), np.asarray(mean_abs, dtype=float))
    new = w.copy()
    new[active] = alpha * w[active] + (1.0 - alpha) * what[active]
    w0 = np.asarray(w0, dtype=float)
    new[active] = np.clip(new[active], w0[active] / cap, w0[active] * cap)
    if not np.all(np.isfinite(new)):
        return w, True
    if keepLoss:
        L = np.asarray(L, dtype=float)
        den = float(np.sum(new[active] * L[active]))
        num = float(np.sum(w[active] * L[active]))
        if np.isfinite(num) and np.isfinite(den) and den > 0.0 and num > 0.0:
            new = new * (num / den)
    return new, False


def cosines(gram):
    """The cosine matrix of a Gram matrix; rows and columns of a zero vector are zeros."""
    G = np.asarray(gram, dtype=float)
    d = np.sqrt(np.clip(np.diag(G), 0.0, None))
    out = np.zeros_like(G)
    ok = d > 0.0
    out[np.ix_(ok, ok)] = G[np.ix_(ok, ok)] / np.outer(d[ok], d[ok])
    return out
