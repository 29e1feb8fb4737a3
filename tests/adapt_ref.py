"""
NumPy restatement of the self-adaptive test-function weights (vn_set_tf_adapt, `VarNet(tfAdapt=...)`): both update rules, the
normalisation and the statistics, in fp64 (the reference) or in fp32 (dtype=np.float32: what the single-update bar of
tests/adapt_cases.py is measured from).  With l_k >= 0 the unweighted loss field of a step, lambda_k >= 0 the state and tau the
count of updates that moved it:

    weights     omega_k = m(lambda_k) / Z,  m(x) = x^p (p = 1, 2),  Z = mean_j m(lambda_j) if normalize else 1
    rba         r_k = sqrt(l_k):  lambda'_k = gamma lambda_k + eta r_k / max_j r_j
    sa          g_k = m'(lambda_k) l_k / mean_j l_j,  m1 = b1 m1 + (1 - b1) g,  m2 = b2 m2 + (1 - b2) g^2,
                lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) with t = tau + 1,  lambda'_k = clip(lambda_k + lr_t m1 / (sqrt(m2) + eps), 0, cap)
    max_j l_j (rba) or mean_j l_j (sa) zero or not finite: the state does not move (lambda, slots, tau kept)
    statistics  min, max, mean omega, effective sample share (sum omega)^2 / (n_k sum omega^2), Z, tau

Loss and gradient under the weights: tests/causal_ref.loss_and_grad with omega passed as static weights (the weights are a
constant of the gradient).

Test infrastructure (imported by the tests; not a conftest).
"""
import numpy as np

RBA = dict(rule='rba', gamma=0.999, eta=0.01, power=2, init=1.0, normalize=True, every=1)
SA = dict(rule='sa', lr=0.005, beta1=0.9, beta2=0.999, eps=1e-8, cap=1e3, power=2, init=1.0, normalize=True, every=1)
DEFAULTS = {'rba': RBA, 'sa': SA}


def spec_of(rule, **kw):
    s = dict(DEFAULTS[rule])
    s.update(kw)
    return s


def m_fun(lam, power):
    return lam * lam if power == 2 else lam


def weights(lam, spec, dtype=np.float64):
    """(omega [n_k], Z, stats dict without tau) of a state.  In fp32 mode m is formed in fp32 (as the kernel does) and
    everything after it in fp64 with one rounding of omega to fp32, the kernel's own order."""
    lam = np.asarray(lam, dtype=dtype).reshape(-1)
    m = m_fun(lam, spec['power']).astype(np.float64)
    n = m.size
    Z = float(m.sum() / n) if spec['normalize'] else 1.0
    if not (Z > 0.0 and np.isfinite(Z)):
        Z = 1.0
    om = m / Z
    s1, s2 = float(m.sum()), float((m * m).sum())
    stats = dict(min=float(m.min() / Z), max=float(m.max() / Z), mean=s1 / (n * Z), share=(s1 * s1 / (n * s2) if s2 > 0.0 else 0.0), Z=Z)
    return (om.astype(np.float32) if dtype == np.float32 else om), Z, stats


def update(lam, slots, tau, lossVec, spec, dtype=np.float64):
    """One update from a step's loss field: (lambda', slots' [2, n_k] or None, tau').  dtype np.float32: every elementwise
    operation rounded to fp32, the reductions (max, mean) and lr_t in fp64, as in the kernel."""
    f = dtype
    lam = np.asarray(lam, dtype=f).reshape(-1)
    l = np.asarray(lossVec, dtype=f).reshape(-1)
    assert lam.size == l.size
    slots = None if slots is None else np.asarray(slots, dtype=f).reshape(2, -1)
    if spec['rule'] == 'rba':
        lmax = float(np.max(l.astype(np.float64))) if np.all(np.isfinite(l)) else np.inf
        if not (lmax > 0.0 and np.isfinite(lmax)):
            return lam.copy(), None, tau
        r = np.sqrt(np.maximum(l, f(0)))
        rmax = np.sqrt(f(lmax))
        return (f(spec['gamma']) * lam + f(spec['eta']) * (r / rmax)).astype(f), None, tau + 1
    assert spec['rule'] == 'sa'
    if slots is None:
        slots = np.zeros((2, lam.size), dtype=f)
    with np.errstate(invalid='ignore'):
        lbar = float(np.sum(l.astype(np.float64)) / l.size)
    if not (lbar > 0.0 and np.isfinite(lbar) and f(lbar) > 0 and np.isfinite(f(lbar))):
        return lam.copy(), slots.copy(), tau
    b1, b2 = f(spec['beta1']), f(spec['beta2'])
    mp = f(2) * lam if spec['power'] == 2 else np.ones_like(lam)
    g = mp * (l / f(lbar))
    m1 = b1 * slots[0] + f(1.0 - spec['beta1']) * g                  # (1 - beta formed in double, as in the kernel)
    m2 = b2 * slots[1] + f(1.0 - spec['beta2']) * (g * g)
    t = tau + 1.0
    lr_t = f(spec['lr'] * np.sqrt(1.0 - spec['beta2'] ** t) / (1.0 - spec['beta1'] ** t))
    lam1 = np.clip(lam + lr_t * (m1 / (np.sqrt(m2) + f(spec['eps']))), f(0), f(spec['cap']))
    return lam1.astype(f), np.stack([m1, m2]).astype(f), tau + 1


def step(lam, slots, tau, lossVec, spec, dtype=np.float64):
    """update + weights: what a committed step leaves -- dict(lam, slots, tau, omega, Z, stats) with stats['tau']."""
    lam1, slots1, tau1 = update(lam, slots, tau, lossVec, spec, dtype)
    om, Z, stats = weights(lam1, spec, dtype)
    stats['tau'] = float(tau1)
    return dict(lam=lam1, slots=slots1, tau=tau1, omega=om, Z=Z, stats=stats)


def rba_bound(spec):
    """lambda_k <= max(init, eta / (1 - gamma)) at all times (gamma < 1)."""
    return max(spec['init'], spec['eta'] / (1.0 - spec['gamma'])) if spec['gamma'] < 1.0 else np.inf
