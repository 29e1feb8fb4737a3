"""
fp64 restatement of the regularisation of the learnt vectors (vn_set_learnt_prior; the prior part of vn_learnt_apply_kernel in
vn_learnt.hip), its fp32 twin, named wrong variants of it, and the bars between the device and the
restatement.  Plain module (no GPU, no pytest marks), shared by tests/test_prior_host.py and tests/test_prior_gpu.py; the vectors
and sequences the two tiers run are in tests/prior_cases.py.

A learnt vector a of length J with learnt mask M, at step counter t:
    d      = a - mean                                   a as the gradient evaluation read it, unmasked entries included
    grad_j = data_j + weight (R d)_j   (j in M),  0 (else)    fp64, inside the fold of a gradient evaluation only
    (m, v) = Adam's recurrences on float32(grad)          tests/learnt_adam_ref.py
    c      = a - lr_t m / (sqrt(v) + eps)
    c      = copysign(max(|c| - lr_t l1_j, 0), c)         where l1_j > 0: the proximal map of lr_t l1_j |.|
    a      = clamp(c, lo, hi)
    Q      = 1/2 weight d^T R d,      L = sum_j l1_j |a_j|        read on demand; no part of any reported loss

Bars.
  gradient   |g1 - g0 - weight (R d)_j| <= (J + 3) 2^-52 (|g0_j| + weight sum_i |R_ji| |d_i|): the forward error of a length-J fp64 sum
             (J - 1 additions and J products, or J fused multiply-adds) plus the product with the weight and the addition to g0.
  Q          (2 J + 4) 2^-52 1/2 weight sum_ij |d_i R_ij d_j|: two nested length-J sums and the two factors.
  L          (J + 2) 2^-52 sum_j l1_j |a_j|
  step       tests/learnt_adam_ref.bar with C = 4 max(MEASURED_C, MEASURED_C_PRIOR): MEASURED_C_PRIOR is the largest
             (|Adam32Prox - Adam64Prox| - ulp / 2) / lr_t over every step of every sequence of tests/prior_cases.py, measured the way
             MEASURED_C is; the factor 4 stands for the same reason (fused multiply-adds the device compiler may contract).
             tests/test_prior_host.py measures it again and fails on a stale constant; profiles/prior_parity.json records it.

MUTANTS: each a plausible slip of the kernel or of the host path, as a variant of Step64.  The tests show, in NumPy alone, that each
leaves a bar on the sequences they run -- so a device that had the slip would have failed.  What each needs of a sequence:
  a  prior gradient with the wrong sign                     weight > 0
  b  mean ignored (d = a)                                   weight > 0, mean != 0
  c  prior also added on the unmasked entries               weight > 0, an unmasked entry (the gradient bar of that entry)
  d  prior added again in an apply after a gradient call    weight > 0, a step taken as vn_grad + vn_apply
  e  d taken from the values after the update               weight > 0 (a race: threads that step before others have read)
  f  shrinkage before Adam's move                           an entry with l1 > 0 that starts within lr_t l1 of zero
  g  shrinkage threshold lr l1 in place of lr_t l1          l1 > 0
  h  shrinkage after the clamp                              an entry with l1 > 0 that reaches a bound
  i  shrinkage fed into the gradient as l1 sign(a)          l1 > 0 (no proximal map then)
"""
import copy

import numpy as np

from tests import learnt_adam_ref as ar
from tests.learnt_adam_ref import Adam32, Adam64, f32

U = 2.0 ** -52
MEASURED_C_PRIOR = 1.4609413538822369e-05   # ('fbc/37+27': tests/test_prior_host.py prints all eleven; values of 2 to 3 and two more roundings)
C = ar.C_FACTOR * max(ar.MEASURED_C, MEASURED_C_PRIOR)


def bar(before, after, lr_t):
    """The step's bar: tests/learnt_adam_ref.bar with the constant of this module."""
    return ar.bar(before, after, lr_t, c=C)


def over(err, allowed):
    """err / allowed per entry; where nothing is allowed, 0 for no error and inf for any."""
    err, allowed = np.asarray(err, dtype=np.float64), np.asarray(allowed, dtype=np.float64)
    safe = np.where(allowed > 0.0, allowed, 1.0)
    return np.where(allowed > 0.0, err / safe, np.where(err > 0.0, np.inf, 0.0))


# ---- the matrices ------------------------------------------------------------------------------------------------------------
def identity(n):
    return np.eye(n)


def difference(n):
    """D^T D of the first differences (D a)_i = a_{i+1} - a_i in amplitude order."""
    D = np.diff(np.eye(n), axis=0)
    return D.T @ D


def block_diag(blocks):
    n = sum(b.shape[0] for b in blocks)
    out, i0 = np.zeros((n, n)), 0
    for b in blocks:
        out[i0:i0 + b.shape[0], i0:i0 + b.shape[0]] = b
        i0 += b.shape[0]
    return out


def random_psd(rng, n):
    """A dense symmetric positive semi-definite matrix of rank max(n - 1, 1) with entries of order one, exactly symmetric."""
    A = rng.standard_normal((n, max(n - 1, 1)))
    R = A @ A.T / max(n - 1, 1)
    return 0.5 * (R + R.T)


# ---- the prior ---------------------------------------------------------------------------------------------------------------
class Prior64:
    """Quadratic prior and L1 weights of one vector in fp64: R None is the identity, mean None zeros, l1 None no shrinkage (its
    entries as the engine stores them: fp32)."""

    def __init__(self, n, weight=0.0, R=None, mean=None, l1=None, mask=None):
        self.n, self.weight = n, float(weight)
        self.R = np.eye(n) if R is None else np.asarray(R, dtype=np.float64)
        self.mean = np.zeros(n) if mean is None else np.asarray(mean, dtype=np.float64)
        self.l1 = np.zeros(n) if l1 is None else f32(l1)
        self.mask = np.ones(n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        assert self.R.shape == (n, n) and np.array_equal(self.R, self.R.T) and self.mean.shape == (n,) and self.l1.shape == (n,)

    def d(self, a):
        return np.asarray(a, dtype=np.float64) - self.mean

    def grad_all(self, a):
        """weight R d on every entry."""
        return self.weight * (self.R @ self.d(a))

    def grad(self, a):
        """... on the masked entries, 0 on the others: what the fold adds."""
        return np.where(self.mask, self.grad_all(a), 0.0)

    def grad_bound(self, a, g0):
        return (self.n + 3) * U * (np.abs(g0) + self.weight * (np.abs(self.R) @ np.abs(self.d(a))))

    def Q(self, a):
        d = self.d(a)
        return 0.5 * self.weight * float(d @ self.R @ d)

    def Q_bound(self, a):
        d = np.abs(self.d(a))
        return (2 * self.n + 4) * U * 0.5 * self.weight * float(d @ np.abs(self.R) @ d)

    def L1(self, a):
        return float(np.sum(self.l1 * np.abs(np.asarray(a, dtype=np.float64))))

    def L1_bound(self, a):
        return (self.n + 2) * U * self.L1(a)


# ---- the step ----------------------------------------------------------------------------------------------------------------
class Adam64Prox(Adam64):
    """tests/learnt_adam_ref.Adam64 with the proximal shrinkage between Adam's move and the clamp."""
    ORDER = 'move-prox-clamp'

    def __init__(self, n, mask=None, lr=0.02, lo=None, hi=None, rounded=True, l1=None):
        Adam64.__init__(self, n, mask, lr, lo, hi, rounded)
        self.l1 = np.zeros(n) if l1 is None else (f32(l1) if rounded else np.asarray(l1, dtype=np.float64))

    def threshold(self, t):
        return self.lr_t(t) * self.l1

    def prox(self, c, t):
        return np.where(self.l1 > 0.0, np.copysign(np.maximum(np.abs(c) - self.threshold(t), 0.0), c), c)

    def step(self, value, g, t):
        value = np.asarray(value, dtype=np.float64)
        g = f32(g) if self.rounded else np.asarray(g, dtype=np.float64)
        on = self._on(value, g, t)
        start = self.prox(value, t) if self.ORDER == 'prox-move-clamp' else value
        self.m, self.v = self._recur(value, self._g(g, t), t, self._slots_on(value, on))
        moved = start - self.lr_t(t) * self.m / (np.sqrt(self.v) + self.eps)
        if self.ORDER == 'move-prox-clamp':
            moved = self.prox(moved, t)
        self.unclamped = np.where(on, moved, value)
        out = np.minimum(np.maximum(moved, self.lo), self.hi)
        if self.ORDER == 'move-clamp-prox':
            out = self.prox(out, t)
        return np.where(on, out, value)


class Adam32Prox(Adam32):
    """The same step in NumPy fp32, one rounding per operation, in the order the kernel writes it."""

    def __init__(self, n, mask=None, lr=0.02, lo=None, hi=None, l1=None):
        Adam32.__init__(self, n, mask, lr, lo, hi)
        self.l1 = np.zeros(n, dtype=np.float32) if l1 is None else np.asarray(l1, dtype=np.float32)

    def step(self, value, g, t):
        F = np.float32
        value, gi = np.asarray(value, dtype=F), np.asarray(g, dtype=F)
        lr_t = F(ar.lr_t_of(self.lr, t))
        mi = self.b1 * self.m + (F(1.0) - self.b1) * gi
        vi = self.b2 * self.v + (F(1.0) - self.b2) * gi * gi
        self.m, self.v = np.where(self.mask, mi, self.m), np.where(self.mask, vi, self.v)
        c = value - lr_t * mi / (np.sqrt(vi) + self.eps)
        c = np.where(self.l1 > 0, np.copysign(np.maximum(np.abs(c) - lr_t * self.l1, F(0.0)), c), c)
        assert c.dtype == F
        return np.where(self.mask, np.minimum(np.maximum(c, self.lo), self.hi), value)


class _ProxBeforeMove(Adam64Prox):
    ORDER = 'prox-move-clamp'


class _ProxAfterClamp(Adam64Prox):
    ORDER = 'move-clamp-prox'


class _ProxPlainLr(Adam64Prox):
    def threshold(self, t):
        return float(np.float32(self.lr)) * self.l1


class _NoProx(Adam64Prox):
    def prox(self, c, t):
        return c


class Step64:
    """One vector's whole step under a prior: step() returns (the gradient the engine reports, the values after the step).
    `after_grad`: the step is a vn_apply after a vn_grad (else one vn_train_step)."""
    ADAM = Adam64Prox

    def __init__(self, prior, lr=0.02, lo=None, hi=None):
        self.p = prior
        self.adam = self.ADAM(prior.n, prior.mask, lr, lo, hi, l1=prior.l1)

    def reported(self, before, g_data, t):
        return np.where(self.p.mask, np.asarray(g_data, dtype=np.float64) + self.p.grad_all(before), 0.0)

    def fed(self, before, g, t, after_grad):
        return g

    def step(self, before, g_data, t, after_grad=False):
        g = self.reported(before, g_data, t)
        return g, self.adam.step(before, self.fed(before, g, t, after_grad), t)


class _WrongSign(Step64):
    def reported(self, before, g_data, t):
        return np.where(self.p.mask, np.asarray(g_data, dtype=np.float64) - self.p.grad_all(before), 0.0)


class _MeanIgnored(Step64):
    def reported(self, before, g_data, t):
        return np.where(self.p.mask, np.asarray(g_data, dtype=np.float64) + self.p.weight * (self.p.R @ np.asarray(before, dtype=np.float64)), 0.0)


class _OnUnmasked(Step64):
    def reported(self, before, g_data, t):
        return np.where(self.p.mask, np.asarray(g_data, dtype=np.float64), 0.0) + self.p.grad_all(before)


class _AddedAgain(Step64):
    def fed(self, before, g, t, after_grad):
        return g + self.p.grad(before) if after_grad else g


class _PostUpdate(Step64):
    def reported(self, before, g_data, t):
        trial = copy.deepcopy(self.adam).step(before, Step64.reported(self, before, g_data, t), t)
        return np.where(self.p.mask, np.asarray(g_data, dtype=np.float64) + self.p.grad_all(trial), 0.0)


class _ProxBefore(Step64):
    ADAM = _ProxBeforeMove


class _ProxLr(Step64):
    ADAM = _ProxPlainLr


class _ProxClamp(Step64):
    ADAM = _ProxAfterClamp


class _ProxInGrad(Step64):
    ADAM = _NoProx

    def reported(self, before, g_data, t):
        return Step64.reported(self, before, g_data, t) + np.where(self.p.mask, self.p.l1 * np.sign(before), 0.0)


MUTANTS = {
    'a_prior_sign': _WrongSign,
    'b_mean_ignored': _MeanIgnored,
    'c_prior_on_unmasked': _OnUnmasked,
    'd_prior_added_again_in_apply': _AddedAgain,
    'e_d_from_updated_values': _PostUpdate,
    'f_prox_before_move': _ProxBefore,
    'g_prox_threshold_plain_lr': _ProxLr,
    'h_prox_after_clamp': _ProxClamp,
    'i_prox_in_grad': _ProxInGrad,
}
# what a vector must have for a variant to show (the others show on every vector with weight > 0 and l1 > 0)
NEEDS = {'c_prior_on_unmasked': 'unmasked', 'f_prox_before_move': 'near_zero'}


def replay(cls, steps, prior, lr=0.02, lo=None, hi=None):
    """Teacher-forced run of the variant `cls` next to Step64 over `steps`: a list of dicts with t, before, g_data, after_grad, and
    optionally after and g (what was observed: the device's values and reported gradient; default: Step64's own).  Returns the
    largest of (|variant - observed| over the step's bar, |variant's gradient - observed gradient| over the gradient bar) of every
    step and entry, [len(steps), n]."""
    ref, mut = Step64(prior, lr, lo, hi), cls(prior, lr, lo, hi)
    out = np.zeros((len(steps), prior.n))
    for k, s in enumerate(steps):
        g_want, want = ref.step(s['before'], s['g_data'], s['t'], s['after_grad'])
        g_got, got = mut.step(s['before'], s['g_data'], s['t'], s['after_grad'])
        seen = want if s.get('after') is None else np.asarray(s['after'], dtype=np.float64)
        g_seen = g_want if s.get('g') is None else np.asarray(s['g'], dtype=np.float64)
        g0 = np.where(prior.mask, np.asarray(s['g_data'], dtype=np.float64), 0.0)
        out[k] = np.maximum(over(np.abs(got - seen), bar(s['before'], want, ref.adam.lr_t(s['t']))),
                            over(np.abs(g_got - g_seen), prior.grad_bound(s['before'], g0)))
    return out
