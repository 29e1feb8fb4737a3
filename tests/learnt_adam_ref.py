"""
fp64 restatement of the step the three learnt vectors take (vn_learnt_apply_kernel of vn_learnt.hip; driven by learnt_finish in
vn_api.hip), its fp32 twin, named wrong variants of it, and the bar between the device and the restatement.
Plain module (no GPU, no pytest marks), shared by tests/test_learnt_adam_host.py and tests/test_learnt_adam_gpu.py.

The step of entry i at step counter t (masked entries only; the others and their slots are not touched):
    lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t)          formed in double, handed to the kernel as fp32
    m    = beta1 m + (1 - beta1) g
    v    = beta2 v + (1 - beta2) g g
    x    = clamp(x - lr_t m / (sqrt(v) + eps), lo, hi)    the slots are written whatever the clamp does
`Adam64` is oracle.tf1_graph.TF1Adam plus mask and clamp (tests/test_learnt_adam_host.py holds the two together to 1e-15) with the
hyper-parameters as the kernel receives them: beta1, beta2, eps, lr_t and the bounds rounded to fp32, g rounded to fp32 and widened
-- the rule of the existing first-step tests (test_train_step_is_adam_on_the_masked_*).  `Adam32` is the same recurrence in NumPy
fp32, operation by operation in the kernel's order; it serves only to measure the bar.

The bar of one step:   |device - Adam64| <= bar(before, after, lr_t) = ulp32(max(|before|, |after|)) / 2 + C lr_t
The first term is the rounding of the stored fp32 value.  C is MEASURED_C x C_FACTOR: MEASURED_C is the largest
(|Adam32 - Adam64| - ulp / 2) / lr_t over every step of every sequence of tests/learnt_cases.py, Adam64 started from Adam32's value
at each step; the factor 4 covers the fused multiply-adds the device compiler may contract and NumPy does not (about one ulp per
recurrence; no fast-math flag in the build, so sqrtf and the division are IEEE on both sides).  tests/test_learnt_adam_host.py
measures it again and fails on a stale constant; profiles/learnt_adam_parity.json records it.

MUTANTS: each a plausible slip of the kernels or of the host path, as a variant of Adam64.  The tests show, in NumPy alone, that each
leaves the bar on the sequences they run -- so a device that had the slip would have failed.
  a  beta1 and beta2 exchanged in the two recurrences
  b  slots not carried (zero before every step: stored to the wrong half of `state`, or not stored)
  c  lr_t formed from t - 1 (first step: from 1) or from t + 1
  d  lr_t frozen at t = 1
  e  a step with g == 0 skipped, where Adam moves the entry by its momentum
  f  slots zeroed by a value setter (vn_set_coefs / vn_set_source_amps / vn_set_field_amps)
  g  slots frozen while the entry sits on a bound
  h  gradient doubled on every second step (a fold that runs in both vn_grad and vn_apply: the tests' even steps are grad + apply)
About (h): a gradient doubled at EVERY step is no different step.  m doubles, v quadruples, m / sqrt(v) stays: Adam does not see
the scale of its gradient except through eps, and the doubled run is the true run with eps / 2 -- on the sequences here 1e-2 of
the bar at the most ('h_every_step' is kept to show that figure; nothing asserts on it).  What a trajectory can see, and does, is
a scale that changes between steps.
"""
import math

import numpy as np

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
C_FACTOR = 4.0
MEASURED_C = 5.452704912527487e-07          # (case 0, 'bound', coefficients: tests/test_learnt_adam_host.py prints all eighteen)
C = C_FACTOR * MEASURED_C

f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)


def lr_t_of(lr, t, rounded=True):
    """lr sqrt(1 - beta2^t) / (1 - beta1^t) in double; `rounded`: as the kernel receives it."""
    x = lr * math.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)
    return float(np.float32(x)) if rounded else x


def ulp32(x):
    """The spacing of fp32 at |x| (of the smallest normal number below it)."""
    return np.spacing(np.maximum(np.abs(np.asarray(x, dtype=np.float64)), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def bar(before, after, lr_t, c=None):
    return 0.5 * ulp32(np.maximum(np.abs(before), np.abs(after))) + (C if c is None else c) * lr_t


class Adam64:
    """The learnt vectors' step in fp64.  mask: the learnt entries; lo / hi: the clamp (None: unbounded).  rounded=False keeps the
    hyper-parameters and the gradient in double (the comparison with the oracle)."""

    def __init__(self, n, mask=None, lr=0.02, lo=None, hi=None, rounded=True):
        r = f32 if rounded else (lambda x: np.asarray(x, dtype=np.float64))
        self.n, self.lr, self.rounded = n, lr, rounded
        self.mask = np.ones(n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        self.lo = r(np.full(n, -np.inf) if lo is None else lo)
        self.hi = r(np.full(n, np.inf) if hi is None else hi)
        self.b1, self.b2, self.eps = float(r(BETA1)), float(r(BETA2)), float(r(EPS))
        self.m, self.v = np.zeros(n), np.zeros(n)
        self.unclamped = np.zeros(n)               # of the last step (unmasked entries: the value)

    def lr_t(self, t):
        return lr_t_of(self.lr, t, self.rounded)

    def on_set(self):
        """A value setter ran: the slots stay."""

    def _recur(self, value, g, t, on):
        m = np.where(on, self.b1 * self.m + (1.0 - self.b1) * g, self.m)
        v = np.where(on, self.b2 * self.v + (1.0 - self.b2) * g * g, self.v)
        return m, v

    def step(self, value, g, t):
        """The values after step t from `value`, with the gradient g; moves the slots."""
        value = np.asarray(value, dtype=np.float64)
        g = f32(g) if self.rounded else np.asarray(g, dtype=np.float64)
        on = self._on(value, g, t)
        self.m, self.v = self._recur(value, self._g(g, t), t, self._slots_on(value, on))
        moved = value - self.lr_t(t) * self.m / (np.sqrt(self.v) + self.eps)
        self.unclamped = np.where(on, moved, value)
        return np.where(on, np.minimum(np.maximum(moved, self.lo), self.hi), value)

    # (what the variants change)
    def _on(self, value, g, t):
        return self.mask

    def _slots_on(self, value, on):
        return on

    def _g(self, g, t):
        return g


class Adam32:
    """The same step in NumPy fp32, one rounding per operation, in the order the kernels write it."""

    def __init__(self, n, mask=None, lr=0.02, lo=None, hi=None):
        F = np.float32
        self.n, self.lr = n, lr
        self.mask = np.ones(n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        self.lo = np.asarray(np.full(n, -np.inf) if lo is None else lo, dtype=F)
        self.hi = np.asarray(np.full(n, np.inf) if hi is None else hi, dtype=F)
        self.b1, self.b2, self.eps = F(BETA1), F(BETA2), F(EPS)
        self.m, self.v = np.zeros(n, dtype=F), np.zeros(n, dtype=F)

    def step(self, value, g, t):
        F = np.float32
        value, gi = np.asarray(value, dtype=F), np.asarray(g, dtype=F)
        lr_t = F(lr_t_of(self.lr, t))
        mi = self.b1 * self.m + (F(1.0) - self.b1) * gi
        vi = self.b2 * self.v + (F(1.0) - self.b2) * gi * gi
        self.m, self.v = np.where(self.mask, mi, self.m), np.where(self.mask, vi, self.v)
        c = value - lr_t * mi / (np.sqrt(vi) + self.eps)
        assert c.dtype == F and mi.dtype == F and vi.dtype == F
        return np.where(self.mask, np.minimum(np.maximum(c, self.lo), self.hi), value)


class _BetasSwapped(Adam64):
    def _recur(self, value, g, t, on):
        m = np.where(on, self.b2 * self.m + (1.0 - self.b2) * g, self.m)
        v = np.where(on, self.b1 * self.v + (1.0 - self.b1) * g * g, self.v)
        return m, v


class _SlotsNotCarried(Adam64):
    def _recur(self, value, g, t, on):
        self.m, self.v = np.zeros(self.n), np.zeros(self.n)
        return Adam64._recur(self, value, g, t, on)


class _LrMinus(Adam64):
    def lr_t(self, t):
        return lr_t_of(self.lr, max(t - 1, 1), self.rounded)


class _LrPlus(Adam64):
    def lr_t(self, t):
        return lr_t_of(self.lr, t + 1, self.rounded)


class _LrFrozen(Adam64):
    def lr_t(self, t):
        return lr_t_of(self.lr, 1, self.rounded)


class _ZeroGradSkipped(Adam64):
    def _on(self, value, g, t):
        return self.mask & (g != 0.0)


class _SetterZeroesSlots(Adam64):
    def on_set(self):
        self.m, self.v = np.zeros(self.n), np.zeros(self.n)


class _FrozenOnBound(Adam64):
    def _slots_on(self, value, on):
        return on & (value != self.lo) & (value != self.hi)


class _DoubledOnEvenSteps(Adam64):
    def _g(self, g, t):
        return 2.0 * g if t % 2 == 0 else g


class _DoubledEveryStep(Adam64):
    def _g(self, g, t):
        return 2.0 * g


MUTANTS = {
    'a_betas_swapped': _BetasSwapped,
    'b_slots_not_carried': _SlotsNotCarried,
    'c_lr_t_of_t_minus_1': _LrMinus,
    'c_lr_t_of_t_plus_1': _LrPlus,
    'd_lr_t_frozen': _LrFrozen,
    'e_zero_gradient_skipped': _ZeroGradSkipped,
    'f_setter_zeroes_slots': _SetterZeroesSlots,
    'g_slots_frozen_on_bound': _FrozenOnBound,
    'h_gradient_doubled': _DoubledOnEvenSteps,
}
# (those any sequence of a few steps shows; the others need a zero gradient, a setter or a bound)
ANY_SEQUENCE = ['a_betas_swapped', 'b_slots_not_carried', 'c_lr_t_of_t_minus_1', 'c_lr_t_of_t_plus_1', 'd_lr_t_frozen',
                'h_gradient_doubled']
NOT_ASSERTED = {'h_every_step': _DoubledEveryStep}


def replay(cls, steps, n, mask=None, lr=0.02, lo=None, hi=None, c=None):
    """Teacher-forced run of the variant `cls` next to Adam64 over `steps`: a list of dicts with t, before, g, and optionally
    after (what was observed: the device's values; default: Adam64's own) and set (True: a value setter ran before this step).
    Returns err / bar of every step and entry, [len(steps), n]: |variant - observed| over bar(before, Adam64, lr_t)."""
    ref, mut = Adam64(n, mask, lr, lo, hi), cls(n, mask, lr, lo, hi)
    out = np.zeros((len(steps), n))
    for k, s in enumerate(steps):
        if s.get('set'):
            ref.on_set()
            mut.on_set()
        want = ref.step(s['before'], s['g'], s['t'])
        got = mut.step(s['before'], s['g'], s['t'])
        seen = want if s.get('after') is None else np.asarray(s['after'], dtype=np.float64)
        out[k] = np.abs(got - seen) / bar(s['before'], want, ref.lr_t(s['t']), c)
    return out
