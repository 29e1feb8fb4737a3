"""
The vectors, priors and sequences the tests of the learnt vectors' regularisation run (tests/test_prior_host.py,
tests/test_prior_gpu.py).  Plain module (no GPU, no pytest marks).

Vectors -- the smallest at which vn_learnt_apply_kernel can go wrong:
  lc<i>/coef, /source, /field   the nine coefficients (the 16-lane fold) and the J = 3 source and field amplitudes of cases 0 and 6
                                of tests/learnt_cases.py, cut into its two batches and stepped on its schedule
  fbc/<Jl>+<Jc>                 the flux-row amplitudes of case 1 of tests/fbc_cases.py at (1, 0): J = 1, (5, 4), (37, 27) and
                                (40, 24): J = 64, the cap
  bic/3                         the boundary / initial amplitudes of case 0 of tests/bic_cases.py, J = 3
Every vector gets the same kind of registration (config()), from its case's own values a0 and its fp64 reference gradient:
  mask    all entries, but entry 1 where J >= 3 (an unmasked entry whose fixed value still enters d)
  start   a0, but entry 2 where J >= 3 starts at 0.2 lr, inside the first step's shrinkage threshold 0.316 lr l1
  bounds  entry 0 within +- 0.5 lr of its start: Adam's first move is lr, the shrinkage takes 0.316 lr of it back at the most, so
          one of the two bounds is reached at step 1 whatever the sign of the gradient; at J = 1, where entry 0 is the only one and
          has to show the shrinkage too, within +- 1.5 lr, reached at the second step
  l1      1 on entries 0, 2 and every fourth one, 0 on the others (which keep the arithmetic they had; J = 3 has no room for one)
  R       dense random positive semi-definite of rank J - 1, mean = start + 0.5 N(0, 1): non-zero
  weight  so that |weight R d| over the masked entries at the start is half the geometric mean of the batches' data gradient
          norms: Adam does not see a small prior (the host tier asserts a factor 10 at the most between the two, at every step),
          and at J = 1 the two cannot cancel
The host sequences hold each batch's data gradient at its reference value (tests/learnt_cases.reference64 and its siblings): the
prior's part moves with the values, the data's does not.  Eight steps, odd ones as vn_train_step, even ones as vn_grad + vn_apply.
"""
import functools

import numpy as np

from tests import bic_cases as bc
from tests import fbc_cases as fc
from tests import learnt_adam_ref as ar
from tests import learnt_cases as lc
from tests import prior_ref as pr

LR = lc.LR
K = lc.K
SCHEDULE = lc.SCHEDULE
FBC_CASE, FBC_VARIANTS = 1, [(1, 0), (5, 4), (37, 27), (40, 24)]
BIC_CASE, BIC_J = 0, 3
RATIO = 10.0                          # |weight R d| and the data gradient's norm are within this factor of each other


def config(tag, a0, grads, seed):
    """The registration of one vector (module docstring): dict(tag, n, mask, start, lo, hi, prior, near_zero, bounded, unmasked)."""
    a0 = np.asarray(a0, dtype=np.float64)
    n = a0.size
    rng = np.random.default_rng(seed)
    mask = np.ones(n, dtype=bool)
    start = ar.f32(a0).copy()
    near_zero = unmasked = None
    if n >= 3:
        unmasked, near_zero = 1, 2
        mask[unmasked] = False
        start[near_zero] = ar.f32(0.2 * LR * (np.sign(a0[near_zero]) or 1.0))
    lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
    half = (0.5 if n >= 3 else 1.5) * LR
    lo[0], hi[0] = ar.f32(start[0] - half), ar.f32(start[0] + half)
    l1 = np.where(np.arange(n) % 4 == 0, 1.0, 0.0)
    if near_zero is not None:
        l1[near_zero] = 1.0
    R = pr.random_psd(rng, n)
    mean = start + 0.5 * rng.standard_normal(n)
    unit = pr.Prior64(n, 1.0, R, mean, l1, mask)
    norms = [np.linalg.norm(np.asarray(g, dtype=np.float64)[mask]) for g in grads]
    weight = float(0.5 * np.exp(np.mean(np.log(norms))) / np.linalg.norm(unit.grad(start)[mask]))
    return dict(tag=tag, n=n, mask=mask, start=start, lo=lo, hi=hi, prior=pr.Prior64(n, weight, R, mean, l1, mask),
                near_zero=near_zero, bounded=0, unmasked=unmasked)


@functools.lru_cache(maxsize=None)
def lc_configs(i):
    """{vector: config} of the three vectors of case i of tests/learnt_cases.py."""
    ref = [lc.reference64(i, which) for which in (0, 1)]
    return {k: config('lc%d/%s' % (i, k), lc.initial(i)[k], [r[k][0] for r in ref], 1000 + 10 * i + n) for n, k in enumerate(lc.VECTORS)}


@functools.lru_cache(maxsize=None)
def fbc_config(Jl, Jc):
    return config('fbc/%d+%d' % (Jl, Jc), fc.basis(FBC_CASE, Jl, Jc)[1], [fc.reference64(FBC_CASE, Jl, Jc)[2]], 2000 + 64 * Jl + Jc)


@functools.lru_cache(maxsize=None)
def bic_config():
    return config('bic/%d' % BIC_J, bc.basis(BIC_CASE, BIC_J)[1], [bc.reference64(BIC_CASE, BIC_J)[2]], 3000)


def data_gradients():
    """Every (config, the data gradient of steps 1..K) the two tiers run."""
    for i in lc.CASES:
        for k, cfg in lc_configs(i).items():
            yield cfg, [lc.reference64(i, which)[k][0] for which in SCHEDULE]
    for Jl, Jc in FBC_VARIANTS:
        yield fbc_config(Jl, Jc), [fc.reference64(FBC_CASE, Jl, Jc)[2]] * K
    yield bic_config(), [bc.reference64(BIC_CASE, BIC_J)[2]] * K


def after_grad(t):
    """Odd steps through vn_train_step, even ones through vn_grad + vn_apply."""
    return t % 2 == 0


def run64(cfg, grads):
    """The fp64 sequence of a config on the data gradients `grads`: step records (t, before, g_data, after_grad, g, after,
    unclamped)."""
    ref = pr.Step64(cfg['prior'], LR, cfg['lo'], cfg['hi'])
    x, steps = cfg['start'].copy(), []
    for t, g_data in enumerate(grads, 1):
        g, after = ref.step(x, g_data, t, after_grad(t))
        steps.append(dict(t=t, before=x.copy(), g_data=np.asarray(g_data, dtype=np.float64), after_grad=after_grad(t), g=g, after=after.copy(),
                          unclamped=ref.adam.unclamped.copy()))
        x = after
    return steps


@functools.lru_cache(maxsize=None)
def sequences():
    """((config, steps), ...) of every vector, computed once."""
    return tuple((cfg, tuple(run64(cfg, grads))) for cfg, grads in data_gradients())


def shows(cfg, name):
    """Whether the vector of `cfg` has what the variant `name` needs to show (tests/prior_ref.NEEDS)."""
    need = pr.NEEDS.get(name)
    return need is None or cfg[need] is not None
