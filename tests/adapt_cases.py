"""
Host-side tables of the self-adaptive weight tests (vn_set_tf_adapt, `VarNet(tfAdapt=...)`): the seven cases of
tests/reaction_cases.py (imported, not edited; n_k = 300, 40, 5, 9, 3, 5, 40: below a wave, and across a 256-function seed block)
and three more on the (1, 1, [20], q = 4) network of case 0:

    n_k = 1       one test function: max = mean = the only entry, omega = 1 under normalisation
    n_k = 33      one past the de-duplicated step's 32-function loss partial
    n_k = 2739    2.67 spans of the update kernels' 1024-function block span, not a multiple of 4: three blocks fold in order,
                  the last one ends in a partial span and a scalar tail

Inputs: tests/parity_cases.synth(seed 11), parameters glorot_init(seed 3) + 0.05 N(0,1) (default_rng(5)), as in
tests/reaction_cases.py.  Initial state: lambda = default_rng(31).uniform(0.5, 2, n_k) rounded to fp32, so the weights are real
(`weights_are_real`, asserted on the registration of the weights-in-use tests, `parity_spec`: without normalisation; for
n_k = 1 the normalised weight is 1 by construction, so `spec_of` drops the normalisation for that case everywhere).

The single-update bar is MEASURED here (`single_update_bar`): the fp32 restatement of one update (tests/adapt_ref.py) against the
fp64 one over eight chained updates on the cases' own loss fields, plus an allowance in ulps for what the device may round
differently from NumPy.  Plain module (no GPU, no pytest marks), shared by tests/test_adapt_host.py and tests/test_adapt_gpu.py.
"""
import functools

import numpy as np
import torch

from tests import adapt_ref, causal_ref, nldiff_cases, nlflux_cases, reaction_cases
from tests.parity_cases import synth

BASE = len(reaction_cases.CASES)
_NET0 = reaction_cases.CASES[0]
EXTRA_NK = (1, 33, 2739)
CASES = list(reaction_cases.CASES) + [_NET0[:4] + (n_k,) + _NET0[5:] for n_k in EXTRA_NK]
IDS = list(reaction_cases.IDS) + ['1d_steady_%d' % n_k for n_k in EXTRA_NK]
SPAN = 1024                                  # VN_ADAPT_SPAN of varnet_amd/csrc/vn_adapt.h
assert EXTRA_NK[2] % SPAN != 0 and EXTRA_NK[2] >= 2.5 * SPAN and EXTRA_NK[2] % 4 != 0
SINGLE_CASES = (0, 1, 3, BASE, BASE + 1, BASE + 2)
RULES = ('rba', 'sa')


@functools.lru_cache(maxsize=None)
def inputs(i):
    """The inputs dict of CASES[i]: computed once, shared, never modified."""
    if i < BASE:
        return reaction_cases.inputs(i)[0]
    d_in, dim, widths, q, n_k, nB, bDof, td, act, source, integW, detJvec, rows = CASES[i]
    d = synth(11, d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec)
    d['N_rows'] = d['dNt_rows'] = None
    # few test functions against the one boundary row: the variational term would be under 1 % of the gradient at synth's weights
    # (3, 2, 5) and the weights under test with it; its weight grows with (300 / n_k)^2 so that it stands beside the BC term
    d['w'] = np.array([3.0, 2.0, 5.0 * max(1.0, (300.0 / n_k) ** 2)])
    return d


def theta(i):
    return reaction_cases.theta(i if i < BASE else 0)                        # the extra cases share case 0's network


def ref_kw(i, dtype=torch.float64):
    if i < BASE:
        return reaction_cases.ref_kw(i, dtype)
    d_in, dim, widths, q, n_k, nB, bDof, td, act, source, integW, detJvec, rows = CASES[i]
    d = inputs(i)
    f = np.float64 if dtype == torch.float64 else np.float32
    nb = nB if td else bDof
    return dict(Input=d['Input'].astype(f), gcoef=d['gcoef'].astype(f), source=None, N=d['N'].astype(f), dNt=d['dNt'].astype(f),
                integW=None, intShape=[n_k, q], detJ=float(d['detJ']), detJvec=False, biInput=d['biInput'][:nb].astype(f),
                biLabel=d['biLabel'][:nb].astype(f), bDof=bDof, biDimVal=2.0, w=d['w'], dim=dim, time_dependent=td,
                is_source=False, integWflag=False, activation=act)


@functools.lru_cache(maxsize=None)
def lambda0(i):
    return np.random.default_rng(31).uniform(0.5, 2.0, CASES[i][4]).astype(np.float32)


def spec_of(i, rule, **kw):
    """The rule's defaults; the one-function case without normalisation (its normalised weight is 1 whatever lambda is)."""
    if CASES[i][4] == 1:
        kw.setdefault('normalize', False)
    return adapt_ref.spec_of(rule, **kw)


def parity_spec(rule='rba', **kw):
    """The registration of the weights-in-use tests: no normalisation, omega = lambda^2 with mean 1.75 or so.  (Under
    normalisation the mean weight is 1 and var moves only through the correlation of omega with l: below 1e-2 on cases 0, 1, 3
    and the 33-function case, measured with this very seed, which would leave `weights_are_real` nothing to hold on to.)"""
    kw.setdefault('normalize', False)
    return adapt_ref.spec_of(rule, **kw)


def omega0(i, rule='rba'):
    """The weights of the initial state under parity_spec, fp64."""
    return adapt_ref.weights(lambda0(i), parity_spec(rule))[0]


def terms_of(i, variant):
    if variant == 'plain':
        return None, None, None
    assert variant == 'terms' and i < BASE, (variant, i)
    nlflux, reaction = nlflux_cases.terms_of(i, 'both')
    return (nldiff_cases.psi(i), nldiff_cases.DIFF), nlflux, reaction


def reference(i, omega=None, variant='plain', flat=None, dtype=torch.float64):
    """tests/causal_ref.loss_and_grad on CASES[i] with omega as static weights (None: weights 1)."""
    f = np.float64 if dtype == torch.float64 else np.float32
    flat = theta(i) if flat is None else flat
    cast = lambda t: None if t is None else (None if t[0] is None else t[0].astype(f), t[1])
    nldiff, nlflux, reaction = (cast(t) for t in terms_of(i, variant))
    return causal_ref.loss_and_grad(np.asarray(flat).astype(f), CASES[i][0], CASES[i][2], omega, None, nldiff, nlflux, reaction,
                                    dtype, **ref_kw(i, dtype))


@functools.lru_cache(maxsize=None)
def reference64(i, weighted=True, variant='plain'):
    """The fp64 reference of CASES[i] under the initial state's weights (or none), computed once."""
    return reference(i, omega0(i) if weighted else None, variant)


def weights_are_real(i, variant='plain'):
    """In the reference: removing the weights moves varLoss and the gradient norm by more than 1e-2 relative."""
    ref, g = reference64(i, True, variant)
    ref0, g0 = reference64(i, False, variant)
    assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss']), (ref['varLoss'], ref0['varLoss'])
    assert np.linalg.norm(g - g0) > 1e-2 * np.linalg.norm(g)


# ---- the single-update bar, measured ------------------------------------------------------------------------------------
ULP32 = 2.0 ** -23                           # the largest relative size of one fp32 ulp
# What the device may round differently from the fp32 NumPy restatement, in ulps, from the error bounds the HIP programming
# guide's math tables give for the functions vn_adapt.hip actually calls -- __fsqrt_rn and __fdiv_rn, 1 ulp each in the single
# precision intrinsics table -- plus 1 ulp for every multiply-add the compiler may contract into one fma (NumPy rounds twice).
#   rba: sqrt(l_k), sqrt(max l), the division r_k / r_max, one contracted multiply-add                      = 4
#   sa:  the divisions l_k / lbar and m1 / (sqrt(m2) + eps), sqrt(m2), the three contracted updates of m1, m2, lambda   = 6
# omega = m(lambda) / Z squares lambda (power 2) and divides by a mean of squares: twice the allowance of lambda.
DEVICE_ULPS = {'rba': 4, 'sa': 6}


def rel_dev(got, want):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    den = np.maximum(np.abs(want), 1e-30)
    return float(np.max(np.abs(got - want) / den)) if want.size else 0.0


@functools.lru_cache(maxsize=None)
def single_update_bar(rule):
    """dict(measured_lambda, measured_omega, measured_slots, allowance_ulps, bar): the largest relative deviation of one fp32
    update from the fp64 one over eight chained updates on SINGLE_CASES (each fp32 update starts from the fp64 chain's state
    rounded to fp32, on the case's fp64 reference loss field rounded to fp32, scaled per step so the field moves), and
    bar = max(measured) + 2 * allowance_ulps * ULP32.  The GPU tests read their bar from here, never from the engine."""
    dev = {'lambda': 0.0, 'omega': 0.0, 'slots': 0.0}
    for i in SINGLE_CASES:
        spec = spec_of(i, rule)
        lv = reference64(i, False)[0]['lossVec'].reshape(-1).astype(np.float32)
        lam, slots, tau = lambda0(i).astype(np.float64), None, 0
        mod = np.random.default_rng(32).uniform(0.5, 1.5, (8, lv.size)).astype(np.float32)
        for s in range(8):
            l = lv * mod[s]
            want = adapt_ref.step(lam, slots, tau, l, spec)
            lam32 = lam.astype(np.float32)
            slots32 = None if slots is None else slots.astype(np.float32)
            got = adapt_ref.step(lam32, slots32, tau, l, spec, dtype=np.float32)
            # (against the fp64 step from the SAME rounded state, so the figure is the update's error alone)
            base = adapt_ref.step(lam32.astype(np.float64), None if slots32 is None else slots32.astype(np.float64), tau, l, spec)
            dev['lambda'] = max(dev['lambda'], rel_dev(got['lam'], base['lam']))
            dev['omega'] = max(dev['omega'], rel_dev(got['omega'], base['omega']))
            if base['slots'] is not None:
                dev['slots'] = max(dev['slots'], rel_dev(got['slots'], base['slots']))
            lam, slots, tau = want['lam'], want['slots'], want['tau']
    ulps = DEVICE_ULPS[rule]
    bar = max(dev.values()) + 2 * ulps * ULP32
    return dict(measured_lambda=dev['lambda'], measured_omega=dev['omega'], measured_slots=dev['slots'], allowance_ulps=ulps,
                device_functions=['__fsqrt_rn', '__fdiv_rn', 'fma contraction'], bar=bar)
