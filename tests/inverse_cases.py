"""
Host-side tables of the inverse-mode tests (vn_set_coef_learn): the fp64 reference of tests/inverse_ref.py on the ten cases of
tests/dedup_term_cases.py (row-wise data Input = Xu[uid] plus a shared-point map), computed once per (case, variant) and never
modified, and the bar of the coefficient gradient.  Plain module (no GPU, no pytest marks), shared by tests/test_inverse_host.py and
tests/test_inverse_gpu.py.

The bar, per component m:   |g_m - g64_m| <= GRAD_RTOL * max(|g64_m|, COND_FLOOR * S_m)
with S_m = sum_r |row contribution| (tests/inverse_ref.py).  The floor may be the binding branch for at most BINDING_CAP of the 90
components of the ten 'all' cases; tests/test_inverse_host.py asserts that from the fp64 numbers alone.
"""
import functools

import numpy as np
import torch

from tests import inverse_ref
from tests.dedup_term_cases import CASES, ref_kw, terms_of, theta
from tests.parity_cases import GRAD_RTOL

COND_FLOOR = 0.01
BINDING_CAP = 3
NAMES = ['c1', 'c2', 'c3', 'f1', 'f2', 'f3', 'd0', 'd1', 'd2']
GROUP = {'react': 0, 'flux': 1, 'd': 2, 'psi': 2}


def coefs_of(i, variant):
    return inverse_ref.nine(*terms_of(i, variant))


def evaluate(i, variant, coef=None, dtype=torch.float64):
    nldiff, nlflux, reaction = terms_of(i, variant)
    coef = coefs_of(i, variant) if coef is None else coef
    return inverse_ref.evaluate(theta(i), CASES[i][0], CASES[i][2], coef, nldiff, nlflux, reaction, dtype, **ref_kw(i, dtype))


@functools.lru_cache(maxsize=None)
def reference64(i, variant='all'):
    """(loss pieces, theta-gradient, coefficient gradient [9], S [9]) of CASES[i] in fp64 at the case's own coefficients."""
    out = evaluate(i, variant)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def bars(g64, S):
    """The allowed |g - g64| per component."""
    return GRAD_RTOL * np.maximum(np.abs(g64), COND_FLOOR * S)


def present(variant):
    """The entries (of nine) whose term a variant carries."""
    m = np.zeros(9, dtype=bool)
    if variant == 'all':
        m[:] = True
    else:
        m[3 * GROUP[variant]:3 * GROUP[variant] + 3] = True
    return m
