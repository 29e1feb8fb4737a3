"""
Host-side tables of the quasilinear-diffusion tests (vn_set_nldiff, `ADPDE(nldiff=[d0, d1, d2])`): the seven cases of
tests/reaction_cases.py, their seeded inputs and the fp64 / fp32 evaluations of tests/nldiff_ref.py on them.  Plain module (no
GPU, no pytest marks), shared by tests/test_nldiff_host.py and tests/test_nldiff_gpu.py.

Inputs: those of tests/reaction_cases.py with gcoef x 8 and the parameters x 2 (both exact in fp32).  As they stand a deep sigmoid
net at glorot scale has almost no spatial gradient, so D(u) would move the compared quantities by little more than their bars; with
the two scalings each of D and psi alone moves every compared quantity by at least 100 x its bar, which
tests/test_nldiff_host.py::test_inputs_make_a_missing_term_fail asserts from the fp64 reference.  psi = PSI_SCALE x
default_rng(15).standard_normal((nT, 1)) rounded to fp32 (the engine registers fp32 rows), D = (0.7, 0.4, 0.3).
Variants: 'dpsi' (D and psi), 'd' (D, psi = None), 'psi' (D = 1 with psi), 'all' (D, psi, the reaction's rate stream and COEF, the
flux term's phi and FLUX), 'rf' (reaction + flux alone: nlflux_ref), 'pm' (D = (0, 0, 1): degenerate, with psi), 'none' (the oracle).
"""
import functools

import numpy as np
import torch

from tests import nldiff_ref, reaction_cases
from tests.nlflux_cases import FLUX, phi  # noqa: F401  (re-exported)
from tests.reaction_cases import CASES, COEF, IDS  # noqa: F401  (re-exported)

DIFF = (0.7, 0.4, 0.3)
DEGENERATE = (0.0, 0.0, 1.0)
GCOEF_SCALE = 8.0
THETA_SCALE = 2.0
PSI_SCALE = 8.0


@functools.lru_cache(maxsize=None)
def inputs(i):
    """(inputs dict, rate [nT,1] fp32) of CASES[i] with gcoef x 8: computed once, shared, never modified."""
    d, rate = reaction_cases.inputs(i)
    d = dict(d)
    d['gcoef'] = (np.float32(GCOEF_SCALE) * d['gcoef']).astype(np.float32)
    return d, rate


@functools.lru_cache(maxsize=None)
def theta(i):
    return (np.float32(THETA_SCALE) * reaction_cases.theta(i)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def psi(i):
    """psi [nT,1] fp32 of CASES[i]: computed once, shared, never modified."""
    n = CASES[i][4] * CASES[i][3]
    return (np.float32(PSI_SCALE) * np.random.default_rng(15).standard_normal((n, 1)).astype(np.float32)).astype(np.float32)


def ref_kw(i, dtype=torch.float64):
    return reaction_cases.ref_kw(i, dtype, d=inputs(i)[0])


def terms_of(i, variant):
    """(nldiff, nlflux, reaction) of a variant: nldiff = (psi or None, dcoef) or None, nlflux = (phi, fcoef) or None, reaction =
    (rate, coef) or None."""
    rate = inputs(i)[1]
    return {'dpsi': ((psi(i), DIFF), None, None), 'd': ((None, DIFF), None, None), 'psi': ((psi(i), (1.0, 0.0, 0.0)), None, None),
            'all': ((psi(i), DIFF), (phi(i), FLUX), (rate, COEF)), 'rf': (None, (phi(i), FLUX), (rate, COEF)),
            'pm': ((psi(i), DEGENERATE), None, None), 'none': (None, None, None)}[variant]


def reference(i, variant, flat=None, dtype=torch.float64):
    """tests/nldiff_ref.loss_and_grad on CASES[i] for a variant."""
    f = np.float64 if dtype == torch.float64 else np.float32
    flat = theta(i) if flat is None else flat
    cast = lambda t: None if t is None else (None if t[0] is None else t[0].astype(f), t[1])
    nldiff, nlflux, reaction = (cast(t) for t in terms_of(i, variant))
    return nldiff_ref.loss_and_grad(np.asarray(flat).astype(f), CASES[i][0], CASES[i][2], nldiff, nlflux, reaction, dtype,
                                    **ref_kw(i, dtype))


@functools.lru_cache(maxsize=None)
def reference64(i, variant='dpsi'):
    """The fp64 reference of CASES[i], computed once per variant."""
    return reference(i, variant)
