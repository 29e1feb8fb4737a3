"""
Host-side tables of the flux-term tests (vn_set_nlflux, `ADPDE(nlflux=...)`): the seven cases of tests/reaction_cases.py, their
seeded inputs and the fp64 / fp32 evaluations of tests/nlflux_ref.py on them.  Plain module (no GPU, no pytest marks), shared by
tests/test_nlflux_host.py and tests/test_nlflux_gpu.py.

Inputs: those of tests/reaction_cases.py (synth(seed 11), parameters glorot_init(seed 3) + 0.05 N(0,1)), phi =
default_rng(14).standard_normal((nT, 1)) rounded to fp32 (the engine registers fp32 rows), flux coefficients (0.6, 0.5, -0.3).
Variants: 'flux' (FLUX), 'linear' ((0.7, 0, 0)), 'both' (FLUX plus the reaction's rate stream and COEF), 'react' (the reaction
alone: reaction_ref), 'none' (the oracle).
"""
import functools

import numpy as np
import torch

from tests import nlflux_ref
from tests.reaction_cases import CASES, COEF, IDS, inputs, ref_kw, theta  # noqa: F401  (re-exported)

FLUX = (0.6, 0.5, -0.3)
LINEAR = (0.7, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def phi(i):
    """phi [nT,1] fp32 of CASES[i]: computed once, shared, never modified."""
    n = CASES[i][4] * CASES[i][3]
    return np.random.default_rng(14).standard_normal((n, 1)).astype(np.float32)


def terms_of(i, variant):
    """(nlflux, reaction) of a variant: nlflux = (phi, fcoef) or None, reaction = (rate, coef) or None."""
    rate = inputs(i)[1]
    return {'flux': ((phi(i), FLUX), None), 'linear': ((phi(i), LINEAR), None), 'both': ((phi(i), FLUX), (rate, COEF)),
            'react': (None, (rate, COEF)), 'none': (None, None)}[variant]


def reference(i, variant, flat=None, dtype=torch.float64):
    """tests/nlflux_ref.loss_and_grad on CASES[i] for a variant."""
    f = np.float64 if dtype == torch.float64 else np.float32
    flat = theta(i) if flat is None else flat
    nlflux, reaction = terms_of(i, variant)
    if nlflux is not None:
        nlflux = (nlflux[0].astype(f), nlflux[1])
    if reaction is not None:
        reaction = (reaction[0].astype(f), reaction[1])
    return nlflux_ref.loss_and_grad(np.asarray(flat).astype(f), CASES[i][0], CASES[i][2], nlflux, reaction, dtype, **ref_kw(i, dtype))


@functools.lru_cache(maxsize=None)
def reference64(i, variant='flux'):
    """The fp64 reference of CASES[i], computed once per variant."""
    return reference(i, variant)
