"""
Host-side tables of the loss-weight tests (vn_set_tf_weights, vn_set_causal, `VarNet(causal=eps)`): the seven cases of
tests/reaction_cases.py, their slabs, static weights and per-case eps, and the fp64 / fp32 evaluations of tests/causal_ref.py on
them.  Plain module (no GPU, no pytest marks), shared by tests/test_causal_host.py and tests/test_causal_gpu.py.

Inputs: those of tests/reaction_cases.py (synth(seed 11), parameters glorot_init(seed 3) + 0.05 N(0,1)).
Slabs: S = min(n_k, 5), slab = default_rng(21).permutation(arange(n_k) % S): interleaved, as after a shuffle.
Static weights: default_rng(22).uniform(0.2, 1.5, n_k) rounded to fp32 (the engine registers fp32 weights).
eps per case and variant: ln 4 / C_{S-1} of the fp64 reference's own loss field, so the smallest weight is exactly 1/4 there.
Variants: 'plain' (no term), 'terms' (the 'both' variant of tests/nlflux_cases.py -- flux FLUX on phi plus the reaction's rate
stream and COEF -- plus the diffusivity DIFF with psi of tests/nldiff_cases.py).
Modes: 'none' (weights 1: the underlying reference), 'static', 'causal'.
"""
import functools

import numpy as np
import torch

from tests import causal_ref, nldiff_cases, nlflux_cases
from tests.reaction_cases import CASES, IDS, inputs, ref_kw, theta  # noqa: F401  (re-exported)

LN4 = float(np.log(4.0))


def n_slabs(i):
    return min(CASES[i][4], 5)


@functools.lru_cache(maxsize=None)
def slabs(i):
    """slab ids [n_k] int32 of CASES[i]: computed once, shared, never modified."""
    n_k = CASES[i][4]
    return np.random.default_rng(21).permutation(np.arange(n_k) % n_slabs(i)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def static_weights(i):
    return np.random.default_rng(22).uniform(0.2, 1.5, CASES[i][4]).astype(np.float32)


def terms_of(i, variant):
    """(nldiff, nlflux, reaction) of a variant, as tests/nldiff_ref.loss_and_grad takes them."""
    if variant == 'plain':
        return None, None, None
    assert variant == 'terms', variant
    nlflux, reaction = nlflux_cases.terms_of(i, 'both')
    return (nldiff_cases.psi(i), nldiff_cases.DIFF), nlflux, reaction


@functools.lru_cache(maxsize=None)
def eps_of(i, variant='plain'):
    """ln 4 / C_{S-1} from the fp64 reference's loss field: min omega = 1/4 there."""
    lv = reference64(i, 'none', variant)[0]['lossVec'].reshape(-1)
    S = n_slabs(i)
    sl = slabs(i)
    L = np.array([lv[sl == s].mean() if np.any(sl == s) else 0.0 for s in range(S)])
    C = float(np.sum(L[:-1]))
    assert C > 0.0
    return LN4 / C


def weights_of(i, mode, variant='plain', eps=None):
    """(omega, causal) keyword values of causal_ref.loss_and_grad for a mode."""
    if mode == 'none':
        return None, None
    if mode == 'static':
        return static_weights(i), None
    assert mode == 'causal', mode
    return None, (slabs(i), n_slabs(i), eps_of(i, variant) if eps is None else eps)


def reference(i, mode, variant='plain', flat=None, dtype=torch.float64, omega=None, eps=None):
    """tests/causal_ref.loss_and_grad on CASES[i]; omega given: those static weights whatever the mode says."""
    f = np.float64 if dtype == torch.float64 else np.float32
    flat = theta(i) if flat is None else flat
    cast = lambda t: None if t is None else (None if t[0] is None else t[0].astype(f), t[1])
    nldiff, nlflux, reaction = (cast(t) for t in terms_of(i, variant))
    om, causal = (omega, None) if omega is not None else weights_of(i, mode, variant, eps)
    return causal_ref.loss_and_grad(np.asarray(flat).astype(f), CASES[i][0], CASES[i][2], om, causal, nldiff, nlflux, reaction,
                                    dtype, **ref_kw(i, dtype))


@functools.lru_cache(maxsize=None)
def reference64(i, mode='causal', variant='plain'):
    """The fp64 reference of CASES[i], computed once per mode and variant."""
    return reference(i, mode, variant)


def weights_are_real(i, mode, variant='plain'):
    """In the reference: removing the weights moves varLoss and the gradient norm by more than 1e-2 relative."""
    ref, g = reference64(i, mode, variant)
    ref0, g0 = reference64(i, 'none', variant)
    assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss']), (ref['varLoss'], ref0['varLoss'])
    assert np.linalg.norm(g - g0) > 1e-2 * np.linalg.norm(g)
