"""
Host-side tables of the reaction-term tests (vn_set_reaction, `ADPDE(reaction=...)`): the cases, their seeded inputs and the
fp64 / fp32 evaluations of tests/reaction_ref.py on them.  Plain module (no GPU, no pytest marks), shared by
tests/test_reaction_host.py and tests/test_reaction_gpu.py.

Inputs: tests/parity_cases.synth(seed 11), rate = default_rng(12).uniform(0.5, 2, (nT, 1)) rounded to fp32 (the engine
registers fp32 rows), coefficients (1, -1, 0.5), parameters glorot_init(seed 3) + 0.05 N(0,1) (default_rng(5)) in fp32.
"""
import functools

import numpy as np
import torch

from oracle import tf1_graph as og
from tests import reaction_ref
from tests.parity_cases import synth

COEF = (1.0, -1.0, 0.5)

CASES = [
    # d_in dim widths          integNum n_k  nB  bDof td     act        source integW detJvec per-row tables
    (1, 1, [20],               4,       300, 1,  1,   False, 'sigmoid', False, False, False,  False),   # crosses a 256-test-function seed block; no dNt term
    (2, 1, [20],               16,      40,  50, 30,  True,  'tanh',    False, False, False,  False),
    (3, 2, [10, 20],           64,      5,   33, 20,  True,  'sigmoid', True,  False, True,   False),   # source + detJ vector + rate stream
    (3, 2, [50] * 5,           64,      9,   77, 40,  True,  'sigmoid', False, False, False,  False),   # the bench network
    (3, 2, [64, 64],           216,     3,   5,  2,   True,  'tanh',    False, True,  False,  False),   # two-pass already
    (3, 2, [128, 128],         64,      5,   33, 20,  True,  'sigmoid', False, False, False,  False),   # layer by layer
    (2, 1, [20],               16,      40,  50, 30,  True,  'tanh',    False, False, False,  True),    # case 2 with N_rows / dNt_rows
]
IDS = ['1d_steady_300', '1dt_tanh', '2dt_src_detJv', '2dt_50x5', '2dt_gauss3', '2dt_128x2', '1dt_tanh_rows']


@functools.lru_cache(maxsize=None)
def inputs(i):
    """(inputs dict, rate [nT,1] fp32) of CASES[i]: computed once, shared, never modified."""
    d_in, dim, widths, q, n_k, nB, bDof, td, act, source, integW, detJvec, rows = CASES[i]
    d = synth(11, d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec)
    n = n_k * q
    rate = np.random.default_rng(12).uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    d['N_rows'] = d['dNt_rows'] = None
    if rows:
        rng = np.random.default_rng(13)
        d['N_rows'] = rng.uniform(0, 1, (n, 1)).astype(np.float32)
        d['dNt_rows'] = rng.standard_normal((n, 1)).astype(np.float32)
        d['N'], d['dNt'] = d['N_rows'], d['dNt_rows']
    return d, rate


@functools.lru_cache(maxsize=None)
def theta(i):
    d_in, widths = CASES[i][0], CASES[i][2]
    flat = og.glorot_init(d_in, widths, 3)
    return flat + 0.05 * np.random.default_rng(5).standard_normal(flat.size).astype(np.float32)


def ref_kw(i, dtype=torch.float64, d=None):
    d_in, dim, widths, q, n_k, nB, bDof, td, act, source, integW, detJvec, rows = CASES[i]
    d = inputs(i)[0] if d is None else d
    f = np.float64 if dtype == torch.float64 else np.float32
    nb = nB if td else bDof
    return dict(Input=d['Input'].astype(f), gcoef=d['gcoef'].astype(f),
                source=None if d['source'] is None else d['source'].astype(f), N=d['N'].astype(f), dNt=d['dNt'].astype(f),
                integW=None if d['integW'] is None else d['integW'].astype(f), intShape=[n_k, q],
                detJ=(d['detJ'].astype(f) if detJvec else float(d['detJ'])), detJvec=detJvec,
                biInput=d['biInput'][:nb].astype(f), biLabel=d['biLabel'][:nb].astype(f), bDof=bDof, biDimVal=2.0, w=d['w'],
                dim=dim, time_dependent=td, is_source=source, integWflag=integW, activation=act)


def reference(i, reaction, flat=None, dtype=torch.float64):
    """tests/reaction_ref.loss_and_grad on CASES[i]; reaction = (rate or None, coef) or None (the oracle itself)."""
    f = np.float64 if dtype == torch.float64 else np.float32
    flat = theta(i) if flat is None else flat
    if reaction is not None and reaction[0] is not None:
        reaction = (np.asarray(reaction[0]).astype(f), reaction[1])
    return reaction_ref.loss_and_grad(np.asarray(flat).astype(f), CASES[i][0], CASES[i][2], reaction, dtype, **ref_kw(i, dtype))


@functools.lru_cache(maxsize=None)
def reference64(i, variant='rate'):
    """The fp64 reference of CASES[i], computed once per variant: 'rate' (rate stream, COEF), 'unit' (rate = 1, COEF),
    'linear' ((0.7, 0, 0) with the rate stream), 'none' (no reaction)."""
    return reference(i, reaction_of(i, variant))


def reaction_of(i, variant):
    rate = inputs(i)[1]
    return {'rate': (rate, COEF), 'unit': (None, COEF), 'linear': (rate, (0.7, 0.0, 0.0)), 'none': None}[variant]
