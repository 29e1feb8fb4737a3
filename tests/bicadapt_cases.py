"""
Host-side tables of the tests of the weights on the Dirichlet and initial rows (vn_set_bic_weights, vn_set_bic_adapt,
`VarNet(bicWeights=..., bicAdapt=...)`): the networks and the (nB, bDof) the issue names, their seeded inputs, parameters and
initial states, and the fp64 restatement (tests/bicadapt_ref.py) evaluated on them.

    case            net            d_in  q    n_k  (nB, bDof)          why
    n50_30          [20]           2     16   40   (50, 30)
    n33_21          3 x 20         3     64   9    (33, 21)            both parts odd, neither a multiple of 4
    n77_40          5 x 50         3     64   9    (77, 40)
    n5_4            [20]           2     16   11   (5, 4)              an initial part of one row
    steady40        3 x 20         3     16   20   (40, 40)            steady engine: no initial part
    n300_257        3 x 20         3     64   5    (300, 257)          two 256-row loss-partial blocks, one row in the second
    twopass33_21    3 x 20         3     216  5    (33, 21)            integNum 216: the two-pass sequence
    big             [20]           2     16   8    (262 294, 262 244)  bc part past 262 144 rows: the section-34 kernels' 256
                                                                       blocks of 1024 are all in use and every thread strides

Sigmoid networks (oracle/tangent_ref.py, which the restatement extends, states the sigmoid).  Inputs: tests/parity_cases.synth
(seed 11); parameters: glorot_init(seed 3) + 0.05 N(0, 1) (default_rng(5)); initial state per part:
default_rng(31 + part).uniform(0.5, 2, n_s) rounded to fp32, registered WITHOUT normalisation in the weights-in-use tests so
that the weights are real (`weights_are_real`).

The single-update bar is tests/adapt_cases.single_update_bar: the rules are the same functions.  Plain module (no GPU, no pytest
marks), shared by tests/test_bicadapt_host.py and tests/test_bicadapt_gpu.py.
"""
import functools

import numpy as np

from oracle import tf1_graph as og
from tests import adapt_ref, bicadapt_ref
from tests.parity_cases import synth

BIDIMVAL = 2.0
BIG_BC = 262144 + 100
#        name            d_in dim widths            q    n_k nB            bDof    td
CASES = [
    ('n50_30',       2, 1, [20],                16,  40, 50,           30,     True),
    ('n33_21',       3, 2, [20, 20, 20],        64,  9,  33,           21,     True),
    ('n77_40',       3, 2, [50, 50, 50, 50, 50], 64, 9,  77,           40,     True),
    ('n5_4',         2, 1, [20],                16,  11, 5,            4,      True),
    ('steady40',     3, 2, [20, 20, 20],        16,  20, 40,           40,     False),
    ('n300_257',     3, 2, [20, 20, 20],        64,  5,  300,          257,    True),
    ('twopass33_21', 3, 2, [20, 20, 20],        216, 5,  33,           21,     True),
    ('big',          2, 1, [20],                16,  8,  BIG_BC + 50,  BIG_BC, True),
]
IDS = [c[0] for c in CASES]
IDX = {name: i for i, name in enumerate(IDS)}
BIG = IDX['big']
SMALL = [i for i in range(len(CASES)) if i != BIG]
RULES = ('rba', 'sa')
assert BIG_BC > 256 * 1024                   # VN_ADAPT_MAX_BLOCKS * VN_ADAPT_SPAN of varnet_amd/csrc/vn_adapt.h


def rows(i):
    """(rows of bc, rows of ic) of CASES[i] as the engine counts them."""
    c = CASES[i]
    return bicadapt_ref.part_rows(c[6], c[7], c[8])


def parts_of(i):
    return [s for s in (0, 1) if rows(i)[s] > 0]


@functools.lru_cache(maxsize=None)
def inputs(i):
    """The inputs dict of CASES[i]: computed once, shared, never modified."""
    name, d_in, dim, widths, q, n_k, nB, bDof, td = CASES[i]
    return synth(11, d_in, dim, widths, q, n_k, nB, bDof)


@functools.lru_cache(maxsize=None)
def theta(i):
    name, d_in, dim, widths = CASES[i][:4]
    flat = og.glorot_init(d_in, widths, 3)
    return (flat + 0.05 * np.random.default_rng(5).standard_normal(flat.size).astype(np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def lambda0(i, part):
    return np.random.default_rng(31 + part).uniform(0.5, 2.0, rows(i)[part]).astype(np.float32)


def omega_rows(i, per_part):
    """{part: omega of the part} -> one weight per row the reference counts (a part that is not given: 1)."""
    n = rows(i)
    return np.concatenate([np.asarray(per_part.get(s, np.ones(n[s])), dtype=np.float64).reshape(-1) for s in (0, 1)])


def reference(i, omega=None, flat=None, dtype=np.float64, label=None):
    """tests/bicadapt_ref.loss_and_grad on CASES[i]; omega: one weight per row the engine counts (None: 1)."""
    name, d_in, dim, widths, q, n_k, nB, bDof, td = CASES[i]
    d = inputs(i)
    f = dtype
    nb = nB if td else bDof
    flat = theta(i) if flat is None else flat
    lab = d['biLabel'] if label is None else label
    return bicadapt_ref.loss_and_grad(np.asarray(flat).astype(f), d_in, widths, dim, d['Input'].astype(f), d['gcoef'].astype(f), None,
                                      d['N'].astype(f), d['dNt'].astype(f), None, n_k, q, f(d['detJ']), d['biInput'][:nb].astype(f),
                                      np.asarray(lab)[:nb].astype(f), bDof, f(BIDIMVAL), d['w'].astype(f), td,
                                      None if omega is None else np.asarray(omega, dtype=f))


def parity_spec(rule='rba', **kw):
    """The registration of the weights-in-use tests: no normalisation, omega = lambda^2."""
    kw.setdefault('normalize', False)
    return adapt_ref.spec_of(rule, **kw)


@functools.lru_cache(maxsize=None)
def reference64(i, weighted=True):
    om = omega_rows(i, {s: lambda0(i, s).astype(np.float64) ** 2 for s in parts_of(i)}) if weighted else None
    return reference(i, om)


def weights_are_real(i):
    """In the reference: removing the weights moves BC (and IC, where the part exists) and the gradient by more than 1e-2."""
    ref, g = reference64(i, True)
    ref0, g0 = reference64(i, False)
    assert abs(ref['BCloss'] - ref0['BCloss']) > 1e-2 * abs(ref['BCloss'])
    if rows(i)[1] > 0:
        assert abs(ref['ICloss'] - ref0['ICloss']) > 1e-2 * abs(ref['ICloss'])
    assert np.linalg.norm(g - g0) > 1e-2 * np.linalg.norm(g)
