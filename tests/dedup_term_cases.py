"""
Host-side tables of the parity tests of the three nonlinear terms (vn_set_reaction, vn_set_nlflux, vn_set_nldiff) on shared-point
de-duplication maps: the cases, their seeded inputs and maps, the CSR builder and the fp64 / fp32 evaluations of
tests/nldiff_ref.py on the expanded rows Input = Xu[uid].  Plain module (no GPU, no pytest marks), shared by
tests/test_dedup_terms_host.py and tests/test_dedup_terms_gpu.py.

What each case is there for (the branches of vn_terms.hip and of run_dedup / eval_dedup it reaches):

  bench_rand      the bench network on a random map: segments of 1..9 rows (the four-in-flight CSR loop beyond one pass and
                  its tails 1, 2, 3), a plain source below the terms (`base` non-null with each term alone)
  1dt_gauss3      integ_num 36: rows -> (test function, quadrature point) by DIVISION, the feW factor of the three gather
                  kernels, widths 33..64 point kernels, source
  2dt_gauss3_per  integ_num 216 (division, feW) with a PERIODIC gcoef: the integ_num-entry table (`gper`) of
                  vn_nldiff_source_kernel
  3dt             dim 3: pd[1 + d] up to d = 2 and seed_g[j * dim + d]
  3dt_q256        dim 3 at the integ_num limit 256 (one test function per 256-row chunk)
  2d_steady       steady 2D (no dNt term), widths 33..64, source; 260 unique points (with 300 this seed gives no point more than 7
                  rows, and a dim >= 2 case has to have one with 8 or more)
  1d_steady_q6    steady 1D, integ_num 6 (division), feW, periodic table, nT = 462 (nT % 4 == 2: the one-row elementwise
                  kernels on the row-wise side)
  mor6_q8         d_in = 6 > dim + 1 (MOR-shaped inputs), integ_num 8, feW, source
  1dt_q100        integ_num 100 (division; two test functions per chunk, ragged), feW
  3dt_8in         8 inputs, dim 3, source

Map (tests/test_engine_gpu.py::_dedup_parity): default_rng(21), Xu = U(-1, 1), uid = integers(0, U) with every point used,
shuffled; `csr` below turns it into (rowptr, rowidx).  Every case has points with 1, 2, ..., 7 rows and the dim >= 2 cases points
with 8 or more (tests/test_dedup_terms_host.py asserts it).  EMPTY names the cases that additionally get a map in which about 5 %
of the unique points own no row: those points are appended to Xu, and rowptr repeats its last entry there.

Inputs (the scalings of tests/nldiff_cases.py are the starting point; the per-case scales are columns of the table): gcoef =
gscale x N(0,1) (periodic: one [integ_num, dim] table tiled), parameters tscale x (glorot_init(seed 3) + 0.05 N(0,1)), psi =
pscale x N(0,1), phi = N(0,1), rate = U(0.5, 2), N1 = U(0.1, 1) (the term folds divide by N_p), D = (0.7, 0.4, 0.3), F = (0.6,
0.5, -0.3), p = (1, -1, 0.5), detJ = 0.05, weights (3, 2, 5) (steady: (3, 0, 5)).  All rounded to fp32: the engine registers fp32.
That each term alone, and each term left out of 'all', moves every compared quantity by a multiple of its bar is asserted from the
fp64 reference by tests/test_dedup_terms_host.py::test_inputs_make_a_missing_term_fail.  With the starting scales (8, 2, 8) four cases
fell short of it and were changed: bench_rand (D alone moved the least-moved tensor by 0.0026 < 0.01: parameters x 4),
2d_steady (D left out moved bo by 0.00093 < 0.001: fewer unique points changed the draw, now 0.0097), 1d_steady_q6 (the flux left
out moved bo by 6.8e-5: gcoef and psi x 4) and 3dt_8in (D left out moved bo by 0.0008: gcoef x 16, parameters x 3).

Variants: 'all' (D with psi, flux, reaction) and each of 'd', 'psi', 'flux', 'react' alone; 'none' (the oracle) and 'no_d',
'no_psi', 'no_flux', 'no_react' ('all' with one term left out) serve the input condition.
"""
import functools

import numpy as np
import torch

from oracle import tf1_graph as og
from tests import nldiff_ref

DIFF = (0.7, 0.4, 0.3)
FLUX = (0.6, 0.5, -0.3)
COEF = (1.0, -1.0, 0.5)
ONE = (1.0, 0.0, 0.0)
DETJ = 0.05
BIDIMVAL = 2.0

CASES = [
    # d_in dim widths        q    n_k U    nB  bDof source integW td     act        periodic gscale tscale pscale
    (3, 2, [50] * 5,         64,  24, 500, 40, 22,  True,  False, True,  'sigmoid', False,   8.0,   4.0,   8.0),
    (2, 1, [50, 50, 50],     36,  53, 700, 31, 11,  True,  True,  True,  'tanh',    False,   8.0,   2.0,   8.0),
    (3, 2, [20, 20, 20],     216, 7,  410, 20, 9,   False, True,  True,  'sigmoid', True,    8.0,   2.0,   8.0),
    (4, 3, [50] * 4,         64,  21, 333, 40, 22,  False, False, True,  'tanh',    False,   8.0,   2.0,   8.0),
    (4, 3, [20, 30],         256, 7,  600, 12, 6,   False, False, True,  'sigmoid', False,   8.0,   2.0,   8.0),
    (2, 2, [33, 50, 41],     16,  45, 260, 20, 20,  True,  False, False, 'sigmoid', False,   8.0,   2.0,   8.0),
    (1, 1, [20, 20],         6,   77, 200, 2,  2,   False, True,  False, 'tanh',    True,    4.0,   2.0,   4.0),
    (6, 2, [32, 17],         8,   45, 120, 12, 6,   True,  True,  True,  'sigmoid', False,   8.0,   2.0,   8.0),
    (2, 1, [24, 31],         100, 37, 900, 8,  5,   False, True,  True,  'tanh',    False,   8.0,   2.0,   8.0),
    (8, 3, [50] * 4,         64,  21, 333, 40, 22,  True,  False, True,  'sigmoid', False,   16.0,  3.0,   8.0),
]
IDS = ['bench_rand', '1dt_gauss3', '2dt_gauss3_per', '3dt', '3dt_q256', '2d_steady', '1d_steady_q6', 'mor6_q8', '1dt_q100', '3dt_8in']
VARIANTS = ['all', 'd', 'psi', 'flux', 'react']
ALONE = ['d', 'psi', 'flux', 'react']
LEFT_OUT = ['no_d', 'no_psi', 'no_flux', 'no_react']
EMPTY = [1, 3]                      # cases that also get a map with unique points that own no row
PERIODIC = [i for i, c in enumerate(CASES) if c[12]]


def csr(uid, U):
    """(rowptr [U+1], rowidx [nT]) int32 of a row -> point map: the rows of point j are rowidx[rowptr[j]:rowptr[j+1]], in
    increasing order; points beyond the largest uid (or any point no row names) get an empty segment."""
    uid = np.asarray(uid, dtype=np.int64)
    rowptr = np.zeros(U + 1, dtype=np.int64)
    np.add.at(rowptr, uid + 1, 1)
    rowptr = np.cumsum(rowptr)
    fill = rowptr[:-1].copy()
    rowidx = np.empty(uid.size, dtype=np.int32)
    for r, j in enumerate(uid):                   # rows in increasing order land in each segment in increasing order
        rowidx[fill[j]] = r
        fill[j] += 1
    return rowptr.astype(np.int32), rowidx


@functools.lru_cache(maxsize=None)
def inputs(i, n_k=None, q=None):
    """The seeded inputs of CASES[i] as a dict of fp32 arrays: computed once, shared, never modified.  (n_k, q: another number of
    test functions and of quadrature points on the case's network, unique points and BC/IC rows -- tests/source_cases.BIG.)"""
    d_in, dim, widths, q0, n_k0, U, nB, bDof, source, integW, td, act, periodic, gscale, tscale, pscale = CASES[i]
    n_k, q = n_k or n_k0, q or q0
    rng = np.random.default_rng(21)
    n = n_k * q
    Xu = rng.uniform(-1, 1, (U, d_in)).astype(np.float32)
    uid = rng.integers(0, U, n).astype(np.int32)
    uid[:U] = np.arange(U)                                           # every unique point is used
    rng.shuffle(uid)
    if periodic:
        gcoef = np.tile(rng.standard_normal((q, dim)).astype(np.float32), (n_k, 1))
    else:
        gcoef = rng.standard_normal((n, dim)).astype(np.float32)
    d = dict(Xu=Xu, uid=uid, Input=Xu[uid], gcoef=(np.float32(gscale) * gcoef).astype(np.float32),
             source=rng.standard_normal((n, 1)).astype(np.float32) if source else None,
             N1=rng.uniform(0.1, 1, q).astype(np.float32), dNt1=rng.standard_normal(q).astype(np.float32),
             integW=rng.uniform(0.5, 1, (1, q)).astype(np.float32) if integW else None,
             biInput=rng.uniform(-1, 1, (nB, d_in)).astype(np.float32), biLabel=rng.standard_normal((nB, 1)).astype(np.float32),
             w=np.array([3.0, 2.0, 5.0]) if td else np.array([3.0, 0.0, 5.0]))
    d['rowptr'], d['rowidx'] = csr(uid, U)
    d['rate'] = np.random.default_rng(12).uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    d['phi'] = np.random.default_rng(14).standard_normal((n, 1)).astype(np.float32)
    d['psi'] = (np.float32(pscale) * np.random.default_rng(15).standard_normal((n, 1)).astype(np.float32)).astype(np.float32)
    for k, v in d.items():
        if isinstance(v, np.ndarray) and k != 'w':    # (w goes to torch.as_tensor as it is, which wants a writable array)
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def empty_map(i):
    """(Xu, rowptr) of CASES[i] with about 5 % more unique points appended that own no row (uid and rowidx are unchanged)."""
    d = inputs(i)
    U, d_in = d['Xu'].shape
    extra = max(1, (U + 19) // 20)
    Xu = np.concatenate([d['Xu'], np.random.default_rng(22).uniform(-1, 1, (extra, d_in)).astype(np.float32)])
    rowptr = np.concatenate([d['rowptr'], np.full(extra, d['rowptr'][-1], dtype=np.int32)])
    return Xu, rowptr


@functools.lru_cache(maxsize=None)
def theta(i):
    d_in, widths, tscale = CASES[i][0], CASES[i][2], CASES[i][14]
    flat = og.glorot_init(d_in, widths, 3)
    flat = flat + 0.05 * np.random.default_rng(5).standard_normal(flat.size).astype(np.float32)
    return (np.float32(tscale) * flat).astype(np.float32)


def ref_kw(i, dtype=torch.float64, gcoef=None, d=None):
    """Keyword arguments of tests/nldiff_ref.loss_and_grad for CASES[i] on the expanded rows (gcoef: another [nT, dim] array; d:
    another interior data set on the same network, tables and BC/IC rows -- `big_batch`)."""
    d_in, dim, widths, _, n_k, U, nB, bDof, source, integW, td, act = CASES[i][:12]
    d = inputs(i) if d is None else d
    f = np.float64 if dtype == torch.float64 else np.float32
    n, q = d['Input'].shape[0], d['N1'].size
    n_k = n // q
    nb = nB if td else bDof
    return dict(Input=d['Input'].astype(f), gcoef=(d['gcoef'] if gcoef is None else gcoef).astype(f),
                source=None if d['source'] is None else d['source'].astype(f),
                N=np.tile(d['N1'], n_k).reshape(n, 1).astype(f), dNt=np.tile(d['dNt1'], n_k).reshape(n, 1).astype(f),
                integW=None if d['integW'] is None else d['integW'].astype(f), intShape=[n_k, q], detJ=DETJ, detJvec=False,
                biInput=d['biInput'][:nb].astype(f), biLabel=d['biLabel'][:nb].astype(f), bDof=bDof, biDimVal=BIDIMVAL, w=d['w'],
                dim=dim, time_dependent=td, is_source=source, integWflag=integW, activation=act)


def terms_of(i, variant, d=None):
    """(nldiff, nlflux, reaction) of a variant: nldiff = (psi or None, dcoef) or None, nlflux = (phi, fcoef) or None, reaction =
    (rate, coef) or None."""
    d = inputs(i) if d is None else d
    D, P1, Pd = (None, DIFF), (d['psi'], ONE), (d['psi'], DIFF)
    F, R = (d['phi'], FLUX), (d['rate'], COEF)
    return {'all': (Pd, F, R), 'd': (D, None, None), 'psi': (P1, None, None), 'flux': (None, F, None), 'react': (None, None, R),
            'none': (None, None, None), 'no_d': (P1, F, R), 'no_psi': (D, F, R), 'no_flux': (Pd, None, R),
            'no_react': (Pd, F, None)}[variant]


def reference(i, variant, flat=None, dtype=torch.float64, gcoef=None, d=None):
    """tests/nldiff_ref.loss_and_grad on the expanded rows of CASES[i] for a variant."""
    f = np.float64 if dtype == torch.float64 else np.float32
    flat = theta(i) if flat is None else flat
    cast = lambda t: None if t is None else (None if t[0] is None else t[0].astype(f), t[1])
    nldiff, nlflux, reaction = (cast(t) for t in terms_of(i, variant, d))
    return nldiff_ref.loss_and_grad(np.asarray(flat).astype(f), CASES[i][0], CASES[i][2], nldiff, nlflux, reaction, dtype,
                                    **ref_kw(i, dtype, gcoef, d))


@functools.lru_cache(maxsize=None)
def reference64(i, variant='all'):
    """The fp64 reference of CASES[i], computed once per variant."""
    return reference(i, variant)


@functools.lru_cache(maxsize=None)
def big_batch(i, factor=4):
    """A second interior data set for the engine of CASES[i]: `factor` x the test functions and unique points, its own map and
    streams (default_rng(23)); the tables, the BC/IC rows and the weights are the case's (they are the engine's, not a batch's)."""
    d_in, dim, widths, q, n_k, U = CASES[i][:6]
    source, gscale, pscale = CASES[i][8], CASES[i][13], CASES[i][15]
    rng = np.random.default_rng(23)
    n_k, U = factor * n_k, factor * U
    n = n_k * q
    d = dict(inputs(i))
    Xu = rng.uniform(-1, 1, (U, d_in)).astype(np.float32)
    uid = rng.integers(0, U, n).astype(np.int32)
    uid[:U] = np.arange(U)
    rng.shuffle(uid)
    d.update(Xu=Xu, uid=uid, Input=Xu[uid], gcoef=(np.float32(gscale) * rng.standard_normal((n, dim)).astype(np.float32)).astype(np.float32),
             source=rng.standard_normal((n, 1)).astype(np.float32) if source else None,
             rate=rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32), phi=rng.standard_normal((n, 1)).astype(np.float32),
             psi=(np.float32(pscale) * rng.standard_normal((n, 1)).astype(np.float32)).astype(np.float32))
    d['rowptr'], d['rowidx'] = csr(uid, U)
    return d
