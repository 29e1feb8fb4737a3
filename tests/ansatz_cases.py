"""
Host-side tables of the hard-constraint-ansatz tests (vn_set_ansatz, vn_set_ansatz_points, vn_set_ansatz_rows): the cases, their
seeded inputs and streams and the fp64 / fp32 evaluations of tests/ansatz_ref.py on them.  Plain module (no GPU, no pytest marks),
shared by tests/test_ansatz_host.py and tests/test_ansatz_gpu.py.

Shapes: the smallest that reach every branch of the elementwise kernels -- (n_k, q) = (1, 4): one thread on the four-row path;
(3, 6): 18 rows on the one-row path; (257, 4): 1028 rows, two blocks, the last one partial -- on the three nets 3x20 tanh,
5x50 sigmoid (the bf16-piece range) and 2x64, with nB in {1, 33, 257} BC/IC rows, one case steady (bDof = nB), and one case
of the two-pass route's own (q = 216).

Inputs: tests/parity_cases.synth(seed 21) with the parameters x 2 and gcoef x GCOEF_SCALE[i] (both exact in fp32).  gcoef x 8 is
what tests/nldiff_cases.py found necessary for a deep net's tangent to matter; on the 2x64 net and the q = 216 case (3, 4) the
tangent of the tanh nets is large as it stands, and at x 8 it drowns A: leaving A out moved the least-moved gradient tensor by
0.5 % and 0.3 % of its size, short of 100 x GRAD_RTOL, so those two keep gcoef x 1 (1.9 % and 1.7 %; B alone: 37 %).
Streams, each rounded to fp32 (the engine registers fp32 rows): A = 0.5 N(0,1), B = U(0.3, 1.7), a, b = N(0,1); that A alone
and B alone (with b) each move every compared quantity by at least 100 x its bar is asserted from the fp64 reference by
tests/test_ansatz_host.py.
"""
import functools

import numpy as np
import torch

from oracle import tf1_graph as og
from tests import ansatz_ref
from tests.dedup_term_cases import csr
from tests.parity_cases import synth

GCOEF_SCALE = [8.0, 8.0, 8.0, 1.0, 1.0]               # per case, see above; the edge and de-duplication inputs: x 8
THETA_SCALE = 2.0
BIDIMVAL = 2.0

CASES = [
    # d_in dim widths        q    n_k  nB   bDof td     act        source integW
    (1, 1, [20, 20, 20],     4,   1,   1,   1,   False, 'tanh',    False, False),   # one thread, four-row path; steady: bDof = nB
    (2, 1, [20, 20, 20],     6,   3,   33,  20,  True,  'tanh',    True,  True),     # 18 rows: one-row path
    (3, 2, [50] * 5,         4,   257, 257, 130, True,  'sigmoid', False, False),   # 1028 rows: two blocks, partial last block
    (3, 2, [64, 64],         4,   257, 33,  20,  True,  'tanh',    False, False),
    (3, 2, [20, 20, 20],     216, 2,   33,  20,  True,  'tanh',    False, True),    # the two-pass route's own
]
IDS = ['1d_steady_1x4', '1dt_3x6', '2dt_50x5_257x4', '2dt_64x2_257x4', '2dt_gauss3']


def stream_set(rng, n, deriv=True):
    """dict(A, B, a, b) of fp32 [n] arrays; deriv False: a set without directions (a = b = None)."""
    z = dict(A=(0.5 * rng.standard_normal(n)).astype(np.float32), B=rng.uniform(0.3, 1.7, n).astype(np.float32), a=None, b=None)
    if deriv:
        z['a'] = rng.standard_normal(n).astype(np.float32)
        z['b'] = rng.standard_normal(n).astype(np.float32)
    return z


@functools.lru_cache(maxsize=None)
def inputs(i):
    """The seeded inputs of CASES[i] with gcoef scaled: computed once, shared, never modified."""
    d_in, dim, widths, q, n_k, nB, bDof, td, act, source, integW = CASES[i]
    d = synth(21, d_in, dim, widths, q, n_k, nB, bDof, source, integW, False)
    d['gcoef'] = (np.float32(GCOEF_SCALE[i]) * d['gcoef']).astype(np.float32)
    return d


@functools.lru_cache(maxsize=None)
def theta(i):
    d_in, widths = CASES[i][0], CASES[i][2]
    flat = og.glorot_init(d_in, widths, 3)
    flat = flat + 0.05 * np.random.default_rng(5).standard_normal(flat.size).astype(np.float32)
    return (np.float32(THETA_SCALE) * flat).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ansatz(i):
    """dict(int=streams, bic=streams) of CASES[i]: computed once, shared, never modified."""
    q, n_k, nB = CASES[i][3], CASES[i][4], CASES[i][5]
    rng = np.random.default_rng(22)
    return dict(int=stream_set(rng, n_k * q), bic=stream_set(rng, nB, deriv=False))


def ref_kw(i, dtype=torch.float64):
    d_in, dim, widths, q, n_k, nB, bDof, td, act, source, integW = CASES[i]
    d = inputs(i)
    f = np.float64 if dtype == torch.float64 else np.float32
    nb = nB if td else bDof
    return dict(Input=d['Input'].astype(f), gcoef=d['gcoef'].astype(f), source=None if d['source'] is None else d['source'].astype(f),
                N=d['N'].astype(f), dNt=d['dNt'].astype(f), integW=None if d['integW'] is None else d['integW'].astype(f),
                intShape=[n_k, q], detJ=float(d['detJ']), detJvec=False, biInput=d['biInput'][:nb].astype(f),
                biLabel=d['biLabel'][:nb].astype(f), bDof=bDof, biDimVal=BIDIMVAL, w=d['w'], dim=dim, time_dependent=td,
                is_source=source, integWflag=integW, activation=act)


def cast(z, f):
    """A stream set (or a dict of them) in the float type f."""
    if z is None:
        return None
    if 'B' not in z:
        return {k: cast(v, f) for k, v in z.items()}
    return {k: (None if v is None else np.asarray(v).astype(f)) for k, v in z.items()}


def reference(i, az='default', flat=None, dtype=torch.float64, w=None, **sets):
    """tests/ansatz_ref.loss_and_grad on CASES[i]; az: the ansatz dict ('default': ansatz(i); None: the bare network);
    sets: nldiff / nlflux / reaction / flux / periodic / obs of that function; w: other loss weights."""
    f = np.float64 if dtype == torch.float64 else np.float32
    flat = theta(i) if flat is None else flat
    az = ansatz(i) if isinstance(az, str) else az
    kw = ref_kw(i, dtype)
    if az is not None and az.get('bic') is not None:
        nb = kw['biInput'].shape[0]                       # a steady problem keeps the first bDof rows
        az = dict(az, bic={k: (None if v is None else v[:nb]) for k, v in az['bic'].items()})
    if w is not None:
        kw['w'] = np.asarray(w, dtype=float)
    return ansatz_ref.loss_and_grad(np.asarray(flat).astype(f), CASES[i][0], CASES[i][2], cast(az, f), dtype=dtype, **kw, **sets)


@functools.lru_cache(maxsize=None)
def reference64(i):
    """The fp64 reference of CASES[i] with its default ansatz, computed once."""
    return reference(i)


# ---- the edge sets ------------------------------------------------------------------------------------------------------
EDGE_ROWS = [1, 33, 257, 600]
EDGE_KINDS = ['flux', 'periodic_g0', 'periodic_g1', 'obs_values', 'obs_dirs_rowptr']
EDGE_CASE = 1                                            # the 1D+t tanh net


@functools.lru_cache(maxsize=None)
def edge(kind, rows):
    """(name of the set, its registration dict for tests/ansatz_ref.loss_and_grad, its stream set) on the net of
    CASES[EDGE_CASE]: `rows` flux rows, pairs (2 rows each) or observed points."""
    d_in, dim = CASES[EDGE_CASE][0], CASES[EDGE_CASE][1]
    rng = np.random.default_rng(23 + rows)
    unit = lambda n: (lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))(rng.standard_normal((n, dim)))
    if kind == 'flux':
        reg = dict(X=rng.uniform(-1, 1, (rows, d_in)).astype(np.float32), normal=unit(rows),
                   coef=rng.uniform(0.5, 1.5, rows).astype(np.float32), label=rng.standard_normal(rows).astype(np.float32))
        return 'flux', reg, stream_set(rng, rows)
    if kind.startswith('periodic'):
        gamma = 1.0 if kind.endswith('g1') else 0.0
        X = rng.uniform(-1, 1, (2 * rows, d_in)).astype(np.float32)
        dirs = np.tile(unit(rows), (2, 1))
        return 'periodic', dict(X=X, dir=dirs, gamma=gamma), stream_set(rng, 2 * rows, deriv=gamma > 0)
    if kind == 'obs_values':
        reg = dict(X=rng.uniform(-1, 1, (rows, d_in)).astype(np.float32), value=rng.standard_normal(rows).astype(np.float32), lam=1.5)
        return 'obs', reg, stream_set(rng, rows, deriv=False)
    # observations with directions, quadrature weights and segments of 1..3 points
    seg = rng.integers(1, 4, rows)
    n = int(seg.sum())
    reg = dict(X=rng.uniform(-1, 1, (n, d_in)).astype(np.float32), value=rng.standard_normal(rows).astype(np.float32), lam=1.5,
               q=rng.uniform(0.2, 1.0, n).astype(np.float32), dir=unit(n), rowptr=np.concatenate([[0], np.cumsum(seg)]).astype(np.int32),
               wgt=rng.uniform(0.5, 2.0, rows).astype(np.float32))
    return 'obs', reg, stream_set(rng, n)


# ---- de-duplication maps ------------------------------------------------------------------------------------------------
DEDUP = [
    # U    dim d_in widths        q   n_k  act
    (1,    1,  2,   [20, 20, 20], 16, 3,   'tanh'),
    (255,  2,  3,   [50] * 5,     16, 20,  'sigmoid'),
    (256,  3,  4,   [20, 20, 20], 16, 20,  'tanh'),
    (257,  2,  3,   [64, 64],     16, 20,  'tanh'),
]
DEDUP_IDS = ['U1_dim1', 'U255_dim2', 'U256_dim3', 'U257_dim2']
DEDUP_NB, DEDUP_BDOF, DEDUP_DETJ = 33, 20, 0.05


@functools.lru_cache(maxsize=None)
def dedup_inputs(j):
    """Inputs, map and streams of DEDUP[j]: a random map in which about one point in eight owns no row (U > 1); the point streams
    (A, B, grad A, grad B) at Xu, and the row streams the same map induces: A_r = A[uid], a_r = grad A[uid] . gcoef_r (formed in
    fp64 from the fp32 operands; `rows32` holds them rounded to fp32 for a row-wise registration)."""
    U, dim, d_in, widths, q, n_k, act = DEDUP[j]
    rng = np.random.default_rng(31 + j)
    n = n_k * q
    used = np.arange(U) if U == 1 else np.flatnonzero(rng.random(U) > 0.125)
    uid = used[rng.integers(0, used.size, n)].astype(np.int32)
    Xu = rng.uniform(-1, 1, (U, d_in)).astype(np.float32)
    gcoef = (np.float32(8.0) * rng.standard_normal((n, dim)).astype(np.float32)).astype(np.float32)
    d = dict(Xu=Xu, uid=uid, U=U, Input=Xu[uid], gcoef=gcoef, N1=rng.uniform(0.1, 1, q).astype(np.float32),
             dNt1=rng.standard_normal(q).astype(np.float32), biInput=rng.uniform(-1, 1, (DEDUP_NB, d_in)).astype(np.float32),
             biLabel=rng.standard_normal((DEDUP_NB, 1)).astype(np.float32), w=np.array([3.0, 2.0, 5.0]), n_k=n_k,
             empty=int(U - np.unique(uid).size))
    d['rowptr'], d['rowidx'] = csr(uid, U)
    pts = dict(A=(0.5 * rng.standard_normal(U)).astype(np.float32), B=rng.uniform(0.3, 1.7, U).astype(np.float32),
               gA=rng.standard_normal((U, dim)).astype(np.float32), gB=rng.standard_normal((U, dim)).astype(np.float32))
    g64 = gcoef.astype(np.float64)
    rows = dict(A=pts['A'][uid].astype(np.float64), B=pts['B'][uid].astype(np.float64),
                a=(pts['gA'][uid].astype(np.float64) * g64).sum(axis=1), b=(pts['gB'][uid].astype(np.float64) * g64).sum(axis=1))
    d['pts'], d['rows'] = pts, rows
    d['rows32'] = {k: v.astype(np.float32) for k, v in rows.items()}
    d['bic'] = stream_set(rng, DEDUP_NB, deriv=False)
    flat = og.glorot_init(d_in, widths, 3)
    flat = flat + 0.05 * np.random.default_rng(5).standard_normal(flat.size).astype(np.float32)
    d['theta'] = (np.float32(THETA_SCALE) * flat).astype(np.float32)
    return d


def dedup_reference(j, dtype=torch.float64):
    """tests/ansatz_ref.loss_and_grad of DEDUP[j] on the expanded rows Input = Xu[uid]."""
    U, dim, d_in, widths, q, n_k, act = DEDUP[j]
    d = dedup_inputs(j)
    f = np.float64 if dtype == torch.float64 else np.float32
    n = n_k * q
    kw = dict(Input=d['Input'].astype(f), gcoef=d['gcoef'].astype(f), source=None, N=np.tile(d['N1'], n_k).reshape(n, 1).astype(f),
              dNt=np.tile(d['dNt1'], n_k).reshape(n, 1).astype(f), integW=None, intShape=[n_k, q], detJ=DEDUP_DETJ, detJvec=False,
              biInput=d['biInput'].astype(f), biLabel=d['biLabel'].astype(f), bDof=DEDUP_BDOF, biDimVal=BIDIMVAL, w=d['w'], dim=dim,
              time_dependent=True, is_source=False, integWflag=False, activation=act)
    az = cast(dict(int=d['rows'], bic=d['bic']), f)
    return ansatz_ref.loss_and_grad(d['theta'].astype(f), d_in, widths, az, dtype=dtype, **kw)
