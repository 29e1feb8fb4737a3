"""
Host-side tables of the parity tests of the de-duplicated step on heavily shared and skewed point maps: seeded map generators
returning (uid, U), the cases built on them, their inputs and the fp64 / fp32 oracle on the expanded rows Input = Xu[uid].  Plain
module (no GPU, no pytest marks), shared by tests/test_dedup_maps_host.py and tests/test_dedup_maps_gpu.py; the CSR builder is
tests/dedup_term_cases.csr.

vn_dedup_gather_kernel gives a workgroup PB = VN_GATHER_PB consecutive unique points and walks their CSR entries through an LDS
buffer of CH = VN_GATHER_CH entries; csr_walk (vn_terms.hip) walks the rows of one point four at a time.  Both constants are read
out of the text of vn_dedup.hip, so a change of either in the kernel moves the constructed cases (chunk_edges) or fails
tests/test_dedup_maps_host.py.  The unit below is the number of CSR entries one PB-point block owns; every other map of the suite
stays at or below CH (asserted by the host module), i.e. never enters the chunk loop a second time.

What each map is there for:

  grid_3dt        uniform tensor grid, 3 space axes + time, two-point Gauss, from geometry alone: 4 interior nodes per axis, 256
                  test functions of integ_num 256, 65 536 rows on 10 000 points; interior points own 2^4 = 16 rows; blocks of one
                  and of two chunks (largest 2768 entries); periodic gcoef (constant coefficients): table path against the
                  CSR-ordered copy at base > 0
  grid_3dt_small  the same geometry with 3 nodes per axis: 20 736 rows, 4096 points, largest block 1728 -- the control, one chunk
  hot_point       7680 rows on 300 points, 70 % of them on one: a segment longer than two whole chunks, a block of four chunks
  single_point    U = 1: one thread adds 7680 entries across four chunks, nj = 1
  dense           40 points of about 192 rows: one block of four chunks, every chunk boundary cuts a segment; periodic gcoef
  edge_ch, edge_ch1, edge_2ch
                  block 0 owns exactly CH, CH + 1 and 2 CH entries: n == CH, a one-entry last chunk, a full last chunk
  edge_between    block 0 owns CH + 700 entries and a segment ends exactly at CH: the empty clip hi == lo on the second pass
  empty_blocks    700 points: block 1 (points 256..511) owns no row at all (e0 == e1) between two populated blocks, and the first
                  and last point of blocks 0 and 2 are empty
  long_tails      segments of 16, 17, 18 and 19 rows among 1..9: csr_walk beyond two passes with tails 1, 2 and 3

Inputs: Xu = U(-1, 1), gcoef = N(0,1) (periodic: one [integ_num, dim] table tiled), N1 = U(0.1, 1) (the term folds divide by
N_p), parameters = glorot_init(seed 3) (= the engine's init_params(3), bit for bit) + 0.05 N(0,1), detJ = 0.05, weights (3, 2, 5).
The three nonlinear terms together ('all' of tests/dedup_term_cases.py) run on TERM_CASES with gcoef x 8, psi x 8, and that
module's bench_rand parameter scale x 4 and phi x 8: with its common scales (parameters x 2, phi = N(0,1)) leaving the flux out
moved the least-moved gradient tensor of grid_3dt by 1.8e-4 of its size and leaving D out that of hot_point by 8.2e-4, short of the
10 x GRAD_RTOL that tests/test_dedup_maps_host.py asks; now the least-moved tensor moves by 1.2e-2 or more.

SWEEP: 12 seeded random maps, integ_num from {16, 36, 64, 256}, mean rows per point 1..40, odd seeds with Zipf-distributed shares,
at most 20 000 rows.  SWEEP_SEEDS is a constant list: a seed the host test finds ill-conditioned (the fp32 oracle deviating from
the fp64 one by more than a tenth of the bars) is replaced there by the next one, never skipped at run time.
"""
import functools
import os
import re

import numpy as np
import torch

from oracle import tf1_graph as og
from tests import nldiff_ref
from tests.dedup_term_cases import COEF, DIFF, FLUX, ONE, csr

DETJ = 0.05
BIDIMVAL = 2.0
NB, BDOF = 30, 14
TERM_SCALES = (8.0, 4.0, 8.0, 8.0)                  # gcoef, parameters, psi, phi of the terms run


def gather_constants():
    """(VN_GATHER_PB, VN_GATHER_CH) as vn_dedup.hip defines them."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'varnet_amd', 'csrc', 'vn_dedup.hip')
    with open(path) as f:
        text = f.read()
    out = []
    for name in ('VN_GATHER_PB', 'VN_GATHER_CH'):
        m = re.findall(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, text)
        assert len(m) == 1, '%s: expected one definition in vn_dedup.hip, found %d' % (name, len(m))
        out.append(int(m[0]))
    return tuple(out)


PB, CH = gather_constants()


# ---- the maps: (uid [nT] int32, U) --------------------------------------------------------------------------------------
def grid_map(nodes, axes=4):
    """Row -> point map of a uniform tensor grid from geometry alone: per axis `nodes` interior nodes carry hat functions over
    nodes + 1 elements with two Gauss points each; the hat of node i spans elements i and i + 1, i.e. the points 2 i .. 2 i + 3 of
    the axis.  Test functions and the quadrature points inside one are numbered lexicographically over the axes (row = k *
    integ_num + p), and so are the unique points (2 (nodes + 1) per axis)."""
    pts = 2 * (nodes + 1)
    k = np.stack(np.meshgrid(*[np.arange(nodes)] * axes, indexing='ij'), -1).reshape(-1, 1, axes)       # node index per axis
    p = np.stack(np.meshgrid(*[np.arange(4)] * axes, indexing='ij'), -1).reshape(1, -1, axes)           # local point per axis
    g = 2 * k + p                                                                                       # [n_k, 4^axes, axes]
    uid = np.zeros(g.shape[:2], dtype=np.int64)
    for a in range(axes):
        uid = uid * pts + g[..., a]
    return uid.reshape(-1).astype(np.int32), pts ** axes


def counts_map(counts, rng):
    """A map in which point j owns counts[j] rows, the rows assigned at random."""
    uid = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    rng.shuffle(uid)
    return uid, len(counts)


def split(total, parts, rng):
    """`parts` positive integers that add up to `total`."""
    assert total >= parts
    return 1 + rng.multinomial(total - parts, np.full(parts, 1.0 / parts))


def hot_point_map(n, U, rng, share=0.7):
    hot = int(rng.integers(0, min(U, PB)))
    uid = np.where(rng.random(n) < share, hot, rng.integers(0, U, n)).astype(np.int32)
    uid[:U] = np.arange(U)                                           # every unique point is used
    rng.shuffle(uid)
    return uid, U


def dense_map(n, U, rng):
    uid = rng.integers(0, U, n).astype(np.int32)
    uid[:U] = np.arange(U)
    rng.shuffle(uid)
    return uid, U


def edge_map(n, block0, rng, cut=None):
    """Block 0 (PB points, none empty) owns exactly `block0` entries, 100 points of block 1 the other n - block0; with `cut`, the
    first 128 points of block 0 own exactly `cut` entries (a segment ends at entry `cut`)."""
    if cut is None:
        c0 = split(block0, PB, rng)
    else:
        c0 = np.concatenate([split(cut, PB // 2, rng), split(block0 - cut, PB - PB // 2, rng)])
    return counts_map(np.concatenate([c0, split(n - block0, 100, rng)]), rng)


def empty_blocks_map(n, rng):
    """700 points in three blocks: block 1 all empty, blocks 0 and 2 populated but for their first and last point."""
    U = 2 * PB + 188
    counts = np.zeros(U, dtype=np.int64)
    n0 = n // 2
    counts[1:PB - 1] = split(n0, PB - 2, rng)
    counts[2 * PB + 1:U - 1] = split(n - n0, U - 2 * PB - 2, rng)
    return counts_map(counts, rng)


def long_tails_map(q, rng):
    """Three points each of 16, 17, 18 and 19 rows among 200 of 1..9, padded with one-row points to whole test functions."""
    counts = np.concatenate([np.repeat([16, 17, 18, 19], 3), rng.integers(1, 10, 200)])
    counts = np.concatenate([counts, np.ones(-int(counts.sum()) % q, dtype=np.int64)])
    rng.shuffle(counts)
    return counts_map(counts, rng)


@functools.lru_cache(maxsize=None)
def sweep_map(seed):
    """(q, uid, U) of one draw of the sweep."""
    rng = np.random.default_rng(7000 + seed)
    q = int(rng.choice([16, 36, 64, 256]))
    n_k = int(rng.integers(max(1, 4000 // q), 20000 // q + 1))
    n = n_k * q
    U = max(1, n // int(rng.integers(1, 41)))
    if seed % 2:                                                     # Zipf-distributed shares: a few points own most rows
        w = 1.0 / np.arange(1, U + 1) ** 1.1
        uid = rng.permutation(U)[rng.choice(U, n, p=w / w.sum())].astype(np.int32)
    else:
        uid = rng.integers(0, U, n).astype(np.int32)
    uid[:U] = np.arange(U)
    rng.shuffle(uid)
    return q, uid, U


# ---- the cases ----------------------------------------------------------------------------------------------------------
NET256 = (4, 3, [20, 30])
NETS = [(3, 2, [50] * 4), (3, 2, [33, 50, 41]), (2, 1, [20, 20])]
Q, NK = 64, 120                                                      # 7680 rows

CASES = {
    # name:           d_in dim widths   q    act        source integW periodic seed  map(rng)
    'grid_3dt':       (*NET256,         256, 'sigmoid', False, False, True,    31,   lambda rng: grid_map(4)),
    'grid_3dt_small': (*NET256,         256, 'sigmoid',  False, False, True,    32,   lambda rng: grid_map(3)),
    'hot_point':      (*NETS[0],        Q,   'sigmoid', True,  False, False,   33,   lambda rng: hot_point_map(Q * NK, 300, rng)),
    'single_point':   (*NETS[2],        Q,   'tanh',    False, True,  False,   34,   lambda rng: (np.zeros(Q * NK, dtype=np.int32), 1)),
    'dense':          (*NETS[1],        Q,   'sigmoid', False, True,  True,    35,   lambda rng: dense_map(Q * NK, 40, rng)),
    'edge_ch':        (*NETS[2],        Q,   'sigmoid', False, False, False,   36,   lambda rng: edge_map(Q * 60, CH, rng)),
    'edge_ch1':       (*NETS[2],        Q,   'tanh',    True,  False, False,   37,   lambda rng: edge_map(Q * 60, CH + 1, rng)),
    'edge_2ch':       (*NETS[2],        Q,   'sigmoid', False, True,  False,   38,   lambda rng: edge_map(Q * 100, 2 * CH, rng)),
    'edge_between':   (*NETS[2],        Q,   'tanh',    False, False, False,   39,   lambda rng: edge_map(Q * 60, CH + 700, rng, cut=CH)),
    'empty_blocks':   (*NETS[1],        36,  'tanh',    True,  True,  False,   40,   lambda rng: empty_blocks_map(36 * 90, rng)),
    'long_tails':     (*NETS[0],        16,  'tanh',    True,  False, False,   41,   lambda rng: long_tails_map(16, rng)),
}
IDS = list(CASES)
CONTROL = 'grid_3dt_small'
PERIODIC = [k for k, c in CASES.items() if c[7]]
BITWISE = ['grid_3dt', 'dense']                     # the table path against the CSR-ordered copy
TERM_CASES = ['grid_3dt', 'hot_point', 'long_tails']
SWEEP_SEEDS = list(range(12))
SWEEP_IDS = ['sweep%d' % s for s in SWEEP_SEEDS]


def config(name):
    """(d_in, dim, widths, q, act, source, integW, periodic, seed, map function) of a case or of a sweep draw ('sweep<seed>')."""
    if name in CASES:
        return CASES[name]
    seed = int(name[len('sweep'):])
    q, uid, U = sweep_map(seed)
    net = NET256 if q == 256 else NETS[seed % 3]
    return (*net, q, 'tanh' if seed % 4 >= 2 else 'sigmoid', seed % 3 == 0, q == 36 or seed % 5 == 0, seed % 6 == 1, 100 + seed,
            lambda rng: (uid, U))


def net_of(name):
    """(d_in, dim, widths, td) of a case: what the per-block gradient rule needs."""
    c = config(name)
    return c[0], c[1], c[2], True


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The seeded inputs of a case as a dict of fp32 arrays (and its map): computed once, shared, never modified."""
    d_in, dim, widths, q, act, source, integW, periodic, seed, mapfn = config(name)
    rng = np.random.default_rng(seed)
    uid, U = mapfn(rng)
    n = uid.size
    n_k = n // q
    assert n_k * q == n
    Xu = rng.uniform(-1, 1, (U, d_in)).astype(np.float32)
    if periodic:
        gcoef = np.tile(rng.standard_normal((q, dim)).astype(np.float32), (n_k, 1))
    else:
        gcoef = rng.standard_normal((n, dim)).astype(np.float32)
    d = dict(Xu=Xu, uid=uid, Input=Xu[uid], gcoef=gcoef, source=rng.standard_normal((n, 1)).astype(np.float32) if source else None,
             N1=rng.uniform(0.1, 1, q).astype(np.float32), dNt1=rng.standard_normal(q).astype(np.float32),
             integW=rng.uniform(0.5, 1, (1, q)).astype(np.float32) if integW else None,
             biInput=rng.uniform(-1, 1, (NB, d_in)).astype(np.float32), biLabel=rng.standard_normal((NB, 1)).astype(np.float32),
             rate=rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32), phi=(np.float32(TERM_SCALES[3]) * rng.standard_normal((n, 1)).astype(np.float32)).astype(np.float32),
             psi=(np.float32(TERM_SCALES[2]) * rng.standard_normal((n, 1)).astype(np.float32)).astype(np.float32),
             w=np.array([3.0, 2.0, 5.0]), bDof=BDOF, n_k=n_k)
    d['rowptr'], d['rowidx'] = csr(uid, U)
    d['gcoef_terms'] = (np.float32(TERM_SCALES[0]) * gcoef).astype(np.float32)
    for k, v in d.items():
        if isinstance(v, np.ndarray) and k != 'w':    # (w goes to torch.as_tensor as it is, which wants a writable array)
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def theta(name, terms=False):
    d_in, dim, widths = config(name)[:3]
    flat = og.glorot_init(d_in, widths, 3)
    flat = (flat + 0.05 * np.random.default_rng(5).standard_normal(flat.size).astype(np.float32)).astype(np.float32)
    return (np.float32(TERM_SCALES[1]) * flat).astype(np.float32) if terms else flat


def block_entries(rowptr):
    """CSR entries owned by each PB-point block of a map."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    U = rowptr.size - 1
    starts = np.arange(0, U, PB)
    return rowptr[np.minimum(starts + PB, U)] - rowptr[starts]


def ref_kw(name, dtype=torch.float64, terms=False):
    """Keyword arguments of oracle/tf1_graph.loss_and_grad for a case on the expanded rows."""
    d_in, dim, widths, q, act, source, integW = config(name)[:7]
    d = inputs(name)
    f = np.float64 if dtype == torch.float64 else np.float32
    n, n_k = d['Input'].shape[0], d['n_k']
    return dict(Input=d['Input'].astype(f), gcoef=d['gcoef_terms' if terms else 'gcoef'].astype(f),
                source=None if d['source'] is None else d['source'].astype(f),
                N=np.tile(d['N1'], n_k).reshape(n, 1).astype(f), dNt=np.tile(d['dNt1'], n_k).reshape(n, 1).astype(f),
                integW=None if d['integW'] is None else d['integW'].astype(f), intShape=[n_k, q], detJ=DETJ, detJvec=False,
                biInput=d['biInput'].astype(f), biLabel=d['biLabel'].astype(f), bDof=BDOF, biDimVal=BIDIMVAL, w=d['w'],
                dim=dim, time_dependent=True, is_source=source, integWflag=integW, activation=act)


@functools.lru_cache(maxsize=None)
def oracle(name, dtype=torch.float64):
    """oracle/tf1_graph.loss_and_grad of a case in fp64 (the reference) or fp32 (its conditioning), computed once."""
    d_in, dim, widths = config(name)[:3]
    f = np.float64 if dtype == torch.float64 else np.float32
    return og.loss_and_grad(theta(name).astype(f), d_in, widths, dtype, **ref_kw(name, dtype))


def terms_of(name, variant='all'):
    """(nldiff, nlflux, reaction) as tests/dedup_term_cases.terms_of gives them: 'all', 'none', or 'all' with one left out."""
    d = inputs(name)
    P1, Pd, D = (d['psi'], ONE), (d['psi'], DIFF), (None, DIFF)
    F, R = (d['phi'], FLUX), (d['rate'], COEF)
    return {'all': (Pd, F, R), 'none': (None, None, None), 'no_d': (P1, F, R), 'no_psi': (D, F, R), 'no_flux': (Pd, None, R),
            'no_react': (Pd, F, None)}[variant]


@functools.lru_cache(maxsize=None)
def terms_reference(name, variant='all', dtype=torch.float64):
    """tests/nldiff_ref.loss_and_grad of a TERM_CASES case with the three terms (or a variant), computed once."""
    d_in, dim, widths = config(name)[:3]
    f = np.float64 if dtype == torch.float64 else np.float32
    cast = lambda t: None if t is None else (None if t[0] is None else t[0].astype(f), t[1])
    nldiff, nlflux, reaction = (cast(t) for t in terms_of(name, variant))
    return nldiff_ref.loss_and_grad(theta(name, True).astype(f), d_in, widths, nldiff, nlflux, reaction, dtype,
                                    **ref_kw(name, dtype, terms=True))
