"""
Host-side tables of the tests of the learnt vectors' step (tests/test_learnt_adam_host.py, tests/test_learnt_adam_gpu.py): the two
WIDE cases of tests/source_cases.py / tests/field_cases.py / tests/inverse_cases.py with all three vectors learnt, each also cut
into two batches, and fp64 reference trajectories of eight steps.  Plain module (no GPU, no pytest marks).

Cases: 0 (bench_rand: 5 x 50, q 64, n_k 24) and 6 (1d_steady_q6: 2 x 20 tanh, q 6, n_k 77, nT % 4 == 2: the one-row-per-thread
kernels).  The vectors as tests/test_learnt_gpu.learnt_engine sets them: J = 3 for source and field, all nine coefficients masked,
vector rate 0.02, engine rate 0.01.

split(i): the test functions [0, n_a) and [n_a, n_k) of case i as two batches -- rows, streams, basis streams and uid sliced, the
CSR map rebuilt over the full Xu (the points that lose their rows become row-less points, as in case 10 of tests/source_cases.py).
Case 0: n_a = 9, 576 and 960 rows, both on the four-row kernels.  Case 6: n_a = 36, 216 rows (a multiple of 4) and 246 rows
(% 4 == 2): a schedule that alternates the batches alternates the four-row and the one-row reduction kernels.  Batch 1 carries no
reaction term; the three reaction coefficients stay masked, so on a batch-1 step their gradient is 0 and they move by the momentum
of the batch-0 steps before.

Reference trajectories (trajectory(i, kind), K = 8 steps, cached, read-only): the parameters step by oracle.tf1_graph.TF1Adam in
fp64, the three vectors by tests/learnt_adam_ref.Adam64, on the gradients of tests/inverse_ref.py, tests/source_ref.py and
tests/field_ref.py, each called with the other two vectors' streams mixed beforehand in fp64.
  'two'    the two batches on the schedule [0, 1, 1, 0, 1, 0, 0, 1]
  'one'    the whole case as one batch
  'bound'  the whole case as one batch with one one-sided bound per vector, and after step 5 every vector overwritten with its
           initial values by its setter (the slots stay), then steps 6..8
  'free'   'bound' without the bounds and the setters, which the bounds are placed from ('one' where the rates are the same)
bound_scenario(i) places each bound from trajectory(i, 'free') alone: on the entry that moves one way for the most steps from the
start (ties: the one that gets furthest), a quarter of the way from its value after step 1 to its value after step 2 -- so the
reference reaches it at step 2, and its momentum holds it there.  tests/test_learnt_adam_host.py asserts from trajectory(i, 'bound')
that each bound is first reached at a step >= 2, holds for two further steps at least, and is left when the setter runs.

Changed inputs.  The cut points were first 10 and 38.  There the conditioning floor 0.01 S of the gradient bars was the binding
branch for three of the 54 components the two-batch references have (|g| / S: 0.0099 for c1 and 0.0025 for b_0 on batch 0 of case
0, 0.0033 for b_0 on batch 1 of case 6), and the sibling tables allow that for 5 % of the field's and the source's components:
none of twelve each.  The nearest cut points with every component above the floor (smallest |g| / S: 0.021 on both cases) are 9 and
36, which keep what the cut is for: both batches of case 0 on the four-row kernels, 4 k and 4 k + 2 rows on case 6, the second
batch the larger one.  Scanned: 6..14 on case 0 (10, 11, 12 have a component on the floor), the even 28..48 on case 6 (34 and 36
have none).  Case 0 runs 'bound' at the engine rate 0.001 (the default of the sibling tests' make_engine), not 0.01: at 0.01
the parameters of that stiff case swing back within three steps and take the source amplitudes' gradient with them -- it hardly
depends on the amplitudes themselves: (6.3e4, 1.5e3, -3.4e4, -5.1e4) on a_0 over steps 1..4 from any start between 0.75 and 1.5
times the table's -- so no bound on any source amplitude holds beyond steps 2 and 3 (measured with the bound half way and a
quarter of the way).  At 0.001 every vector of case 0 has an entry that moves one way through all eight steps, and each bound
holds for steps 2..5.  Case 6 runs 'bound' at 0.01.
"""
import functools

import numpy as np
import torch

from oracle import tf1_graph as og
from tests import dedup_term_cases as dt
from tests import field_cases as fc
from tests import field_ref, inverse_ref, source_ref
from tests import inverse_cases as ic
from tests import source_cases as sc
from tests.learnt_adam_ref import Adam64

CASES = [0, 6]
IDS = [sc.IDS[i] for i in CASES]
J = 3
LR, ENGINE_LR = 0.02, 0.01
N_A = {0: 9, 6: 36}
SCHEDULE = (0, 1, 1, 0, 1, 0, 0, 1)
K = len(SCHEDULE)
SET_AFTER = 5                                  # 'bound': the value setters run after this step
BOUND_ENGINE_LR = {0: 0.001}                   # 'bound': the engine rate of a case that needs another (module docstring)
BOUND_AT = 0.25                                # ... and a bound lies this far on the way from the value after step 1 to that after step 2
VECTORS = ('coef', 'source', 'field')
SIZE = {'coef': 9, 'source': J, 'field': J}
SLICED = ('uid', 'Input', 'gcoef', 'source', 'rate', 'phi', 'psi')


def _freeze(d):
    for k, v in d.items():
        if isinstance(v, np.ndarray) and k != 'w':
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def whole(i):
    """The inputs of case i plus its basis streams: Phi [J, nT], G [J, nT, dim], s0 [nT]; `reaction`: the batch has the term."""
    d = dict(sc.inputs(i))
    d.update(Phi=sc.basis(i, J)[0], G=fc.basis(i, J)[0], s0=sc.s0_of(i), reaction=True, n_k=sc.case(i)[4])
    return _freeze(d)


@functools.lru_cache(maxsize=None)
def split(i):
    """(batch 0, batch 1) of case i: dicts like whole(i)."""
    w = whole(i)
    q, n_k = sc.case(i)[3], sc.case(i)[4]
    out = []
    for k, (a, b) in enumerate(((0, N_A[i]), (N_A[i], n_k))):
        r = slice(a * q, b * q)
        d = dict(w)
        for key in SLICED:
            if d[key] is not None:
                d[key] = np.ascontiguousarray(d[key][r])
        d['Phi'] = np.ascontiguousarray(w['Phi'][:, r])
        d['G'] = np.ascontiguousarray(w['G'][:, r])
        d['s0'] = np.ascontiguousarray(w['s0'][r])
        d['rowptr'], d['rowidx'] = dt.csr(d['uid'], d['Xu'].shape[0])
        d['reaction'], d['n_k'] = k == 0, b - a
        out.append(_freeze(d))
    return tuple(out)


def batch(i, which):
    """which: 'whole', 0 or 1."""
    return whole(i) if which == 'whole' else split(i)[which]


def terms_of(i, d):
    """(nldiff, nlflux, reaction) of a batch as tests/dedup_term_cases.terms_of gives them."""
    return dt.terms_of(i, 'all' if d['reaction'] else 'no_react', d)


def initial(i):
    """(coefficients [9], source amplitudes [J], field amplitudes [J]) the vectors are registered with."""
    return {'coef': sc.coefs_of(i), 'source': sc.basis(i, J)[1], 'field': fc.basis(i, J)[1]}


def gradients(i, which, theta, vec, dtype=torch.float64):
    """The reference's gradients of batch `which` of case i at the parameters theta and the vectors vec (a dict by VECTORS):
    {'theta': g, 'coef': (g, S), 'source': (g, S), 'field': (g, S)}; dtype: the arithmetic (the streams of the other two vectors
    are mixed in fp64 either way)."""
    d = batch(i, which)
    d_in, widths = sc.case(i)[0], sc.case(i)[2]
    kw = dt.ref_kw(i, dtype, d=d)
    nldiff, nlflux, reaction = terms_of(i, d)
    coef, samp, famp = (np.asarray(vec[k], dtype=np.float64) for k in VECTORS)
    gmix = d['gcoef'].astype(np.float64) + np.tensordot(famp, d['G'].astype(np.float64), axes=1)
    smix = (d['s0'].astype(np.float64) + samp @ d['Phi'].astype(np.float64)).reshape(-1, 1)
    mixed = dict(kw, gcoef=gmix, source=smix, is_source=True)
    _, g, gc, Sc = inverse_ref.evaluate(theta, d_in, widths, coef, nldiff, nlflux, reaction, dtype, **mixed)
    _, _, gs, Ss = source_ref.evaluate(theta, d_in, widths, d['s0'], d['Phi'].T, samp, coef, nldiff, nlflux, reaction, dtype,
                                       **dict(kw, gcoef=gmix))
    _, _, gf, Sf = field_ref.evaluate(theta, d_in, widths, d['gcoef'], d['G'], famp, coef, nldiff, nlflux, reaction, dtype,
                                      **dict(kw, source=smix, is_source=True))
    return {'theta': g, 'coef': (gc, Sc), 'source': (gs, Ss), 'field': (gf, Sf)}


@functools.lru_cache(maxsize=None)
def reference64(i, which):
    """gradients() of a batch in fp64 at the initial state, computed once."""
    out = gradients(i, which, sc.theta(i).astype(np.float64), initial(i))
    out['theta'].setflags(write=False)
    for k in VECTORS:
        for a in out[k]:
            a.setflags(write=False)
    return out


BARS = {'coef': ic.bars, 'source': sc.bars, 'field': fc.bars}      # each vector's existing gradient bar


def _run(i, whiches, bounds=None, engine_lr=None):
    theta = sc.theta(i).astype(np.float64)
    vec = {k: v.copy() for k, v in initial(i).items()}
    opt = og.TF1Adam(theta.size, lr=ENGINE_LR if engine_lr is None else engine_lr, dtype=np.float64)
    adam = {}
    for k in VECTORS:
        lo, hi = (None, None) if bounds is None else bounds_of(bounds, k)
        adam[k] = Adam64(SIZE[k], None, LR, lo, hi)
    steps = {k: [] for k in VECTORS}
    for n, which in enumerate(whiches):
        t = n + 1
        was_set = bounds is not None and n == SET_AFTER
        if was_set:
            vec = {k: v.copy() for k, v in initial(i).items()}
            for k in VECTORS:
                adam[k].on_set()
        g = gradients(i, which, theta, vec)
        theta = opt.step(theta, g['theta'])
        for k in VECTORS:
            after = adam[k].step(vec[k], g[k][0], t)
            steps[k].append(_freeze(dict(t=t, batch=which, before=vec[k].copy(), g=g[k][0].copy(), after=after.copy(),
                                         unclamped=adam[k].unclamped.copy(), set=was_set)))
            vec[k] = after
    return {k: tuple(v) for k, v in steps.items()}


def engine_lr(i, kind):
    """The engine's (parameters') rate of a trajectory."""
    return BOUND_ENGINE_LR.get(i, ENGINE_LR) if kind == 'bound' else ENGINE_LR


def bounds_of(scenario, k):
    """(lo, hi) vectors of vector k in a bound scenario."""
    entry, side, value = scenario[k]
    lo, hi = np.full(SIZE[k], -np.inf), np.full(SIZE[k], np.inf)
    (lo if side == 'lo' else hi)[entry] = value
    return lo, hi


@functools.lru_cache(maxsize=None)
def bound_scenario(i):
    """{vector: (entry, 'lo' or 'hi', bound)}: one one-sided bound per vector, an fp32 number, placed from trajectory(i, 'free')."""
    out = {}
    for k in VECTORS:
        steps = trajectory(i, 'free')[k]
        x = np.array([steps[0]['before']] + [s['after'] for s in steps[:SET_AFTER]])        # values after steps 0..5
        dx = np.diff(x, axis=0)
        run = np.array([next((n for n in range(SET_AFTER) if dx[n, e] * dx[0, e] <= 0), SET_AFTER) for e in range(SIZE[k])])
        far = np.array([abs(x[run[e], e] - x[0, e]) for e in range(SIZE[k])])
        entry = int(np.argmax(np.where(run == run.max(), far, -1.0)))
        out[k] = (entry, 'hi' if dx[0, entry] > 0 else 'lo', float(np.float32(x[1, entry] + BOUND_AT * (x[2, entry] - x[1, entry]))))
    return out


@functools.lru_cache(maxsize=None)
def trajectory(i, kind):
    """{vector: K step records (t, batch, before, g, after, unclamped, set)} of the fp64 reference; kind: 'one', 'two', 'bound', 'free'."""
    if kind == 'two':
        return _run(i, SCHEDULE)
    if kind == 'free' and engine_lr(i, 'bound') == ENGINE_LR:
        return trajectory(i, 'one')
    return _run(i, ('whole',) * K, bound_scenario(i) if kind == 'bound' else None, engine_lr(i, 'bound' if kind == 'free' else kind))


def first_bound_step(steps, entry, bound):
    """(the first step t whose result is the bound, how many steps from there on end on it in a row)."""
    on = [s['after'][entry] == bound for s in steps]
    if True not in on:
        return None, 0
    k = on.index(True)
    n = 0
    while k + n < len(on) and on[k + n]:
        n += 1
    return steps[k]['t'], n


def sequences():
    """Every (case, kind, vector, steps, lo, hi) the step is measured and the variants are tried on."""
    for i in CASES:
        for kind in ('one', 'two', 'bound'):
            for k in VECTORS:
                lo, hi = bounds_of(bound_scenario(i), k) if kind == 'bound' else (None, None)
                yield i, kind, k, trajectory(i, kind)[k], lo, hi
