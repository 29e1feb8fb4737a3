"""
GPU tier of the learnt vectors' regularisation (vn_set_learnt_prior, vn_get_learnt_prior; `VarNet(learntPrior=...)`; the prior part
of vn_learnt_apply_kernel in vn_learnt.hip) against the fp64 restatement tests/prior_ref.py on the vectors of tests/prior_cases.py:
the nine coefficients and the J = 3 source and field amplitudes of cases 0 and 6 of tests/learnt_cases.py on the automatic route and
on the shared-point map, the flux-row amplitudes at (Jl, Jc) = (1, 0), (5, 4), (37, 27), (40, 24), and one boundary / initial
vector -- each with a dense random positive semi-definite matrix, a non-zero mean, L1 weights on some entries, an unmasked
entry, an entry that starts inside the shrinkage threshold and one with a bound that is reached.
  1  the prior's part of the gradient within the forward error of a length-J fp64 sum; an apply after a gradient call steps on the
     reported gradient; the penalty values, read without changing any state;
  2  eight steps on a two-batch schedule, vn_train_step and vn_grad + vn_apply in turn, within the step's bar of Adam64Prox on the
     engine's own gradients; the variants of tests/prior_ref.MUTANTS replayed on the observed sequence each leave a bar;
  3  shrinkage to exactly zero, Adam's bound under a quadratic prior, off is off, the launch count, every refusal, and the option
     through VarNet.
The worst err / bar per vector is written to prior_parity.json in the directory VN_RECORD_DIR names (default: profile_out/ beside
tests/; committed copy, next to the CPU-measured constant: profiles/prior_parity.json).
"""
import ctypes
import json
import os
from math import pi

import numpy as np
import pytest
import torch

from tests import bic_cases as bc
from tests import fbc_cases as fc
from tests import learnt_adam_ref as ar
from tests import learnt_cases as lc
from tests import prior_cases as pc
from tests import prior_ref as pr
from tests import test_bic_gpu as tb
from tests import test_fbc_gpu as tf
from tests.dedup_term_cases import DETJ
from tests.test_learnt_adam_gpu import build
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import VNError
from varnet_amd.varnet import VarNet

pytestmark = pytest.mark.gpu

RECORD = {}
GET = {'coef': 'get_coefs', 'source': 'get_source_amps', 'field': 'get_field_amps', 'bic': 'get_bic_amps', 'fluxbc': 'get_fluxbc_amps'}
LEARN = {k: 'set_%s_learn' % k for k in GET}
UNITS = [('lc', i, route) for i in lc.CASES for route in ('auto', 'dedup')] + [('fbc', Jl, Jc) for Jl, Jc in pc.FBC_VARIANTS] + [('bic', 0, 0)]
UNIT_IDS = ['%s-%s-%s' % u for u in UNITS]


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'prior_parity.json'), 'w') as f:
            json.dump({'gpu': RECORD}, f, indent=1, sort_keys=True)
    except OSError:
        pass


# ---- engines -----------------------------------------------------------------------------------------------------------------
def _half(eng, d, q, n_k, detJ, source):
    """The first half of the test functions of the interior rows d as batch 1."""
    m = n_k // 2
    eng.set_interior(1, d['Input'][:m * q], d['gcoef'][:m * q], None if source is None else source[:m * q], n_k=m, detJ=detJ)


def open_unit(unit, prior=True):
    """(engine with two batches, {kind: config}) of a unit, every vector registered from its config (tests/prior_cases.config)
    and, with `prior`, regularised by it."""
    what, a, b = unit
    if what == 'lc':
        eng, vecs = build(a, b, lc.split(a)), pc.lc_configs(a)
    elif what == 'fbc':
        eng, vecs = tf.make_engine(pc.FBC_CASE, 'auto', a, b, lr=lc.ENGINE_LR), {'fluxbc': pc.fbc_config(a, b)}
        case = fc.case(pc.FBC_CASE)
        d = fc.inputs(pc.FBC_CASE)[0]
        _half(eng, d, case[3], case[4], d['detJ'], None)
    else:
        eng, vecs = tb.make_engine(pc.BIC_CASE, 'auto', pc.BIC_J, lr=lc.ENGINE_LR), {'bic': pc.bic_config()}
        case = bc.case(pc.BIC_CASE)
        d = bc.inputs(pc.BIC_CASE)
        _half(eng, d, case[3], case[4], DETJ, d['source'] if case[8] else None)
    try:
        for k, cfg in vecs.items():
            getattr(eng, LEARN[k])([int(x) for x in cfg['mask']], cfg['start'], cfg['lo'], cfg['hi'], lr=pc.LR)
            if prior:
                set_prior(eng, k, cfg)
    except Exception:
        eng.close()
        raise
    return eng, vecs


def set_prior(eng, k, cfg):
    p = cfg['prior']
    eng.set_learnt_prior(k, p.weight, p.R, p.mean, p.l1)


def read(eng, k):
    torch.cuda.synchronize()
    return getattr(eng, GET[k])(grad=True)


def state(eng, kinds):
    torch.cuda.synchronize()
    return (eng.export_state().copy(),) + tuple(getattr(eng, GET[k])() for k in kinds) + (eng.step,)


def same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


# ---- 1. gradient and penalty values ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('unit', UNITS, ids=UNIT_IDS)
def test_prior_gradient_and_penalty_values(unit):
    """At the starting state: g0 without a prior (twice: the same bits), g1 with it; per masked entry |g1 - g0 - weight (R d)_j|
    within prior_ref.Prior64.grad_bound, unmasked entries exactly 0.  vn_get_learnt_prior against Prior64 within Q_bound and
    L1_bound, leaving state() as it was.  Then vn_apply: the reported gradient stays g1 and the step is Adam64Prox's on g1.  This
    test cannot tell a step on g1 from one on g1 + weight R d: Adam's first step is lr sign(g) whatever the size of g, so the two
    lie within a fraction of the bar of each other unless the second helping turns a sign (the distance is recorded, not asserted).
    The variant is asserted where it shows: on the even steps of the trajectories' replay (MUTANTS 'd')."""
    eng, vecs = open_unit(unit, prior=False)
    try:
        rec = {}
        eng.grad(0)
        g0 = {k: read(eng, k)[1] for k in vecs}
        eng.grad(0)
        assert all(np.array_equal(g0[k], read(eng, k)[1]) for k in vecs)
        for k, cfg in vecs.items():
            set_prior(eng, k, cfg)
        s0 = state(eng, vecs)
        pen = {k: eng.learnt_prior(k) for k in vecs}
        assert same(state(eng, vecs), s0) and eng.step == 0
        eng.grad(0)
        before, g1 = {}, {}
        for k, cfg in vecs.items():
            p, on = cfg['prior'], cfg['mask']
            before[k], g1[k] = read(eng, k)
            assert np.array_equal(before[k], cfg['start'])
            err = np.abs(g1[k] - g0[k] - p.grad(before[k]))
            allowed = p.grad_bound(before[k], g0[k])
            rel = float(np.max(np.where(on, err / allowed, 0.0)))
            ratio = float(np.linalg.norm(p.grad(before[k])[on]) / np.linalg.norm(g0[k][on]))
            print('%s %s: prior gradient err/bound %.3f; |weight R d| / |data gradient| %.3f' % (UNIT_IDS[UNITS.index(unit)], k, rel, ratio))
            assert np.all(g1[k][~on] == 0.0) and np.all(g0[k][~on] == 0.0), (k, g1[k])
            assert np.all(err[on] <= allowed[on]), (k, err / allowed)
            assert np.all(g1[k][on] != g0[k][on])
            q_err, l_err = abs(pen[k][0] - p.Q(before[k])), abs(pen[k][1] - p.L1(before[k]))
            print('%s %s: Q %.9g err/bound %.3f, L1 %.9g err/bound %.3f'
                  % (UNIT_IDS[UNITS.index(unit)], k, pen[k][0], q_err / p.Q_bound(before[k]), pen[k][1], l_err / p.L1_bound(before[k])))
            assert pen[k][0] > 0.0 and pen[k][1] > 0.0
            assert q_err <= p.Q_bound(before[k]) and l_err <= p.L1_bound(before[k]), (k, pen[k], p.Q(before[k]), p.L1(before[k]))
            rec[k] = {'gradient_err_over_bound': rel, 'Q_err_over_bound': q_err / p.Q_bound(before[k]),
                      'L1_err_over_bound': l_err / p.L1_bound(before[k]), 'prior_over_data_gradient': ratio}
        eng.apply()
        for k, cfg in vecs.items():
            p, on = cfg['prior'], cfg['mask']
            after, g = read(eng, k)
            assert np.array_equal(g, g1[k])                                          # (the apply folds nothing)
            want = pr.Adam64Prox(cfg['n'], on, pc.LR, cfg['lo'], cfg['hi'], l1=p.l1).step(before[k], g1[k], 1)
            twice = pr.Adam64Prox(cfg['n'], on, pc.LR, cfg['lo'], cfg['hi'], l1=p.l1).step(before[k], g1[k] + p.grad(before[k]), 1)
            allowed = pr.bar(before[k], want, ar.lr_t_of(pc.LR, 1))
            assert np.all(np.abs(after - want)[on] <= allowed[on]), (k, after, want)
            assert np.array_equal(after[~on], before[k][~on])
            rec[k]['added_again_bars_from_engine'] = float(np.max(np.where(on, np.abs(after - twice) / allowed, 0.0)))
            # (Adam's first step is lr sign(g) whatever the size of g: a second helping shows only where it turns a sign or at later
            # steps -- the trajectories' replay asserts it; here the figure is recorded)
        RECORD['gradient/' + UNIT_IDS[UNITS.index(unit)]] = rec
    finally:
        eng.close()


@pytest.mark.parametrize('unit', UNITS, ids=UNIT_IDS)
def test_a_step_reports_the_gradient_of_a_gradient_call(unit):
    """From one state, with the prior registered: the gradient vn_train_step reports is the gradient vn_grad reports, bit for bit.
    vn_grad updates nothing, vn_train_step steps every masked entry in the same launch: a kernel that formed d = a - mean from
    values other threads had already stepped would report another gradient here."""
    eng, vecs = open_unit(unit)
    try:
        eng.grad(0)
        quiet = {k: read(eng, k) for k in vecs}
        eng.train_step(0)
        for k, cfg in vecs.items():
            after, g = read(eng, k)
            on = cfg['mask']
            assert np.array_equal(quiet[k][0], cfg['start']) and np.all(after[on] != cfg['start'][on]), k    # (the step moved them)
            assert np.array_equal(g, quiet[k][1]), (k, g, quiet[k][1])
    finally:
        eng.close()


# ---- 2. trajectories -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('unit', UNITS, ids=UNIT_IDS)
def test_eight_steps_follow_the_restatement(unit):
    """Eight steps on the schedule of tests/learnt_cases.py over the two batches, odd ones through vn_train_step and even ones
    through vn_grad + vn_apply.  After every step each vector is within the step's bar of Adam64Prox started from the values before
    the step on the engine's own gradient; unmasked entries keep their bits; where the restatement's unclamped value lies beyond
    a bound by more than the bar the engine holds the bound bit for bit, and the bounded entry does reach one.  Then every variant
    of MUTANTS that the vector can show, replayed on the observed sequence, leaves a bar."""
    tag = UNIT_IDS[UNITS.index(unit)]
    eng, vecs = open_unit(unit)
    try:
        adam = {k: pr.Adam64Prox(c['n'], c['mask'], pc.LR, c['lo'], c['hi'], l1=c['prior'].l1) for k, c in vecs.items()}
        steps = {k: [] for k in vecs}
        worst = {k: 0.0 for k in vecs}
        vals = {k: read(eng, k)[0] for k in vecs}
        for t, which in enumerate(pc.SCHEDULE, 1):
            if pc.after_grad(t):
                eng.grad(which)
                eng.apply()
            else:
                eng.train_step(which)
            assert eng.step == t
            for k, cfg in vecs.items():
                p, on, a = cfg['prior'], cfg['mask'], adam[k]
                after, g = read(eng, k)
                want = a.step(vals[k], g, t)
                allowed = pr.bar(vals[k], want, a.lr_t(t))
                err = np.abs(after - want)
                rel = float(np.max(np.where(on, err / allowed, 0.0)))
                worst[k] = max(worst[k], rel)
                print('%s step %d batch %d %s: err/bar %.3f' % (tag, t, which, k, rel))
                assert np.all(np.isfinite(g)) and np.all(g[~on] == 0.0), (tag, t, k, g)
                assert np.array_equal(after[~on], vals[k][~on]), (tag, t, k)
                assert np.all(err[on] <= allowed[on]), (tag, t, k, after, want, err / allowed)
                beyond = np.maximum(a.lo - a.unclamped, a.unclamped - a.hi)
                pinned = on & (beyond > allowed)
                bound = np.where(a.unclamped < a.lo, a.lo, a.hi)
                assert np.array_equal(after[pinned], bound[pinned]), (tag, t, k, after, bound)
                steps[k].append(dict(t=t, before=vals[k], g_data=np.where(on, g - p.grad(vals[k]), 0.0), after_grad=pc.after_grad(t),
                                     g=g, after=after))
                vals[k] = after
        rec = {}
        for k, cfg in vecs.items():
            e = cfg['bounded']
            assert any(s['after'][e] in (cfg['lo'][e], cfg['hi'][e]) for s in steps[k]), (tag, k, [s['after'][e] for s in steps[k]])
            seen = {}
            for name, cls in pr.MUTANTS.items():
                if not pc.shows(cfg, name):
                    continue
                w = float(np.max(pr.replay(cls, steps[k], cfg['prior'], pc.LR, cfg['lo'], cfg['hi'])))
                print('%s %s: %s is %.3g bars from the engine' % (tag, k, name, w))
                assert w > 1.0, (tag, k, name, w)
                seen[name] = w
            rec[k] = {'worst_err_over_bar': worst[k], 'variants_bars_from_engine': seen}
        RECORD['steps/' + tag] = rec
    finally:
        eng.close()


# ---- 3. shrinkage to zero, Adam's bound, off is off --------------------------------------------------------------------------------
ZERO_CASE, ZERO_ENTRY = 6, 2


def zero_stream_engine(a0, route='auto'):
    """Case 6 of tests/learnt_cases.py as one batch with source stream 2 identically zero and amplitude 2 started at a0."""
    eng = build(ZERO_CASE, route, [lc.whole(ZERO_CASE)])
    Phi = np.array(lc.whole(ZERO_CASE)['Phi'])
    Phi[ZERO_ENTRY] = 0.0
    eng.set_source_basis(0, Phi)
    start = np.array(lc.initial(ZERO_CASE)['source'])
    start[ZERO_ENTRY] = a0
    eng.set_source_learn([1] * lc.J, start, None, None, lr=pc.LR)
    return eng


def test_shrinkage_reaches_exactly_zero_and_stays():
    """The zero stream's data gradient is exactly 0.  Without L1 the amplitude keeps its bits; with l1 = 1 every step takes
    lr_t off it within the bar, it is exactly 0.0 at the first T with sum_{t <= T} lr_t >= a0 (T +- 1 for rounding) and stays."""
    a0, lam = float(np.float32(0.02)), 1.0
    eng = zero_stream_engine(a0)
    try:
        for t in range(1, 5):
            eng.train_step(0)
            a, g = read(eng, 'source')
            assert g[ZERO_ENTRY] == 0.0 and a[ZERO_ENTRY] == a0, (t, a, g)
    finally:
        eng.close()
    total, T = 0.0, 0
    while total < a0:
        T += 1
        total += ar.lr_t_of(pc.LR, T)
    eng = zero_stream_engine(a0)
    try:
        eng.set_learnt_prior('source', l1=[0.0, 0.0, lam])
        x, first = a0, None
        for t in range(1, T + 4):
            (eng.train_step(0) if t % 2 else (eng.grad(0), eng.apply()))
            a, g = read(eng, 'source')
            lr_t = ar.lr_t_of(pc.LR, t)
            want = max(x - lr_t * lam, 0.0)
            print('zero stream step %d: amplitude %.9g, wanted %.9g' % (t, a[ZERO_ENTRY], want))
            assert g[ZERO_ENTRY] == 0.0
            assert abs(a[ZERO_ENTRY] - want) <= pr.bar(x, want, lr_t), (t, a[ZERO_ENTRY], want)
            if a[ZERO_ENTRY] == 0.0 and first is None:
                first = t
            if first is not None:
                assert a[ZERO_ENTRY] == 0.0, (t, a[ZERO_ENTRY])        # (the zero keeps the sign of c: +0.0 here, -0.0 from below)
            x = a[ZERO_ENTRY]
        assert first is not None and abs(first - T) <= 1, (first, T)
        assert eng.learnt_prior('source') == (0.0, 0.0)
        RECORD['zero_stream'] = {'T': T, 'first_exact_zero': first}
    finally:
        eng.close()


def test_adam_bound_under_a_quadratic_prior():
    """The zero stream with R = I, mean = 0, weight 1 and no L1: the gradient is the amplitude itself, Adam moves it by less than
    3.2 lr a step (|delta| <= lr (1 - beta1) / sqrt(1 - beta2)), so |a| strictly decreases and stays positive for the first
    floor(a0 / (4 lr)) steps."""
    a0 = 0.5
    eng = zero_stream_engine(a0)
    try:
        eng.set_learnt_prior('source', weight=1.0)
        n, x = int(np.floor(a0 / (4.0 * pc.LR))), a0
        assert n == 6
        for t in range(1, n + 1):
            eng.train_step(0)
            a, g = read(eng, 'source')
            assert g[ZERO_ENTRY] == x, (t, g[ZERO_ENTRY], x)                           # (0 + 1 * (x - 0), exact)
            assert 0.0 < a[ZERO_ENTRY] < x and x - a[ZERO_ENTRY] < 3.2 * pc.LR, (t, a[ZERO_ENTRY], x)
            x = a[ZERO_ENTRY]
    finally:
        eng.close()


@pytest.mark.parametrize('route', ['auto', 'dedup'])
def test_off_is_off(route):
    """A prior registered and cleared again (weight = 0, l1 = None), and l1 all zeros with weight = 0: four steps end in the bits
    of an engine that never heard of priors.  The launch count of a learning step is the same with and without a prior."""
    kinds = lc.VECTORS
    cfgs = pc.lc_configs(ZERO_CASE)

    def run(prepare):
        eng = build(ZERO_CASE, route, [lc.whole(ZERO_CASE)])
        try:
            prepare(eng)
            for t in range(1, 5):
                (eng.train_step(0) if t % 2 else (eng.grad(0), eng.apply()))
            return state(eng, kinds)
        finally:
            eng.close()

    def cleared(eng):
        for k in kinds:
            p = cfgs[k]['prior']
            eng.set_learnt_prior(k, p.weight, p.R, p.mean, p.l1)
            eng.set_learnt_prior(k, 0.0, None, None, None)
            assert eng.learnt_prior(k) == (0.0, 0.0)

    def zeros(eng):
        for k in kinds:
            eng.set_learnt_prior(k, 0.0, l1=np.zeros(lc.SIZE[k]))

    def full(eng):
        for k in kinds:
            p = cfgs[k]['prior']
            eng.set_learnt_prior(k, p.weight, p.R, p.mean, p.l1)

    plain = run(lambda eng: None)
    assert same(run(cleared), plain)
    assert same(run(zeros), plain)
    assert not same(run(full), plain)

    def launches(prepare):
        eng = build(ZERO_CASE, route, [lc.whole(ZERO_CASE)])
        try:
            prepare(eng)
            eng.train_step(0)
            eng.profile_begin()
            eng.train_step(0)
            return eng.profile_end()[1]
        finally:
            eng.close()

    n0, n1 = launches(lambda eng: None), launches(full)
    print('launches of a learning step (%s): %d without a prior, %d with' % (route, n0, n1))
    assert n0 == n1 and n0 > 0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    eng = build(ZERO_CASE, 'auto', [lc.whole(ZERO_CASE)])
    try:
        raw = lambda kind, J, w, R=None, mean=None, l1=None: eng._ck(eng.lib.vn_set_learnt_prior(
            eng.h, kind, J, w, *(None if v is None else np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
                                 for v in (R, mean, l1))))
        with pytest.raises(VNError, match=r'error 3: no learnt boundary and initial amplitudes \(call vn_set_bic_learn first\)'):
            eng.set_learnt_prior('bic', 1.0)
        with pytest.raises(VNError, match=r'error 3: no learnt flux and Robin amplitudes \(call vn_set_fluxbc_learn first\)'):
            eng.learnt_prior('fluxbc')
        with pytest.raises(VNError, match='error 1: the engine holds 3 source amplitudes, the prior is for 4'):
            raw(1, 4, 1.0)
        with pytest.raises(VNError, match='error 1: learnt vector kind 5 is none of VN_LEARNT_COEF .. VN_LEARNT_FLUXBC'):
            raw(5, 3, 1.0)
        for w in (-1.0, np.nan, np.inf):
            with pytest.raises(VNError, match='error 1: prior weight .* must be finite and >= 0'):
                eng.set_learnt_prior('source', w)
        R = np.eye(3)
        R[0, 2] = np.inf
        with pytest.raises(VNError, match=r'error 1: prior matrix entries \(2, 0\) = 0 and \(0, 2\) = inf must be finite'):
            eng.set_learnt_prior('source', 1.0, R)
        R = np.eye(3)
        R[1, 0] = 0.5
        with pytest.raises(VNError, match=r'error 1: prior matrix is not symmetric: entry \(1, 0\) = 0.5, entry \(0, 1\) = 0'):
            eng.set_learnt_prior('source', 1.0, R)
        with pytest.raises(VNError, match='error 1: prior mean of amplitude 1 = nan must be finite'):
            eng.set_learnt_prior('source', 1.0, None, [0.0, np.nan, 0.0])
        with pytest.raises(VNError, match='error 1: L1 weight of amplitude 2 = -0.25 must be finite and >= 0'):
            eng.set_learnt_prior('source', 0.0, l1=[0.0, 0.0, -0.25])
        with pytest.raises(VNError, match='error 1: L1 weight of coefficient 8 = -1 must be finite and >= 0'):
            eng.set_learnt_prior('coef', 1.0, l1=[0.0] * 8 + [-1.0])
        with pytest.raises(ValueError, match="unknown learnt vector 'sources'"):
            eng.set_learnt_prior('sources', 1.0)
        with pytest.raises(ValueError, match=r'matrix of the source prior must have shape \(3, 3\), got \(2, 2\)'):
            eng.set_learnt_prior('source', 1.0, np.eye(2))
        # a refused call leaves the registered prior in place; vn_set_source_learn drops it
        eng.set_learnt_prior('source', 2.0, l1=1.0)
        q = eng.learnt_prior('source')
        assert q[0] > 0.0 and q[1] > 0.0
        with pytest.raises(VNError):
            eng.set_learnt_prior('source', -1.0)
        assert eng.learnt_prior('source') == q
        eng.set_source_learn([1] * lc.J, lc.initial(ZERO_CASE)['source'], None, None, lr=pc.LR)
        assert eng.learnt_prior('source') == (0.0, 0.0)
        # ... and so does a refused one (like the snapshot, which it invalidates)
        eng.set_learnt_prior('source', 2.0, l1=1.0)
        assert eng.learnt_prior('source') == q
        with pytest.raises(VNError, match='error 1: amplitude learning rate -1 must be finite and > 0'):
            eng.set_source_learn([1] * lc.J, lc.initial(ZERO_CASE)['source'], None, None, lr=-1.0)
        assert eng.learnt_prior('source') == (0.0, 0.0)
        eng.set_learnt_prior('source', 2.0, l1=1.0)
        eng.set_source_learn(None)
        with pytest.raises(VNError, match=r'error 3: no learnt source amplitudes \(call vn_set_source_learn first\)'):
            eng.learnt_prior('source')
    finally:
        eng.close()


# ---- 5. through VarNet ---------------------------------------------------------------------------------------------------------
KAPPA, T_END = 0.1, 0.5
A0 = [0.5, -0.5, 0.25, 0.05]


def _u(x, t):
    return sum(a * np.sin(j * pi * x) * (1.0 - np.exp(-KAPPA * j * j * pi * pi * t)) / (KAPPA * j * j * pi * pi)
               for a, j in zip((2.0, -1.0, 4.0), (1, 2, 3)))


def test_through_varnet(tmp_path):
    """A small 1D+t source identification with a fourth basis function that is identically zero, started at 0.05, under
    learntPrior={'source': {weight 2, identity, mean (a0 with 0 for the zero stream), l1 5 on the zero stream}}: with l1 above
    (1 - beta1) / sqrt(1 - beta2) = 3.16 the threshold exceeds any move Adam can make, so the entry reaches exactly 0.0 and
    stays (as -0.0 when it is shrunk from below: the proximal map keeps the sign).  priorPenalty() is NumPy's on sourceAmplitudes() within the penalty bounds, setPriorWeight scales it by the ratio of
    the weights, caseData.txt carries the prior's line; the reported loss does not contain the penalty."""
    rng = np.random.default_rng(0)
    x, t = rng.uniform(0, 1, 32), rng.uniform(0, T_END, 32)
    basis = [lambda x, t, j=j: np.sin(j * pi * x) for j in (1, 2, 3)] + [lambda x, t: 0.0 * x]
    pde = ADPDE(Domain1D(np.array([0.0, 1.0])), diff=KAPPA, vel=0.0, tInterval=[0, T_END], IC=lambda x: 0.0 * x, cEx=_u,
                sourceBasis=basis, sourceAmp=A0)
    mean, l1 = [0.5, -0.5, 0.25, 0.0], [0.0, 0.0, 0.0, 5.0]
    with pytest.raises(ValueError, match=r"learntPrior\['field'\]: this instance does not learn that vector \(learnField=\.\.\.\)"):
        VarNet(pde, layerWidth=[10], activationFun='tanh', discNum=10, bDiscNum=None, tDiscNum=5, observations=(np.column_stack([x, t]), _u(x, t)),
               learnSource=True, learntPrior={'field': {'diff': {'weight': 1.0}}})
    np.random.seed(0)
    vn = VarNet(pde, layerWidth=[10], activationFun='tanh', discNum=10, bDiscNum=None, tDiscNum=5, learning_rate=0.01,
                observations=(np.column_stack([x, t]), _u(x, t)), learnSource=True, sourceLr=0.02,
                learntPrior={'source': {'weight': 2.0, 'mean': mean, 'l1': l1}})
    try:
        p = pr.Prior64(4, 2.0, None, mean, l1)
        q0 = vn.priorPenalty()
        assert list(q0) == ['source'] and abs(q0['source'][0] - p.Q(ar.f32(A0))) <= p.Q_bound(ar.f32(A0))
        vn.train(str(tmp_path), weight=[10.0, 10.0, 1.0], epochNum=30, tol=0.0, saveFreq=30, verbose=False)
        a = vn.sourceAmplitudes()
        print('through VarNet: amplitudes %s' % a)
        assert a[3] == 0.0 and np.all(a[:3] != ar.f32(A0)[:3])
        Q, L = vn.priorPenalty()['source']
        assert abs(Q - p.Q(a)) <= p.Q_bound(a) and abs(L - p.L1(a)) <= p.L1_bound(a) and Q > 0.0 and L == 0.0
        vn.setPriorWeight('source', weight=5.0)
        Q5 = vn.priorPenalty()['source'][0]
        assert Q5 == pytest.approx(Q * 5.0 / 2.0, rel=1e-13) and np.array_equal(vn.sourceAmplitudes(), a)
        vn.setPriorWeight('source', l1=1.0)
        L1 = vn.priorPenalty()['source'][1]
        assert abs(L1 - float(np.sum(np.abs(a)))) <= 6 * 2.0 ** -52 * float(np.sum(np.abs(a)))
        with pytest.raises(ValueError, match=r"setPriorWeight\('source'\): weight -1\.0 is negative"):
            vn.setPriorWeight('source', weight=-1.0)
        with pytest.raises(ValueError, match="setPriorWeight: no prior on 'coef'"):
            vn.setPriorWeight('coef', weight=1.0)
        text = open(os.path.join(str(tmp_path), 'caseData.txt')).read()
        assert 'Prior on the learnt source: weight 2.0, matrix identity, mean [0.5, -0.5, 0.25, 0.0], l1 [0.0, 0.0, 0.0, 5.0]' in text
        RECORD['varnet'] = {'amplitudes': [float(v) for v in a], 'Q': Q}
    finally:
        vn.engine.close()
