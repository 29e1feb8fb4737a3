"""
GPU tier of the step the three learnt vectors take -- the nine polynomial coefficients (vn_set_coef_learn), the source amplitudes
(vn_set_source_learn) and the field amplitudes (vn_set_field_learn); vn_learnt_apply_kernel of vn_learnt.hip, driven by
learnt_finish -- against the fp64 restatement tests/learnt_adam_ref.Adam64 over eight steps, on the cases of
tests/learnt_cases.py, on the automatic route and on the case's shared-point map:
  a  one batch, vn_train_step and vn_grad + vn_apply in turn;
  b  one bound per vector that is reached at step 2 and held, then every vector overwritten by its value setter after step 5;
  c  two batches of different sizes on one schedule, the second without a reaction term.
The slots are not in vn_state_export, so the trajectory is the witness: after every step the engine's values are compared with
Adam64 started from the engine's values of the step before, on the engine's own gradients, within tests/learnt_adam_ref.bar
(half an ulp of the stored fp32 value plus C lr_t, C measured on the CPU: tests/test_learnt_adam_host.py).  Each test then replays
the variants of tests/learnt_adam_ref.MUTANTS in NumPy on the sequence it observed and requires each to leave the bar: a device
with that slip would have failed here.

The worst err / bar per test and vector is written to learnt_adam_parity.json in the directory VN_RECORD_DIR names (default:
profile_out/ beside tests/; committed copy, next to the CPU-measured C: profiles/learnt_adam_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import learnt_adam_ref as ar
from tests import learnt_cases as lc
from tests import source_cases as sc
from tests.dedup_term_cases import BIDIMVAL, DETJ
from tests.test_inverse_gpu import STEP_MASK
from varnet_amd.engine import VN_KERNEL_AUTO, VNEngine, VNError

pytestmark = pytest.mark.gpu

RECORD = {}
CASE_IDS = dict(zip(lc.CASES, lc.IDS))
ALL = {'coef': [1] * 9, 'source': [1] * lc.J, 'field': [1] * lc.J}
SOME = {'coef': STEP_MASK, 'source': [1, 1, 0], 'field': [1, 0, 1]}
RUNS = [(i, route, ALL) for i in lc.CASES for route in ('auto', 'dedup')] + [(6, 'auto', SOME)]
RUN_IDS = ['%s-%s%s' % (CASE_IDS[i], route, '' if m is ALL else '-masked') for i, route, m in RUNS]
PAIRS = [(i, route) for i in lc.CASES for route in ('auto', 'dedup')]
PAIR_IDS = ['%s-%s' % (CASE_IDS[i], route) for i, route in PAIRS]
GET = {'coef': 'get_coefs', 'source': 'get_source_amps', 'field': 'get_field_amps'}
SET = {'coef': 'set_coefs', 'source': 'set_source_amps', 'field': 'set_field_amps'}
LEARN = {'coef': 'set_coef_learn', 'source': 'set_source_learn', 'field': 'set_field_learn'}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'learnt_adam_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def build(i, route, batches, masks=ALL, bounds=None, lr=lc.ENGINE_LR):
    """An engine of case i with `batches` (dicts of tests/learnt_cases.py) registered as batch 0, 1, ...: the case's terms (the
    reaction only where the batch has it), both bases, on route 'dedup' the batch's shared-point map; the three vectors learnt
    from the case's own values at the rate lc.LR, with `bounds` (a scenario of lc.bound_scenario) or unbounded."""
    d_in, dim, widths, q, _, _, _, bDof, _, integW, td, act = sc.case(i)[:12]
    w = lc.whole(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=True, integWflag=integW, activationFun=act, learning_rate=lr, kernel=VN_KERNEL_AUTO)
    try:
        eng.set_params(sc.theta(i))
        eng.set_fe_table(w['N1'], w['dNt1'], w['integW'])
        eng.set_bic(w['biInput'], w['biLabel'], bDof, BIDIMVAL)
        eng.set_weights(w['w'])
        for b, d in enumerate(batches):
            eng.set_interior(b, d['Input'], d['gcoef'], d['s0'], n_k=d['n_k'], detJ=DETJ)
            nldiff, nlflux, reaction = lc.terms_of(i, d)
            if reaction is not None:
                eng.set_reaction(b, *reaction)
            eng.set_nlflux(b, *nlflux)
            eng.set_nldiff(b, *nldiff)
            eng.set_source_basis(b, d['Phi'])
            eng.set_field_basis(b, d['G'])
            if route == 'dedup':
                eng.set_dedup(b, d['Xu'], d['uid'], d['rowptr'], d['rowidx'])
        for k in lc.VECTORS:
            lo, hi = (None, None) if bounds is None else lc.bounds_of(bounds, k)
            getattr(eng, LEARN[k])(masks[k], lc.initial(i)[k], lo, hi, lr=lc.LR)
    except Exception:
        eng.close()
        raise
    return eng


def read(eng):
    """({vector: values}, {vector: gradient of the last evaluation}) on the host."""
    torch.cuda.synchronize()
    got = {k: getattr(eng, GET[k])(grad=True) for k in lc.VECTORS}
    return {k: v[0] for k, v in got.items()}, {k: v[1] for k, v in got.items()}


def state(eng):
    """(parameters and their slots, the three vectors, step counter) on the host."""
    vals = read(eng)[0]
    return (eng.export_state().copy(),) + tuple(vals[k] for k in lc.VECTORS) + (eng.step,)


def same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


class Follower:
    """Adam64 per vector beside an engine: after each engine step, check() holds the engine's values against the restatement
    started from the values before the step, on the engine's gradients, and keeps the observed sequence for the variants."""

    def __init__(self, tag, i, masks=ALL, bounds=None):
        self.tag, self.i, self.masks, self.bounds = tag, i, masks, bounds
        self.lohi = {k: (None, None) if bounds is None else lc.bounds_of(bounds, k) for k in lc.VECTORS}
        self.adam = {k: ar.Adam64(lc.SIZE[k], masks[k], lc.LR, *self.lohi[k]) for k in lc.VECTORS}
        self.steps = {k: [] for k in lc.VECTORS}
        self.worst = {k: 0.0 for k in lc.VECTORS}
        self.arith = {k: 0.0 for k in lc.VECTORS}
        self.was_set = False

    def on_set(self):
        for a in self.adam.values():
            a.on_set()
        self.was_set = True

    def check(self, eng, t, before, batch=0):
        assert eng.step == t, (self.tag, eng.step, t)
        after, grad = read(eng)
        for k in lc.VECTORS:
            a, on = self.adam[k], np.asarray(self.masks[k], dtype=bool)
            want = a.step(before[k], grad[k], t)
            bar = ar.bar(before[k], want, a.lr_t(t))
            err = np.abs(after[k] - want)
            self.steps[k].append(dict(t=t, batch=batch, before=before[k], g=grad[k], after=after[k], want=want,
                                      unclamped=a.unclamped.copy(), set=self.was_set))
            rel = float(np.max(np.where(on, err / bar, 0.0)))
            self.worst[k] = max(self.worst[k], rel)
            # (most of the bar is the half ulp, which a rounded result uses up: how much of the C lr_t part the arithmetic took)
            arith = (err - ar.bar(before[k], want, 0.0, c=0.0)) / (ar.C * a.lr_t(t))
            self.arith[k] = max(self.arith[k], float(np.max(np.where(on, arith, 0.0))))
            print('%s step %d batch %s %s: err/bar %.3f' % (self.tag, t, batch, k, rel))
            assert np.all(np.isfinite(grad[k])) and np.all(grad[k][~on] == 0.0), (self.tag, t, k, grad[k])
            assert np.array_equal(after[k][~on], before[k][~on]), (self.tag, t, k)               # unmasked: their bits
            assert np.all(err[on] <= bar[on]), (self.tag, t, k, after[k], want, err / bar)
            lo, hi = a.lo, a.hi
            beyond = np.maximum(lo - a.unclamped, a.unclamped - hi)                              # > 0: Adam's value lies outside
            pinned = on & (beyond > bar)
            bound = np.where(a.unclamped < lo, lo, hi)
            assert np.array_equal(after[k][pinned], bound[pinned]), (self.tag, t, k, after[k], bound)   # the bound, bit for bit
        self.was_set = False
        return after

    def variants(self, names, pick=None, from_t=2):
        """Each named variant replayed on the observed sequence: the largest |variant - engine| / bar over the steps >= from_t
        (and the (steps, entries) `pick` of a vector selects) has to exceed 1 for every vector `pick` names (default: all)."""
        out = {}
        for k in (lc.VECTORS if pick is None else pick):
            steps, n = self.steps[k], lc.SIZE[k]
            keep = np.array([s['t'] >= from_t for s in steps])[:, None] & np.asarray(self.masks[k], dtype=bool)
            if pick is not None:
                keep = keep & pick[k]
            for name in names:
                r = ar.replay(ar.MUTANTS[name], steps, n, self.masks[k], lc.LR, *self.lohi[k])
                w = float(np.max(np.where(keep, r, 0.0)))
                print('%s %s: %s is %.3g bars from the engine' % (self.tag, k, name, w))
                assert w > 1.0, (self.tag, k, name, w)
                out['%s/%s' % (k, name)] = w
        return out

    def record(self, extra=None):
        RECORD[self.tag] = dict({'worst_err_over_bar': dict(self.worst), 'worst_err_beyond_half_ulp_over_C_lr_t': dict(self.arith)},
                                **(extra or {}))
        print('learnt adam %s: %s' % (self.tag, json.dumps(RECORD[self.tag], sort_keys=True)))


def one_step(eng, t, batch=0):
    """Odd steps through vn_train_step, even ones through vn_grad + vn_apply."""
    if t % 2:
        eng.train_step(batch)
    else:
        eng.grad(batch)
        eng.apply()


# ---- a. one batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i,route,masks', RUNS, ids=RUN_IDS)
def test_eight_steps_follow_adam(i, route, masks):
    """Every masked entry of every vector at every step within the bar of Adam64, unmasked entries keep their bits; on the
    observed gradients the variants (a) - (d), (h) leave the bar."""
    tag = 'one/' + RUN_IDS[RUNS.index((i, route, masks))]
    eng = build(i, route, [lc.whole(i)], masks)
    try:
        f = Follower(tag, i, masks)
        vals = read(eng)[0]
        assert all(np.array_equal(vals[k], ar.f32(lc.initial(i)[k])) for k in lc.VECTORS)       # (stored in fp32)
        for t in range(1, lc.K + 1):
            one_step(eng, t)
            vals = f.check(eng, t, vals)
        for k in lc.VECTORS:
            on = np.asarray(masks[k], dtype=bool)
            assert np.all(vals[k][on] != lc.initial(i)[k][on]), (tag, k)
        f.record({'variants_bars_from_engine': f.variants(ar.ANY_SEQUENCE)})
    finally:
        eng.close()


# ---- b. a bound, the setters, the slots they keep ------------------------------------------------------------------------------
@pytest.mark.parametrize('i,route', PAIRS, ids=PAIR_IDS)
def test_bound_is_held_and_setters_keep_the_slots(i, route):
    """The scenario of lc.bound_scenario: while Adam64's unclamped value lies beyond the bound by more than the bar the engine
    holds float32(bound) bit for bit (Follower.check), the slots go on while it does (steps 3..5 are within the bar of an Adam64
    whose slots did), the value setters after step 5 invalidate the snapshot and keep the slots (steps 6..8 within the bar); the
    variants (f) and (g) leave the bar on steps 6..8."""
    tag = 'bound/' + PAIR_IDS[PAIRS.index((i, route))]
    scn = lc.bound_scenario(i)
    eng = build(i, route, [lc.whole(i)], bounds=scn, lr=lc.engine_lr(i, 'bound'))
    try:
        f = Follower(tag, i, bounds=scn)
        vals = read(eng)[0]
        for t in range(1, lc.K + 1):
            if t == lc.SET_AFTER + 1:
                for k in lc.VECTORS:
                    eng.state_snapshot()
                    getattr(eng, SET[k])(lc.initial(i)[k])
                    with pytest.raises(VNError, match='error 3: no snapshot to roll back to'):
                        eng.state_rollback()
                f.on_set()
                vals = read(eng)[0]
                assert eng.step == lc.SET_AFTER and all(np.array_equal(vals[k], ar.f32(lc.initial(i)[k])) for k in lc.VECTORS)
            one_step(eng, t)
            vals = f.check(eng, t, vals)
        for k in lc.VECTORS:
            entry, side, bound = scn[k]
            t0, held = lc.first_bound_step(f.steps[k], entry, bound)
            print('%s %s: entry %d on its bound %.9g from step %s for %d steps' % (tag, k, entry, bound, t0, held))
            assert t0 is not None and t0 >= 2 and held >= 3 and t0 + held - 1 == lc.SET_AFTER, (tag, k, t0, held)   # (as planned)
        late = {k: np.ones(lc.SIZE[k], dtype=bool) for k in lc.VECTORS}
        seen = f.variants(['f_setter_zeroes_slots', 'g_slots_frozen_on_bound'], late, lc.SET_AFTER + 1)
        f.record({'variants_bars_from_engine': seen})
    finally:
        eng.close()


# ---- c. two batches --------------------------------------------------------------------------------------------------------
def evaluate(eng, gb, batch):
    eng.grad(batch)
    return (gb.cpu().numpy().copy(),) + tuple(read(eng)[1][k] for k in lc.VECTORS)


@pytest.mark.parametrize('i,route', PAIRS, ids=PAIR_IDS)
def test_two_batches_share_the_vectors(i, route):
    """Batches of 9 + 15 (case 6: 36 + 41) test functions, the second without a reaction term.  The gradient readers return the
    last evaluation's batch; each vector's gradient on each batch meets its fp64 reference within the vector's own bar, the
    reaction coefficients' on batch 1 read exactly 0; an epoch over the schedule is its single steps; the single steps follow
    Adam64, and on the batch-1 steps the reaction coefficients move by their momentum (variant (e) leaves the bar); snapshot
    after step 3, rollback after step 6, and the replayed steps end in the same bits.  A ninth step on batch 1 with both bases
    cleared: the amplitude gradients read exactly 0 and the amplitudes move by their momentum as Adam64 says."""
    tag = 'two/' + PAIR_IDS[PAIRS.index((i, route))]
    a, b = build(i, route, lc.split(i)), build(i, route, lc.split(i))
    try:
        gb = a.bind_grad_buffer()
        first, second, third = evaluate(a, gb, 0), evaluate(a, gb, 1), evaluate(a, gb, 0)
        assert same(first, third), tag
        assert not any(np.array_equal(p, q) for p, q in zip(first, second)), tag
        grad_rec = {}
        for which, got in ((0, first), (1, second)):
            ref = lc.reference64(i, which)
            for n, k in enumerate(lc.VECTORS):
                g64, S = ref[k]
                bar = lc.BARS[k](g64, S)
                err = np.abs(got[1 + n] - g64)
                live = bar > 0.0
                grad_rec['batch%d/%s' % (which, k)] = float(np.max(err[live] / bar[live]))
                print('%s batch %d %s gradient: err/bar %.3f' % (tag, which, k, grad_rec['batch%d/%s' % (which, k)]))
                assert np.all(err <= bar), (tag, which, k, got[1 + n], g64, bar)
        assert np.all(second[1][:3] == 0.0) and np.all(second[1][3:] != 0.0) and np.all(first[1] != 0.0), tag
        assert a.step == 0 and same(state(a), state(b)), tag                        # (evaluations move nothing)

        a.train_epoch(list(lc.SCHEDULE))
        f = Follower(tag, i)
        vals = read(b)[0]
        s3 = s6 = None
        for t, which in enumerate(lc.SCHEDULE, 1):
            b.train_step(which)
            vals = f.check(b, t, vals, which)
            if t == 3:
                s3 = state(b)
                b.state_snapshot()
            if t == 6:
                s6 = state(b)
                b.state_rollback()
                assert same(state(b), s3) and b.step == 3, tag
                for w in lc.SCHEDULE[3:6]:
                    b.train_step(w)
                assert same(state(b), s6) and not same(s6, s3), tag
        assert same(state(a), state(b)) and b.step == lc.K, tag

        # a ninth step on batch 1 without its bases: nothing to reduce (one zeroed partial row stands in), the slots are not zero
        b.set_source_basis(1, None)
        b.set_field_basis(1, None)
        b.train_step(1)
        moved = f.check(b, lc.K + 1, vals, 1)
        for k in ('source', 'field'):
            assert np.all(f.steps[k][-1]['g'] == 0.0) and np.all(moved[k] != vals[k]), (tag, k)
        last = {k: (np.arange(lc.K + 1) == lc.K)[:, None] & np.ones(lc.J, dtype=bool) for k in ('source', 'field')}
        no_basis = f.variants(['e_zero_gradient_skipped'], last)

        steps = f.steps['coef']
        on_b1 = np.array([s['batch'] == 1 for s in steps])
        assert list(on_b1) == [w == 1 for w in lc.SCHEDULE] + [True]
        for s in steps:
            if s['batch'] == 1:
                assert np.all(s['g'][:3] == 0.0) and np.all(s['after'][:3] != s['before'][:3]), (tag, s['t'])
        pick = {'coef': on_b1[:, None] & (np.arange(9) < 3)}
        seen = dict(f.variants(['e_zero_gradient_skipped'], pick), **no_basis)
        f.record({'gradient_err_over_bar': grad_rec, 'variants_bars_from_engine': seen})
    finally:
        a.close()
        b.close()
