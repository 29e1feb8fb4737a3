"""
CPU tier of the learnt vectors' step: tests/learnt_adam_ref.Adam64 against the project's oracle (oracle.tf1_graph.TF1Adam), the
bar of tests/learnt_adam_ref.bar measured again on every sequence of tests/learnt_cases.py, that each named wrong variant of the
step leaves that bar by a factor of ten at least on those sequences (so the GPU tier, which runs them, would fail on a device that
had the slip), the conditions the bound scenario has to meet, and the input conditions of the two-batch cut -- all from CPU numbers.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests import inverse_cases as ic
from tests import learnt_adam_ref as ar
from tests import learnt_cases as lc
from tests import source_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = dict(zip(lc.CASES, lc.IDS))
FACTOR = 10.0                    # a variant has to leave the bar by this much


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_adam64_is_the_oracle_plus_mask_and_clamp():
    """All entries masked, infinite bounds, unrounded hyper-parameters: Adam64 is TF1Adam in fp64 over 8 steps to 1e-15 relative.
    Then a mask and bounds: unmasked entries and their slots are untouched, masked ones are the clamped oracle step."""
    rng = np.random.default_rng(7)
    n = 12
    x0 = rng.standard_normal(n)
    gs = [rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n) for _ in range(8)]
    oracle, mine = og.TF1Adam(n, lr=0.02, dtype=np.float64), ar.Adam64(n, None, 0.02, rounded=False)
    xo, xm = x0.copy(), x0.copy()
    for t, g in enumerate(gs, 1):
        xo, xm = oracle.step(xo, g), mine.step(xm, g, t)
        assert np.all(np.abs(xm - xo) <= 1e-15 * np.abs(xo)), (t, xm, xo)
        assert np.all(np.abs(mine.m - oracle.m) <= 1e-15 * np.abs(oracle.m)) and np.all(np.abs(mine.v - oracle.v) <= 1e-15 * oracle.v)
    mask = np.arange(n) % 3 != 1
    lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
    lo[[0, 3]], hi[[0, 3]] = x0[[0, 3]] - 0.01, x0[[0, 3]] + 0.01
    oracle, mine = og.TF1Adam(n, lr=0.02, dtype=np.float64), ar.Adam64(n, mask, 0.02, lo, hi, rounded=False)
    x, hit = x0.copy(), 0
    for t, g in enumerate(gs, 1):
        free = oracle.step(x, g)
        x1 = mine.step(x, g, t)
        assert np.array_equal(x1[~mask], x[~mask]) and np.all(mine.m[~mask] == 0.0) and np.all(mine.v[~mask] == 0.0)
        want = np.minimum(np.maximum(free, lo), hi)
        assert np.all(np.abs(x1[mask] - want[mask]) <= 1e-15 * np.abs(want[mask])), t
        assert np.all(np.abs(mine.m[mask] - oracle.m[mask]) <= 1e-15 * np.abs(oracle.m[mask]))        # the clamp does not stop the slots
        x = np.where(mask, x1, free)                                                                   # (the oracle steps every entry)
        hit += int(np.sum((x == lo) | (x == hi)))
    assert hit >= 2                                                                                    # (bounds were reached)


def test_rounded_hyper_parameters_are_those_of_the_first_step_tests():
    """From zero slots Adam64 gives the formula of test_train_step_is_adam_on_the_masked_*: lr_t, beta1, beta2, eps in fp32."""
    g = np.array([3.5, -1e-3, 77.0])
    x = np.array([0.25, -1.0, 2.0])
    b1, b2, eps = (float(np.float32(v)) for v in (0.9, 0.999, 1e-8))
    for t in (1, 2):
        lr_t = float(np.float32(0.1 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)))
        gi = g.astype(np.float32).astype(np.float64)
        want = x - lr_t * ((1 - b1) * gi) / (np.sqrt((1 - b2) * gi * gi) + eps)
        assert np.allclose(ar.Adam64(3, None, 0.1).step(x, g, t), want, rtol=1e-15, atol=0.0)


# ---- the bar -----------------------------------------------------------------------------------------------------------------
def measure():
    """{(case, kind, vector): the largest (|Adam32 - Adam64| - ulp / 2) / lr_t over the steps}, Adam32 running on its own values
    and Adam64 started from them at each step."""
    out = {}
    for i, kind, k, steps, lo, hi in lc.sequences():
        n = lc.SIZE[k]
        a32, a64 = ar.Adam32(n, None, lc.LR, lo, hi), ar.Adam64(n, None, lc.LR, lo, hi)
        x = np.asarray(steps[0]['before'], dtype=np.float32)
        worst = 0.0
        for s in steps:
            if s['set']:
                x = np.asarray(lc.initial(i)[k], dtype=np.float32)
            before = x.astype(np.float64)
            want = a64.step(before, s['g'], s['t'])
            x = a32.step(x, s['g'], s['t'])
            over = (np.abs(x.astype(np.float64) - want) - ar.bar(before, want, 0.0, c=0.0)) / a64.lr_t(s['t'])
            worst = max(worst, float(over.max()))
        out[(i, kind, k)] = worst
    return out


def test_the_bar_is_the_measured_one():
    """Adam32 stays within the bar on every sequence (by the factor), and the constant is the factor times the largest measured
    excess: a change of the cases, of the kernels' restatement or of the constant shows here."""
    got = measure()
    for key, w in got.items():
        print('Adam32 - Adam64, %s %s %s: (err - ulp/2) / lr_t %.4e' % (CASE_IDS[key[0]], key[1], key[2], w))
    worst = max(got.values())
    print('measured C %r, constant %r, factor %g' % (worst, ar.MEASURED_C, ar.C_FACTOR))
    assert worst > 0.0
    assert ar.MEASURED_C == pytest.approx(worst, rel=1e-9)
    assert ar.C == ar.C_FACTOR * ar.MEASURED_C and ar.C_FACTOR == 4.0
    with open(os.path.join(ROOT, 'profiles', 'learnt_adam_parity.json')) as f:
        rec = json.load(f)
    assert rec['cpu']['measured_C'] == ar.MEASURED_C and rec['cpu']['factor'] == ar.C_FACTOR and rec['cpu']['C'] == ar.C


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------
def _worst(name, steps, n, lo, hi, pick=None):
    """The largest err / bar of a variant over the steps t >= 2 (`pick`: over those steps and entries only)."""
    r = ar.replay(ar.MUTANTS.get(name) or ar.NOT_ASSERTED[name], steps, n, None, lc.LR, lo, hi)
    keep = np.array([s['t'] >= 2 for s in steps])[:, None] & np.ones(n, dtype=bool)
    if pick is not None:
        keep &= pick
    return float(np.max(np.where(keep, r, 0.0)))


@pytest.mark.parametrize('i', lc.CASES, ids=lc.IDS)
def test_every_sequence_sees_the_variants_of_the_recurrence(i):
    """(a) - (d), (h): on every (kind, vector) sequence some entry leaves the bar by the factor at some step >= 2."""
    for ii, kind, k, steps, lo, hi in lc.sequences():
        if ii != i:
            continue
        for name in ar.ANY_SEQUENCE:
            w = _worst(name, steps, lc.SIZE[k], lo, hi)
            print('%s %s %s: %s leaves the bar by %.3g' % (lc.IDS[lc.CASES.index(i)], kind, k, name, w))
            assert w >= FACTOR, (kind, k, name, w)
        print('%s %s %s: h_every_step (not asserted: Adam does not see it) %.3g of the bar'
              % (lc.IDS[lc.CASES.index(i)], kind, k, _worst('h_every_step', steps, lc.SIZE[k], lo, hi)))


@pytest.mark.parametrize('i', lc.CASES, ids=lc.IDS)
def test_two_batches_see_a_skipped_zero_gradient(i):
    """(e): on the batch-1 steps of the schedule the reaction coefficients have gradient 0 (exactly, in the reference) and non-zero
    momentum; a step that skipped them leaves the bar by the factor."""
    steps = lc.trajectory(i, 'two')['coef']
    b1 = [s for s in steps if s['batch'] == 1]
    assert [s['batch'] for s in steps] == list(lc.SCHEDULE) and len(b1) == 4
    assert all(np.all(s['g'][:3] == 0.0) and np.all(s['g'][3:] != 0.0) for s in b1)
    assert all(np.all(s['g'] != 0.0) for s in steps if s['batch'] == 0)
    pick = np.array([s['batch'] == 1 for s in steps])[:, None] & (np.arange(9) < 3)
    w = _worst('e_zero_gradient_skipped', steps, 9, None, None, pick)
    print('%s two coef: e_zero_gradient_skipped leaves the bar by %.3g' % (CASE_IDS[i], w))
    assert w >= FACTOR
    for s in b1:
        assert np.all(s['after'][:3] != s['before'][:3])                    # they move


@pytest.mark.parametrize('i', lc.CASES, ids=lc.IDS)
def test_bound_scenario_meets_its_conditions_and_sees_the_setter_variants(i):
    """Every vector's bound is first reached at a step >= 2 (the unclamped value lies beyond it by more than the bar), holds for two
    further steps at least, and the setter takes the value off it; (f) and (g) leave the bar by the factor on steps 6..8."""
    sc_ = lc.bound_scenario(i)
    for k in lc.VECTORS:
        entry, side, bound = sc_[k]
        steps = lc.trajectory(i, 'bound')[k]
        n = lc.SIZE[k]
        lo, hi = lc.bounds_of(sc_, k)
        assert bound == float(np.float32(bound))
        t0, held = lc.first_bound_step(steps, entry, bound)
        print('%s bound %s: entry %d %s %.9g, reached at step %s, held %d steps' % (CASE_IDS[i], k, entry, side, bound, t0, held))
        assert t0 is not None and 2 <= t0 and held >= 3 and t0 + held - 1 <= lc.SET_AFTER, (k, t0, held)
        for s in steps[t0 - 1:t0 - 1 + held]:
            beyond = (bound - s['unclamped'][entry]) if side == 'lo' else (s['unclamped'][entry] - bound)
            assert beyond > ar.bar(s['before'][entry], bound, ar.lr_t_of(lc.LR, s['t'])), (k, s['t'], beyond)
        assert [s['set'] for s in steps] == [False] * lc.SET_AFTER + [True] + [False] * (lc.K - lc.SET_AFTER - 1)
        assert steps[lc.SET_AFTER - 1]['after'][entry] == bound and steps[lc.SET_AFTER]['before'][entry] != bound
        assert np.array_equal(steps[lc.SET_AFTER]['before'], lc.initial(i)[k])
        late = np.array([s['t'] > lc.SET_AFTER for s in steps])[:, None]
        for name in ('f_setter_zeroes_slots', 'g_slots_frozen_on_bound'):
            w = _worst(name, steps, n, lo, hi, late)
            print('%s bound %s: %s leaves the bar by %.3g on steps 6..8' % (CASE_IDS[i], k, name, w))
            assert w >= FACTOR, (k, name, w)


# ---- the two batches' references -----------------------------------------------------------------------------------------------
def test_split_is_the_case_cut_in_two():
    for i in lc.CASES:
        w, (a, b) = lc.whole(i), lc.split(i)
        q = sc.case(i)[3]
        assert a['n_k'] == lc.N_A[i] and a['n_k'] + b['n_k'] == w['n_k']
        for key in lc.SLICED + ('s0',):
            if w[key] is not None:
                assert np.array_equal(np.concatenate([a[key], b[key]]), w[key]), key
        assert np.array_equal(np.concatenate([a['Phi'], b['Phi']], axis=1), w['Phi'])
        assert np.array_equal(np.concatenate([a['G'], b['G']], axis=1), w['G'])
        for d in (a, b):
            assert d['Xu'] is w['Xu'] and d['rowptr'].size == w['Xu'].shape[0] + 1 and d['rowptr'][-1] == d['n_k'] * q
            assert np.array_equal(np.sort(d['rowidx']), np.arange(d['n_k'] * q))
            assert np.all(d['uid'][d['rowidx']] == np.repeat(np.arange(w['Xu'].shape[0]), np.diff(d['rowptr'])))
        assert a['reaction'] and not b['reaction']
    rows = lambda i: [d['n_k'] * sc.case(i)[3] for d in lc.split(i)]
    assert rows(0) == [576, 960] and rows(6) == [216, 246] and rows(6)[0] % 4 == 0 and rows(6)[1] % 4 == 2


def test_two_batch_references_meet_the_sibling_conditions():
    """What tests/test_inverse_host.py, tests/test_source_host.py and tests/test_field_host.py assert of their cases, for the cut
    ones: every component a term of the batch reaches is non-zero, the reference evaluated in fp32 on the CPU stays within the
    vector's bar, and the conditioning floor is the binding branch for no more than the siblings' share of the components."""
    share = {'coef': ic.BINDING_CAP / 90.0, 'source': sc.BINDING_FRAC, 'field': lc.fc.BINDING_FRAC}
    binding = {k: [] for k in lc.VECTORS}
    total = {k: 0 for k in lc.VECTORS}
    for i in lc.CASES:
        for which in (0, 1):
            r64 = lc.reference64(i, which)
            r32 = lc.gradients(i, which, sc.theta(i), lc.initial(i), torch.float32)
            for k in lc.VECTORS:
                g64, S = r64[k]
                live = np.ones(g64.size, dtype=bool)
                if k == 'coef' and which == 1:
                    live[:3] = False
                    assert np.all(g64[:3] == 0.0) and np.all(S[:3] == 0.0) and np.all(r32[k][0][:3] == 0.0)
                assert np.all(g64[live] != 0.0) and np.all(S[live] > 0.0), (i, which, k)
                bar = lc.BARS[k](g64, S)
                rel = np.abs(r32[k][0] - g64)[live] / bar[live]
                print('%s batch %d %s: fp32 restatement worst err/bar %.3f' % (CASE_IDS[i], which, k, rel.max()))
                assert np.all(rel <= 1.0), (i, which, k, rel)
                total[k] += int(live.sum())
                binding[k] += [(CASE_IDS[i], which, int(m), abs(g64[m]) / S[m]) for m in np.flatnonzero(live)
                               if abs(g64[m]) < 0.01 * S[m]]
    for k in lc.VECTORS:
        print('%s: floor binding %d of %d' % (k, len(binding[k]), total[k]), binding[k])
        assert len(binding[k]) <= share[k] * total[k], (k, binding[k])
