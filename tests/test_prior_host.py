"""
CPU tier of the learnt vectors' regularisation (`VarNet(learntPrior=...)`, vn_set_learnt_prior): the matrix builders, every
validation sentence of the option, the step bar's constant measured again on the shrinkage sequences of tests/prior_cases.py, that
the sequences meet the conditions they were built for (prior and data gradient of comparable size, a bound reached, an entry
shrunk to exactly zero), and that each named wrong variant of tests/prior_ref.MUTANTS leaves a bar on them -- all from CPU numbers.
"""
import json
import os

import numpy as np
import pytest

from tests import learnt_adam_ref as ar
from tests import prior_cases as pc
from tests import prior_ref as pr
from varnet_amd.varnet import VarNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = {lv.stem: lv for lv in VarNet.LEARNT}


# ---- builders ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3, 9, 64])
def test_difference_annihilates_constants_and_is_psd(n):
    for R in (VarNet.priorMatrix('difference', n), pr.difference(n)):
        assert R.shape == (n, n) and np.array_equal(R, R.T)
        assert np.all(R @ np.ones(n) == 0.0)
        assert np.linalg.eigvalsh(R)[0] >= -1e-12
        a = np.arange(n, dtype=np.float64) ** 2
        assert a @ R @ a == pytest.approx(float(np.sum(np.diff(a) ** 2)))
    assert np.array_equal(VarNet.priorMatrix('difference', n), pr.difference(n))
    assert np.array_equal(VarNet.priorMatrix('identity', n), np.eye(n))


def _learnt(**kw):
    """The parsed registrations priorData takes: {stem: data or None}."""
    out = {s: None for s in ROW}
    out.update(kw)
    return out


SOURCE = dict(init=np.array([1.0, -2.0, 0.5]), mask=[1, 1, 0])
FIELD = dict(init=np.array([1.0, 2.0, 3.0, -1.0, 0.25]), mask=[1] * 5, Jk=3, Jv=2)


def test_defaults_and_the_unkeyed_block():
    got = VarNet.priorData(None, {'source': {'weight': 2.0, 'l1': 0.5}}, _learnt(source=SOURCE))
    b = got['source']['blocks'][None]
    assert b['weight'] == 2.0 and np.array_equal(b['R'], np.eye(3)) and np.array_equal(b['mean'], SOURCE['init'])
    assert np.array_equal(b['l1'], [0.5] * 3)
    w, R, mean, l1 = VarNet.priorArrays(ROW['source'], got['source']['blocks'], SOURCE)
    assert w == 2.0 and R is None and np.array_equal(mean, SOURCE['init']) and np.array_equal(l1, [0.5] * 3)
    assert VarNet.priorData(None, None, _learnt()) == {}
    # an explicit matrix that is symmetric to rounding is taken, exactly symmetrised
    A = pr.random_psd(np.random.default_rng(0), 3)
    A2 = A.copy()
    A2[0, 1] += 1e-15
    b = VarNet.priorData(None, {'source': {'weight': 1.0, 'matrix': A2, 'mean': [0, 0, 1]}}, _learnt(source=SOURCE))['source']['blocks'][None]
    assert np.array_equal(b['R'], b['R'].T) and np.allclose(b['R'], A, rtol=0, atol=1e-15) and np.array_equal(b['mean'], [0, 0, 1])


def test_keyed_specs_give_block_diagonal_matrices():
    spec = {'field': {'diff': {'weight': 3.0, 'matrix': 'difference'}, 'vel': {'weight': 0.5, 'l1': [0.0, 2.0], 'mean': [0.0, 0.0]}}}
    blocks = VarNet.priorData(None, spec, _learnt(field=FIELD))['field']['blocks']
    w, R, mean, l1 = VarNet.priorArrays(ROW['field'], blocks, FIELD)
    assert w == 1.0
    assert np.array_equal(R, pr.block_diag([3.0 * pr.difference(3), 0.5 * np.eye(2)]))
    assert np.all(R[:3, 3:] == 0.0) and np.all(R[3:, :3] == 0.0)
    assert np.array_equal(mean, [1.0, 2.0, 3.0, 0.0, 0.0]) and np.array_equal(l1, [0.0, 0.0, 0.0, 0.0, 2.0])
    # a key left out gets a zero block
    blocks = VarNet.priorData(None, {'field': {'vel': {'weight': 2.0}}}, _learnt(field=FIELD))['field']['blocks']
    w, R, mean, l1 = VarNet.priorArrays(ROW['field'], blocks, FIELD)
    assert w == 1.0 and np.array_equal(R, pr.block_diag([np.zeros((3, 3)), 2.0 * np.eye(2)])) and l1 is None
    assert np.array_equal(mean, [0.0, 0.0, 0.0, -1.0, 0.25])
    # no weight anywhere: nothing quadratic is registered
    blocks = VarNet.priorData(None, {'field': {'diff': {'l1': 1.0}}}, _learnt(field=FIELD))['field']['blocks']
    w, R, mean, l1 = VarNet.priorArrays(ROW['field'], blocks, FIELD)
    assert w == 0.0 and np.array_equal(l1, [1.0, 1.0, 1.0, 0.0, 0.0])


def test_stems_are_a_field_of_the_learnt_table():
    assert [lv.stem for lv in VarNet.LEARNT] == ['coef', 'source', 'field', 'bic', 'fluxBC']
    assert [lv.kind for lv in VarNet.LEARNT] == ['coef', 'source', 'field', 'bic', 'fluxbc']


INDEFINITE = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
ASYMMETRIC = np.array([[1.0, 0.5, 0.0], [0.25, 1.0, 0.0], [0.0, 0.0, 1.0]])
REFUSALS = [
    ({'sources': {'weight': 1.0}}, _learnt(source=SOURCE), r"learntPrior: unknown stem 'sources' \(one of coef, source, field, bic, fluxBC\)"),
    ({'bic': {'bc': {'weight': 1.0}}}, _learnt(source=SOURCE), r"learntPrior\['bic'\]: this instance does not learn that vector \(learnBic=\.\.\.\)"),
    ({'source': {'weight': 1.0, 'matrix': np.eye(4)}}, _learnt(source=SOURCE),
     r"learntPrior\['source'\]: matrix must be 3 x 3 finite numbers \(one row per amplitude\), got shape \(4, 4\)"),
    ({'source': {'weight': 1.0, 'mean': [0.0, 1.0]}}, _learnt(source=SOURCE),
     r"learntPrior\['source'\]: mean must be 3 finite numbers \(one per amplitude\), got \[0\.0, 1\.0\]"),
    ({'source': {'l1': [1.0] * 4}}, _learnt(source=SOURCE), r"learntPrior\['source'\]: l1 must be a number or 3 finite numbers"),
    ({'source': {'weight': 1.0, 'matrix': ASYMMETRIC}}, _learnt(source=SOURCE),
     r"learntPrior\['source'\]: matrix is not symmetric \(entry \((0, 1|1, 0)\) = "),
    ({'source': {'weight': 1.0, 'matrix': INDEFINITE}}, _learnt(source=SOURCE),
     r"learntPrior\['source'\]: matrix is indefinite \(smallest eigenvalue -1\.0"),
    ({'source': {'weight': -1.0}}, _learnt(source=SOURCE), r"learntPrior\['source'\]: weight -1\.0 is negative"),
    ({'source': {'l1': [0.0, -0.5, 0.0]}}, _learnt(source=SOURCE), r"learntPrior\['source'\]: l1 weight -0\.5 is negative"),
    ({'source': {'weight': 1.0, 'matrix': 'laplace'}}, _learnt(source=SOURCE), r"matrix must be 'identity', 'difference' or a symmetric"),
    ({'source': {'alpha': 1.0}}, _learnt(source=SOURCE), r"learntPrior\['source'\] must be a dict with keys among weight, matrix, mean, l1"),
    ({'field': {'weight': 1.0}}, _learnt(field=FIELD), r"learntPrior\['field'\] must be a dict by key \{'diff': spec, 'vel': spec\}"),
    ({'field': {'vel': {'weight': -2.0}}}, _learnt(field=FIELD), r"learntPrior\['field'\]\['vel'\]: weight -2\.0 is negative"),
    ({'field': {'diff': {'weight': 1.0, 'matrix': np.eye(5)}}}, _learnt(field=FIELD),
     r"learntPrior\['field'\]\['diff'\]: matrix must be 3 x 3 finite numbers"),
    ({'field': {'vel': {'weight': 1.0}}}, _learnt(field=dict(FIELD, init=FIELD['init'][:3], Jv=0)),
     r"learntPrior\['field'\]\['vel'\]: the PDE has no vel basis"),
    ([('source', {})], _learnt(source=SOURCE), r"learntPrior must be a dict \{stem: spec\} with stems among"),
]


@pytest.mark.parametrize('spec,learnt,sentence', REFUSALS, ids=[r[2][:48].replace('\\', '') for r in REFUSALS])
def test_every_refusal_of_the_option_has_its_sentence(spec, learnt, sentence):
    with pytest.raises(ValueError, match=sentence):
        VarNet.priorData(None, spec, learnt)


# ---- the bar -----------------------------------------------------------------------------------------------------------------
def measure():
    """{tag: the largest (|Adam32Prox - Adam64Prox| - ulp / 2) / lr_t over the steps}: Adam32Prox running on its own values,
    Adam64Prox started from them at each step, both on data gradient + the prior's gradient at those values (fp64)."""
    out = {}
    for cfg, steps in pc.sequences():
        p = cfg['prior']
        a32 = pr.Adam32Prox(cfg['n'], cfg['mask'], pc.LR, cfg['lo'], cfg['hi'], p.l1)
        a64 = pr.Adam64Prox(cfg['n'], cfg['mask'], pc.LR, cfg['lo'], cfg['hi'], l1=p.l1)
        x = np.asarray(cfg['start'], dtype=np.float32)
        worst = -np.inf
        for s in steps:
            before = x.astype(np.float64)
            g = np.where(cfg['mask'], s['g_data'] + p.grad_all(before), 0.0)
            want = a64.step(before, g, s['t'])
            x = a32.step(x, g, s['t'])
            excess = (np.abs(x.astype(np.float64) - want) - ar.bar(before, want, 0.0, c=0.0)) / a64.lr_t(s['t'])
            worst = max(worst, float(excess.max()))
        out[cfg['tag']] = worst
    return out


def test_the_bar_is_the_measured_one():
    got = measure()
    for tag, w in got.items():
        print('Adam32Prox - Adam64Prox, %s: (err - ulp/2) / lr_t %.4e' % (tag, w))
    worst = max(got.values())
    print('measured C_prior %r, constant %r; C of the plain step %r; factor %g' % (worst, pr.MEASURED_C_PRIOR, ar.MEASURED_C, ar.C_FACTOR))
    assert worst > 0.0
    assert pr.MEASURED_C_PRIOR == pytest.approx(worst, rel=1e-9)
    assert pr.C == 4.0 * max(ar.MEASURED_C, pr.MEASURED_C_PRIOR) and ar.C_FACTOR == 4.0
    with open(os.path.join(ROOT, 'profiles', 'prior_parity.json')) as f:
        rec = json.load(f)
    assert rec['cpu']['measured_C_prior'] == pr.MEASURED_C_PRIOR and rec['cpu']['measured_C'] == ar.MEASURED_C
    assert rec['cpu']['factor'] == ar.C_FACTOR and rec['cpu']['C'] == pr.C


# ---- the sequences and the variants ----------------------------------------------------------------------------------------------
def test_sequences_meet_the_conditions_they_were_built_for():
    tags = [cfg['tag'] for cfg, _ in pc.sequences()]
    assert tags == ['lc0/coef', 'lc0/source', 'lc0/field', 'lc6/coef', 'lc6/source', 'lc6/field', 'fbc/1+0', 'fbc/5+4', 'fbc/37+27',
                    'fbc/40+24', 'bic/3']
    assert [cfg['n'] for cfg, _ in pc.sequences()] == [9, 3, 3, 9, 3, 3, 1, 9, 64, 64, 3]
    for cfg, steps in pc.sequences():
        p, on = cfg['prior'], cfg['mask']
        assert len(steps) == pc.K and [s['after_grad'] for s in steps] == [False, True] * 4
        # dense matrix, non-zero mean, and a prior Adam can see: within a factor 10 of the data gradient's norm at every step
        assert np.all(p.R != 0.0) and np.all(p.mean != 0.0) and p.weight > 0.0
        for s in steps:
            ratio = np.linalg.norm(p.grad(s['before'])[on]) / np.linalg.norm(s['g_data'][on])
            print('%s step %d: |weight R d| / |data gradient| = %.3f' % (cfg['tag'], s['t'], ratio))
            assert 1.0 / pc.RATIO <= ratio <= pc.RATIO, (cfg['tag'], s['t'], ratio)
        # the bounded entry reaches one of its bounds (J >= 3: at the first step), with Adam's value beyond it by more than the bar
        e = cfg['bounded']
        hit = [s for s in steps if s['after'][e] in (cfg['lo'][e], cfg['hi'][e])]
        assert hit and (cfg['n'] < 3 or hit[0]['t'] == 1) and hit[0]['t'] < pc.K, (cfg['tag'], [s['after'][e] for s in steps])
        s = hit[0]
        beyond = max(cfg['lo'][e] - s['unclamped'][e], s['unclamped'][e] - cfg['hi'][e])
        print('%s: entry %d reaches its bound %.9g at step %d' % (cfg['tag'], e, s['after'][e], s['t']))
        assert beyond > pr.bar(s['before'][e], s['after'][e], ar.lr_t_of(pc.LR, s['t'])), (cfg['tag'], beyond)
        # entries with l1 == 0 and l1 > 0 both, where there is room; the unmasked entry never moves
        if cfg['n'] > 3:
            assert np.any(p.l1[on] == 0.0) and np.any(p.l1[on] > 0.0)
        if cfg['n'] >= 3:
            assert all(s['after'][cfg['unmasked']] == cfg['start'][cfg['unmasked']] for s in steps)
            z = cfg['near_zero']
            assert abs(cfg['start'][z]) < ar.lr_t_of(pc.LR, 1) * p.l1[z]


def test_every_variant_leaves_a_bar_on_every_sequence_that_can_show_it():
    for cfg, steps in pc.sequences():
        clean = pr.replay(pr.Step64, steps, cfg['prior'], pc.LR, cfg['lo'], cfg['hi'])
        assert np.all(clean == 0.0), cfg['tag']                                    # (the restatement replays itself)
        for name, cls in pr.MUTANTS.items():
            w = float(np.max(pr.replay(cls, steps, cfg['prior'], pc.LR, cfg['lo'], cfg['hi'])))
            print('%s: %s is %.3g bars from the restatement%s' % (cfg['tag'], name, w, '' if pc.shows(cfg, name) else ' (not asserted)'))
            if pc.shows(cfg, name):
                assert w > 1.0, (cfg['tag'], name, w)
    assert set(pr.NEEDS) <= set(pr.MUTANTS) and len(pr.MUTANTS) == 9
