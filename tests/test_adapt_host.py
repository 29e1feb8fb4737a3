"""
CPU tier of the self-adaptive test-function weights (vn_set_tf_adapt, vn_get_tf_adapt, vn_set_tf_adapt_state,
`VarNet(tfAdapt=...)`): the properties of the two rules in the fp64 restatement (tests/adapt_ref.py), the
cases' weights (a real part of what the GPU tier compares), the measured single-update bar, the option's parsing and the layout
of par[10], the declaration and binding of the three entry points, and the host layer of `VarNet` through a stand-in engine:
registration of every batch, the state carried across a monitor's borrowing of the engine, the refusals, `setTfAdapt`, and the
caseData.txt line.
"""
import json
import os
import re

import numpy as np
import pytest

from tests import adapt_ref
from tests.adapt_cases import (CASES, DEVICE_ULPS, IDS, RULES, SINGLE_CASES, ULP32, lambda0, parity_spec, reference64, single_update_bar,
                               spec_of, weights_are_real)
from tests.oracle_engine import OracleEngine
from varnet_amd import engine as vn_engine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import tf_adapt_par, tf_adapt_spec
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pi = np.pi


# ---- the rules ------------------------------------------------------------------------------------------------------------
def _fields(n, steps, seed=41):
    return np.random.default_rng(seed).uniform(0.0, 3.0, (steps, n)) ** 2


def test_rba_is_bounded_and_the_arg_max_gains_exactly_eta():
    for kw in ({}, {'gamma': 0.9, 'eta': 0.5}, {'gamma': 0.5, 'eta': 0.01, 'init': 3.0}):
        spec = adapt_ref.spec_of('rba', **kw)
        bound = adapt_ref.rba_bound(spec)
        lam, tau = np.full(50, spec['init']), 0
        for l in _fields(50, 200):
            new, _, tau = adapt_ref.update(lam, None, tau, l, spec)
            k = int(np.argmax(l))
            assert abs(new[k] - (spec['gamma'] * lam[k] + spec['eta'])) <= 1e-15     # r_k / r_max = 1 there
            assert np.all(new <= bound * (1 + 1e-15)) and np.all(new >= 0.0)
            lam = new
        assert tau == 200


def test_sa_is_monotone_and_clamps_at_cap():
    spec = adapt_ref.spec_of('sa', lr=0.5, cap=3.0)
    lam, slots, tau = np.ones(40), None, 0
    for l in _fields(40, 60):
        new, slots, tau = adapt_ref.update(lam, slots, tau, l + 1e-3, spec)
        assert np.all(new >= lam) and np.all(new <= 3.0)                 # ascent: g >= 0, so lambda never falls
        lam = new
    assert np.all(lam == 3.0) and tau == 60                              # ... and ends at the cap
    # power 1: g = l / lbar whatever lambda is
    spec1 = adapt_ref.spec_of('sa', power=1)
    a = adapt_ref.update(np.ones(5), None, 0, np.arange(1.0, 6.0), spec1)
    b = adapt_ref.update(np.full(5, 2.0), None, 0, np.arange(1.0, 6.0), spec1)
    np.testing.assert_allclose(a[1], b[1], rtol=0, atol=0)


@pytest.mark.parametrize('rule', RULES)
def test_normalize_gives_unit_mean_and_the_statistics_add_up(rule):
    lam = np.random.default_rng(42).uniform(0.0, 4.0, 77)
    for power in (1, 2):
        om, Z, st = adapt_ref.weights(lam, adapt_ref.spec_of(rule, power=power))
        assert abs(om.mean() - 1.0) <= 1e-14 and abs(st['mean'] - 1.0) <= 1e-14
        assert st['min'] == om.min() and st['max'] == om.max()
        assert abs(st['share'] - om.sum() ** 2 / (om.size * (om ** 2).sum())) <= 1e-14 and 0.0 < st['share'] <= 1.0
        om1, Z1, st1 = adapt_ref.weights(lam, adapt_ref.spec_of(rule, power=power, normalize=False))
        assert Z1 == 1.0 and np.array_equal(om1, lam ** power) and abs(st1['share'] - st['share']) <= 1e-14
    assert adapt_ref.weights(np.zeros(4), adapt_ref.spec_of(rule))[0].tolist() == [0.0] * 4      # all zero: omega 0, not 0 / 0
    assert adapt_ref.weights(np.ones(9), adapt_ref.spec_of(rule))[2]['share'] == 1.0


@pytest.mark.parametrize('rule', RULES)
def test_a_zero_or_non_finite_field_leaves_the_state_unchanged(rule):
    spec = adapt_ref.spec_of(rule)
    lam = np.random.default_rng(43).uniform(0.5, 2.0, 12)
    slots = None if rule == 'rba' else np.random.default_rng(44).uniform(0.0, 1.0, (2, 12))
    for l in (np.zeros(12), np.full(12, np.nan), np.where(np.arange(12) == 3, np.inf, 1.0)):
        new, s, tau = adapt_ref.update(lam, slots, 5, l, spec)
        assert np.array_equal(new, lam) and tau == 5
        assert s is None if rule == 'rba' else np.array_equal(s, slots)


def test_gamma_one_eta_zero_is_the_identity():
    spec = adapt_ref.spec_of('rba', gamma=1.0, eta=0.0, normalize=False)
    lam = np.ones(9)
    for l in _fields(9, 5):
        for f in (np.float64, np.float32):
            out = adapt_ref.step(lam.astype(f), None, 0, l, spec, dtype=f)
            assert np.all(out['lam'] == 1.0) and np.all(out['omega'] == 1.0) and out['Z'] == 1.0


# ---- the cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_the_cases_weights_are_real(i):
    weights_are_real(i)
    lam = lambda0(i)
    assert lam.dtype == np.float32 and lam.shape == (CASES[i][4],) and lam.min() >= 0.5 and lam.max() <= 2.0
    om = adapt_ref.weights(lam, parity_spec())[0]
    assert np.array_equal(om, lam.astype(np.float64) ** 2)
    assert reference64(i, True)[0]['lossVec'].reshape(-1).shape == lam.shape


def test_the_weights_are_real_with_all_three_terms_on_case_3():
    weights_are_real(3, 'terms')


@pytest.mark.parametrize('rule', RULES)
def test_single_update_bar_is_measured_and_recorded(rule):
    """fp32 against fp64 restatement on the cases' own inputs, plus the ulp allowance: a few 1e-7 to a few 1e-6, far below any
    change of the rule a test could miss; the committed record (profiles/adapt_parity.json) states the same figures."""
    b = single_update_bar(rule)
    measured = max(b['measured_lambda'], b['measured_omega'], b['measured_slots'])
    assert b['allowance_ulps'] == DEVICE_ULPS[rule] and abs(b['bar'] - (measured + 2 * DEVICE_ULPS[rule] * ULP32)) <= 1e-20
    assert 2.0 ** -25 <= measured <= 2e-6 and b['bar'] <= 5e-6, b
    assert len(SINGLE_CASES) == 6
    path = os.path.join(ROOT, 'profiles', 'adapt_parity.json')
    rec = json.load(open(path))['single_update_bar'][rule]
    assert rec['allowance_ulps'] == b['allowance_ulps'] and abs(rec['bar'] - b['bar']) <= 0.25 * b['bar'], (rec, b)
    # one step of the rule at twice the rate, or with the other power, lies far outside the bar
    spec = spec_of(0, rule)
    lam, l = lambda0(0).astype(np.float64), reference64(0, False)[0]['lossVec'].reshape(-1)
    key = 'eta' if rule == 'rba' else 'lr'
    a = adapt_ref.step(lam, None, 0, l, spec)['lam']
    c = adapt_ref.step(lam, None, 0, l, dict(spec, **{key: 2 * spec[key]}))['lam']
    assert np.max(np.abs(a - c) / a) > 100 * b['bar']


# ---- option parsing, par[10], declarations -------------------------------------------------------------------------------
def test_option_parsing_and_par_layout():
    assert tf_adapt_spec(None) is None
    rba, sa = tf_adapt_spec('rba'), tf_adapt_spec({'rule': 'sa'})
    assert rba == adapt_ref.RBA and sa == adapt_ref.SA
    assert tf_adapt_par(rba) == (1, [0.999, 0.01, 0.0, 0.0, 0.0, 2.0, 1.0, 1.0, 1.0, 0.0])
    assert tf_adapt_par(sa) == (2, [0.005, 1e3, 0.9, 0.999, 1e-8, 2.0, 1.0, 1.0, 1.0, 0.0])
    full = tf_adapt_spec({'rule': 'rba', 'gamma': 0.9, 'eta': 0.1, 'power': 1, 'init': 0.5, 'normalize': False, 'every': 10})
    assert tf_adapt_par(full) == (1, [0.9, 0.1, 0.0, 0.0, 0.0, 1.0, 0.5, 0.0, 10.0, 0.0])
    for bad, msg in (('adam', "rule must be 'rba' or 'sa'"), (3, "must be None, 'rba', 'sa' or a dict"), ({'gamma': 0.5}, 'rule must be'),
                     ({'rule': 'rba', 'lr': 0.1}, "a key of the 'sa' rule"), ({'rule': 'sa', 'eta': 0.1}, "a key of the 'rba' rule"),
                     ({'rule': 'rba', 'foo': 1}, 'no key of the adaptive weights'), ({'rule': 'rba', 'gamma': 1.5}, 'gamma must lie'),
                     ({'rule': 'rba', 'eta': -1}, 'eta be >= 0'), ({'rule': 'rba', 'power': 3}, 'power must be 1 or 2'),
                     ({'rule': 'sa', 'cap': 0}, 'cap > 0'), ({'rule': 'sa', 'beta2': 1.0}, 'beta1, beta2 in'),
                     ({'rule': 'sa', 'eps': 0}, 'eps > 0'), ({'rule': 'sa', 'every': 0}, 'every must be a whole number'),
                     ({'rule': 'sa', 'every': 2.5}, 'every must be a whole number'), ({'rule': 'rba', 'init': -1}, 'init must be >= 0'),
                     ({'rule': 'rba', 'eta': float('nan')}, 'must be finite')):
        with pytest.raises(ValueError, match=msg):
            tf_adapt_spec(bad)


def test_entry_points_are_declared_and_bound_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    for proto in (r'int vn_set_tf_adapt\(vn_engine\* h, int32_t batch, int32_t rule, const double par\[10\], const float\* lambda_init_dev\);',
                  r'int vn_get_tf_adapt\(vn_engine\* h, int32_t batch, float\* lambda_host, float\* omega_host, float\* slots_host, '
                  r'double stats\[6\]\);',
                  r'int vn_set_tf_adapt_state\(vn_engine\* h, int32_t batch, const float\* lambda_host, const float\* slots_host, '
                  r'int64_t tau\);'):
        assert re.search(proto, hdr), proto
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr)
    src = open(os.path.join(ROOT, 'varnet_amd', 'engine.py')).read()
    for name in ('vn_set_tf_adapt', 'vn_get_tf_adapt', 'vn_set_tf_adapt_state'):
        assert "'%s': (C.c_int" % name in src
    for meth in ('set_tf_adapt', 'tf_adapt', 'set_tf_adapt_state'):
        assert callable(getattr(vn_engine.VNEngine, meth))
    # the declarations stay out of vn_internal.h, which every kernel's source hash covers
    assert 'adapt' not in open(os.path.join(ROOT, 'varnet_amd', 'csrc', 'vn_internal.h')).read().lower()
    api = open(os.path.join(ROOT, 'varnet_amd', 'csrc', 'vn_api.hip')).read()
    assert 'VN_ADAPT_SPAN' in open(os.path.join(ROOT, 'varnet_amd', 'csrc', 'vn_adapt.h')).read() and '#include "vn_adapt.h"' in api


# ---- VarNet host layer through a stand-in engine ----------------------------------------------------------------------------
class AdaptOracleEngine(OracleEngine):
    """The oracle engine with the registration side of vn_set_tf_adapt: it keeps spec and state per batch (the loss itself stays
    the oracle's, unweighted: the host tests look at what is registered, carried and refused)."""

    def set_interior(self, batch, *a, **kw):
        super().set_interior(batch, *a, **kw)
        self.__dict__.setdefault('adapt', {}).pop(batch, None)           # vn_set_interior clears the registration

    def _n_k(self, batch):
        return self.batches[batch][3]

    def set_tf_adapt(self, batch, spec=None, lambda_init=None):
        spec = tf_adapt_spec(spec)
        reg = self.__dict__.setdefault('adapt', {})
        if spec is None:
            reg.pop(batch, None)
            return
        n = self._n_k(batch)
        reg[batch] = {'spec': spec, 'lambda': np.full(n, spec['init'], np.float32), 'tau': 0,
                      'slots': np.zeros((2, n), np.float32) if spec['rule'] == 'sa' else None}

    def adapt_batches(self):
        return sorted(getattr(self, 'adapt', {}))

    def tf_adapt(self, batch=0, arrays=True):
        r = self.adapt[batch]
        om, Z, st = adapt_ref.weights(r['lambda'], r['spec'], dtype=np.float32)
        st['tau'] = float(r['tau'])
        return {'lambda': r['lambda'].copy(), 'omega': om, 'slots': None if r['slots'] is None else r['slots'].copy(), 'stats': st}

    def set_tf_adapt_state(self, batch, lam, slots=None, tau=0):
        r = self.adapt[batch]
        r['lambda'], r['tau'] = np.asarray(lam, np.float32).copy(), int(tau)
        if r['slots'] is not None:
            r['slots'] = np.zeros_like(r['slots']) if slots is None else np.asarray(slots, np.float32).reshape(2, -1).copy()


@pytest.fixture
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return AdaptOracleEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                                 isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                                 learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


def _pde(**kw):
    return ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, vel=0.5, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x), **kw)


NET = dict(layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)


def test_every_batch_is_registered_and_the_state_is_carried(cpu_engine):
    vn = VarNet(_pde(), tfAdapt={'rule': 'sa', 'lr': 0.01}, **NET)
    assert vn.tfAdapt == adapt_ref.spec_of('sa', lr=0.01)
    eng = vn.engine
    td = vn._build_tdata(batchNum=3)
    assert eng.adapt_batches() == [0, 1, 2]
    sizes = [eng._n_k(b) for b in range(3)]
    assert sum(sizes) == vn.fixData.nt and all(eng.adapt[b]['spec']['lr'] == 0.01 for b in range(3))
    w = vn.tfWeights(td)
    assert [x['omega'].shape for x in w] == [(n,) for n in sizes] and all(x['stats']['tau'] == 0.0 for x in w)
    # the training set's state survives another set's use of the engine (a monitor on the uniform set) and comes back with it
    for b in range(3):
        eng.set_tf_adapt_state(b, np.full(sizes[b], 1.0 + b, np.float32), np.full((2, sizes[b]), 0.25, np.float32), 7 + b)
    other = vn._build_tdata()                                            # takes the engine: batch 0 is now the full set
    assert eng.adapt[0]['tau'] == 0 and np.all(eng.adapt[0]['lambda'] == 1.0) and eng._n_k(0) == vn.fixData.nt
    td.activate()
    for b in range(3):
        s = eng.tf_adapt(b)
        assert np.all(s['lambda'] == 1.0 + b) and np.all(s['slots'] == 0.25) and s['stats']['tau'] == 7.0 + b
    other.activate()
    assert eng.adapt[0]['tau'] == 0 and np.all(eng.adapt[0]['lambda'] == 1.0)
    # setTfAdapt: another rule from its initial state, then off
    vn.tData = td
    vn.setTfAdapt('rba')
    assert eng.adapt_batches() == [0, 1, 2] and all(eng.adapt[b]['spec']['rule'] == 'rba' and eng.adapt[b]['tau'] == 0 for b in range(3))
    vn.setTfAdapt(None)
    assert eng.adapt_batches() == [] and vn.tfAdapt is None
    with pytest.raises(ValueError, match='self-adaptive weights are off'):
        vn.tfWeights()


def test_case_file_and_history(cpu_engine, tmp_path):
    vn = VarNet(_pde(), tfAdapt={'rule': 'rba', 'every': 2}, **NET)
    res = vn.train(str(tmp_path), epochNum=4, tol=0.0, saveFreq=2, verbose=False, lossLag=0)
    case = open(os.path.join(str(tmp_path), 'caseData.txt')).read()
    assert 'Self-adaptive test-function weights: rule rba, eta = 0.01, every = 2, gamma = 0.999' in case
    assert [e for e, _ in res.tfAdaptHist] == [2, 4] and set(res.tfAdaptHist[0][1][0]) == {'min', 'max', 'mean', 'share', 'Z', 'tau'}
    arrays = vn.checkpoint_arrays()
    assert str(arrays['tfadapt_rule']) == 'rba' and list(arrays['tfadapt_batches']) == [0]
    assert arrays['tfadapt_0_lambda'].shape == (vn.fixData.nt,) and 'tfadapt_0_slots' not in arrays
    plain = VarNet(_pde(), **NET)
    assert not any(k.startswith('tfadapt') for k in plain.checkpoint_arrays())
    assert plain.train(str(tmp_path / 'plain'), epochNum=2, tol=0.0, saveFreq=1, verbose=False).tfAdaptHist == []


def test_refusals(cpu_engine, tmp_path):
    with pytest.raises(ValueError, match="a key of the 'sa' rule"):
        VarNet(_pde(), tfAdapt={'rule': 'rba', 'lr': 0.1}, **NET)
    with pytest.raises(ValueError, match='no key of the adaptive weights'):
        VarNet(_pde(), tfAdapt={'rule': 'sa', 'decay': 0.1}, **NET)
    with pytest.raises(ValueError, match=r'tfAdapt=.* with causal='):
        VarNet(_pde(), tfAdapt='rba', causal=1.0, **NET)
    with pytest.raises(ValueError, match=r"tfAdapt=.* with optimizer='lbfgs'"):
        VarNet(_pde(), tfAdapt='rba', optimizer='lbfgs', **NET)
    with pytest.raises(NotImplementedError, match=r'tfAdapt=.* with towers'):
        VarNet(_pde(), tfAdapt='sa', processors=['GPU:0', 'GPU:1'], **NET)
    diffFun = lambda x, t=0, D=1.0: D * np.ones_like(np.asarray(x, dtype=float))
    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    pde = ADPDE(Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x), MORvar=mor)
    with pytest.raises(NotImplementedError, match=r'tfAdapt=.* with model-order reduction'):
        VarNet(pde, layerWidth=[5], discNum=6, bDiscNum=None, tDiscNum=4, MORdiscScheme=[3], tfAdapt='rba')
    # a learnt vector next to the weights: refused as for every per-test-function weight (the engine refuses it, too)
    obs = (np.array([[0.2, 0.1], [0.4, 0.2], [-0.6, 0.3]]), np.array([0.1, 0.2, 0.3]))
    with pytest.raises(NotImplementedError, match=r'learnSource with tfAdapt='):
        VarNet(_pde(sourceBasis=[lambda x, t: np.sin(pi * x)]), tfAdapt='rba', observations=obs, learnSource=True, **NET)
    vn = VarNet(_pde(), tfAdapt='rba', **NET)
    with pytest.raises(NotImplementedError, match='tfAdapt=... with shuffleData=True'):
        vn.train(str(tmp_path), epochNum=2, batchNum=2, shuffleData=True, verbose=False)
    with pytest.raises(ValueError, match=r'causal=.* with tfAdapt='):
        vn.setCausal(1.0)
    plain = VarNet(_pde(), causal=1.0, **NET)
    with pytest.raises(ValueError, match=r'tfAdapt=.* with causal='):
        plain.setTfAdapt('rba')
    with pytest.raises(ValueError, match='self-adaptive weights are off'):
        plain.tfWeights()
