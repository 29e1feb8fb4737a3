"""
CPU tier of the weights on the Dirichlet and initial rows (vn_set_bic_weights, vn_set_bic_adapt, vn_get_bic_adapt,
vn_set_bic_adapt_state, `VarNet(bicWeights=..., bicAdapt=...)`): the fp64 restatement
(tests/bicadapt_ref.py) against the oracle it extends and against central differences, the cases' weights (a real part of what the
GPU tier compares), the declaration and binding of the four entry points, and the host layer of `VarNet` through an oracle engine
that runs the restatement and the commit protocol on the CPU: registration with the rows, the state carried across a monitor's
borrowing of the engine, history records, the case file, a checkpoint round trip, `setBicAdapt`, and every refusal.
"""
import os
import re

import numpy as np
import pytest

from oracle import tangent_ref as tr
from tests import adapt_ref, bicadapt_ref
from tests.bicadapt_cases import BIG, CASES, IDS, RULES, SMALL, inputs, lambda0, omega_rows, parts_of, reference, reference64, rows, theta, \
    weights_are_real
from tests.gradcheck import assert_grad_close
from tests.oracle_engine import OracleEngine
from tests.parity_cases import GRAD_RTOL
from varnet_amd import engine as vn_engine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import tf_adapt_spec
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pi = np.pi


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _oracle(i):
    name, d_in, dim, widths, q, n_k, nB, bDof, td = CASES[i]
    d = inputs(i)
    nb = nB if td else bDof
    f = np.float64
    return tr.loss_and_grad(theta(i).astype(f), d_in, widths, dim, d['Input'].astype(f), d['gcoef'].astype(f), None, d['N'].astype(f),
                            d['dNt'].astype(f), None, n_k, q, f(d['detJ']), d['biInput'][:nb].astype(f), d['biLabel'][:nb].astype(f), bDof,
                            f(2.0), d['w'], td)


@pytest.mark.parametrize('i', [i for i in SMALL if rows(i)[1] > 0 or not CASES[i][8]], ids=lambda i: IDS[i])
def test_unit_weights_reproduce_the_oracle_exactly(i):
    want, gwant = _oracle(i)
    for om in (None, np.ones(sum(rows(i)))):
        got, g = reference(i, om)
        for k in ('loss', 'BCloss', 'ICloss', 'varLoss'):
            assert got[k] == want[k], k
        assert np.array_equal(g, gwant) and np.array_equal(got['lossVec'], want['lossVec'])


@pytest.mark.parametrize('i', [0, 1, 3, 4], ids=lambda i: IDS[i])
def test_gradient_agrees_with_central_differences(i):
    """The weighted loss differentiated numerically, omega held constant: every parameter block at the suite's gradient bar."""
    name, d_in, dim, widths = CASES[i][:4]
    om = omega_rows(i, {s: lambda0(i, s).astype(np.float64) ** 2 for s in parts_of(i)})
    flat = theta(i).astype(np.float64)
    _, g = reference(i, om, flat)
    h = 1e-6
    num = np.empty_like(g)
    for p in range(flat.size):
        e = np.zeros_like(flat)
        e[p] = h
        num[p] = (reference(i, om, flat + e)[0]['loss'] - reference(i, om, flat - e)[0]['loss']) / (2 * h)
    assert_grad_close(g, num, d_in, widths, GRAD_RTOL, dim=dim, td=CASES[i][8], what='%s vs central differences' % name)


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_the_cases_weights_are_real_and_the_field_is_the_unweighted_one(i):
    weights_are_real(i)
    ref, _ = reference64(i, True)
    ref0, _ = reference64(i, False)
    n = rows(i)
    for s in (0, 1):
        assert ref['field'][s].shape == (n[s],) and np.array_equal(ref['field'][s], ref0['field'][s])
        lam = lambda0(i, s)
        assert lam.dtype == np.float32 and lam.shape == (n[s],)
    # BC and IC are the weighted means of the field
    c = CASES[i]
    om = omega_rows(i, {s: lambda0(i, s).astype(np.float64) ** 2 for s in parts_of(i)})
    assert abs(ref['BCloss'] - 2.0 * np.mean(om[:c[7]] * ref['field'][0])) <= 1e-13 * abs(ref['BCloss'])
    if n[1]:
        assert abs(ref['ICloss'] - 2.0 * np.mean(om[c[7]:] * ref['field'][1])) <= 1e-13 * abs(ref['ICloss'])
    assert i != BIG or n[0] > 256 * 1024


def test_static_weights_normalise_per_part():
    om = np.array([1.0, 3.0, 0.0, 0.0, 2.0, 6.0])
    out = bicadapt_ref.static_weights(om, 2, True)
    assert np.array_equal(out, [0.5, 1.5, 0.0, 0.0, 1.0, 3.0])                                 # means 2 (bc) and 2 (ic, over four rows)
    assert np.array_equal(bicadapt_ref.static_weights(om, 2, False), om)
    assert np.array_equal(bicadapt_ref.static_weights(np.zeros(4), 2, True), np.zeros(4))      # all zero: Z = 1, omega = 0
    assert np.array_equal(bicadapt_ref.static_weights(om[:2], 2, True, time_dependent=False), [0.5, 1.5])


@pytest.mark.parametrize('rule', RULES)
def test_the_parts_move_independently(rule):
    """A part's update reads its own field, state and counter: the other part's field does not enter."""
    spec = adapt_ref.spec_of(rule)
    f0, f1 = reference64(1, False)[0]['field']
    a = bicadapt_ref.part_step(lambda0(1, 1).astype(np.float64), None, 0, f1, spec)
    b = adapt_ref.step(lambda0(1, 1).astype(np.float64), None, 0, f1, spec)
    assert np.array_equal(a['lam'], b['lam']) and a['tau'] == 1 and abs(a['omega'].mean() - 1.0) <= 1e-14
    z = bicadapt_ref.part_step(lambda0(1, 0).astype(np.float64), None, 3, np.zeros_like(f0), spec)
    assert np.array_equal(z['lam'], lambda0(1, 0).astype(np.float64)) and z['tau'] == 3      # a zero field leaves the part alone


# ---- declarations ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    for proto in (r'int vn_set_bic_weights\(vn_engine\* h, const float\* omega_dev, int32_t normalize\);',
                  r'int vn_set_bic_adapt\(vn_engine\* h, int32_t part, int32_t rule, const double par\[10\], const float\* lambda_init_dev\);',
                  r'int vn_get_bic_adapt\(vn_engine\* h, int32_t part, float\* lambda_host, float\* omega_host, float\* slots_host, '
                  r'float\* lossfield_host,\s+double stats\[6\]\);',
                  r'int vn_set_bic_adapt_state\(vn_engine\* h, int32_t part, const float\* lambda_host, const float\* slots_host, '
                  r'int64_t tau\);'):
        assert re.search(proto, hdr), proto
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr)
    declared = set(re.findall(r'^\s*(?:int|const char\*|void)\s+(vn_\w+)\(', hdr, flags=re.M))
    assert declared == set(vn_engine.ABI_SYMBOLS), declared ^ set(vn_engine.ABI_SYMBOLS)
    for meth in ('set_bic_weights', 'set_bic_adapt', 'bic_adapt', 'set_bic_adapt_state'):
        assert callable(getattr(vn_engine.VNEngine, meth))
    # the declarations stay out of vn_internal.h, which every kernel's source hash covers
    csrc = os.path.join(ROOT, 'varnet_amd', 'csrc')
    assert 'bic_rows' not in open(os.path.join(csrc, 'vn_internal.h')).read()
    assert 'vn_bic_rows_launch' in open(os.path.join(csrc, 'vn_bicadapt.h')).read()
    assert '#include "vn_bicadapt.h"' in open(os.path.join(csrc, 'vn_api.hip')).read()
    assert 'vn_bicadapt.hip' in open(os.path.join(csrc, 'Makefile')).read()


# ---- VarNet host layer through an oracle engine ---------------------------------------------------------------------------
class BicOracleEngine(OracleEngine):
    """The oracle engine with the rows' weights: the restatement for loss and gradient, the rules of tests/adapt_ref.py per part,
    and the commit protocol (grad writes the pending state, apply commits it)."""

    def set_bic(self, biInput, biLabel, bDof, biDimVal):
        super().set_bic(biInput, biLabel, bDof, biDimVal)
        self.bw, self.pending, self.field = {}, {}, {}

    def bic_rows(self, part):
        s = {'bc': 0, 'ic': 1}.get(part, part)
        return bicadapt_ref.part_rows(self.bic[0].shape[0], self.bic[2], self.td)[s]

    def bic_parts(self):
        return {p: ('static' if r['spec'] is None else r['spec']) for p, r in getattr(self, 'bw', {}).items()}

    def set_bic_weights(self, omega=None, normalize=False):
        if omega is None:
            self.bw = {}
            return
        om = np.asarray(omega, np.float64).reshape(-1)
        assert om.size == self.bic_rows('bc') + self.bic_rows('ic')
        for p, v in zip(('bc', 'ic'), bicadapt_ref.split(om, self.bic[2], self.td)):
            if v.size:
                self.bw[p] = {'spec': None, 'lambda': v.astype(np.float32), 'normalize': bool(normalize), 'tau': 0, 'slots': None}

    def set_bic_adapt(self, part, spec=None, lambda_init=None):
        spec = tf_adapt_spec(spec)
        if spec is None:
            self.bw.pop(part, None)
            return
        n = self.bic_rows(part)
        assert n > 0
        self.bw[part] = {'spec': spec, 'lambda': np.full(n, spec['init'], np.float32), 'tau': 0,
                         'slots': np.zeros((2, n), np.float32) if spec['rule'] == 'sa' else None}

    def _omega(self, r):
        spec = r['spec'] if r['spec'] is not None else dict(power=1, normalize=r['normalize'])
        return adapt_ref.weights(r['lambda'], spec, dtype=np.float32)

    def bic_adapt(self, part, arrays=True):
        r = self.bw[part]
        om, Z, st = self._omega(r)
        st['tau'] = float(r['tau'])
        return {'lambda': r['lambda'].copy(), 'omega': om, 'slots': None if r['slots'] is None else r['slots'].copy(),
                'lossfield': self.field.get(part, np.zeros(r['lambda'].size, np.float32)), 'stats': st}

    def set_bic_adapt_state(self, part, lam, slots=None, tau=0):
        r = self.bw[part]
        assert r['spec'] is not None
        r['lambda'], r['tau'] = np.asarray(lam, np.float32).copy(), int(tau)
        if r['slots'] is not None:
            r['slots'] = np.zeros_like(r['slots']) if slots is None else np.asarray(slots, np.float32).reshape(2, -1).copy()

    def _eval(self, batch):
        if not getattr(self, 'bw', None):
            return super()._eval(batch)
        Input, gcoef, src, n_k, detJ, Nr, dNtr = self.batches[batch]
        biInput, biLabel, bDof, biDimVal = self.bic
        nb = biInput.shape[0] if self.td else bDof
        N, dNt, W = self.fe
        om = np.concatenate([self._omega(self.bw[p])[0].astype(np.float64) if p in self.bw else np.ones(self.bic_rows(p))
                             for p in ('bc', 'ic')])
        res, g = bicadapt_ref.loss_and_grad(self.theta.astype(np.float64), self.inpDim, self.layerWidth, self.dim, Input, gcoef,
                                            src if self.isSource else None, np.tile(N, n_k) if Nr is None else Nr.reshape(-1),
                                            np.tile(dNt, n_k) if dNtr is None else dNtr.reshape(-1), W if self.integWflag else None,
                                            n_k, self.integNum, detJ, biInput[:nb], biLabel[:nb], bDof, biDimVal, self.w, self.td, om)
        self.field = dict(zip(('bc', 'ic'), [f.astype(np.float32) for f in res['field']]))
        return res, g

    def grad(self, batch=0):
        super().grad(batch)
        self.pending = {}
        for p, r in getattr(self, 'bw', {}).items():
            if r['spec'] is not None and self.adam.t % r['spec']['every'] == 0:
                self.pending[p] = adapt_ref.update(r['lambda'], r['slots'], r['tau'], self.field[p], r['spec'], dtype=np.float32)

    def apply(self):
        super().apply()
        for p, (lam, slots, tau) in getattr(self, 'pending', {}).items():
            self.bw[p].update({'lambda': lam, 'slots': slots, 'tau': tau})
        self.pending = {}


@pytest.fixture
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return BicOracleEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                               isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                               learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


def _pde(**kw):
    return ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, vel=0.5, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x), **kw)


NET = dict(layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)


def test_options_are_parsed_by_part():
    chk = lambda w, a, td=True: VarNet._check_bic_weights(w, a, False, False, False, False, td)
    assert chk(None, None) == (None, None)
    assert chk(None, 'rba')[1] == {'ic': adapt_ref.RBA} and chk(None, 'sa', td=False)[1] == {'bc': adapt_ref.SA}
    w, a = chk({'bc': [1.0, 2.0]}, {'ic': {'rule': 'sa', 'lr': 0.01}})
    assert np.array_equal(w['bc'], [1.0, 2.0]) and w['normalize'] is False and a == {'ic': adapt_ref.spec_of('sa', lr=0.01)}
    assert np.array_equal(chk(np.ones(7), None)[0]['rows'], np.ones(7))
    for bad_w, bad_a, msg in (({'xx': 1}, None, "takes the keys 'bc', 'ic' and 'normalize'"), (None, {'foo': 'rba'}, "takes the keys 'bc' and 'ic'"),
                              ({'bc': [-1.0]}, None, 'finite and >= 0'), ({'ic': [1.0]}, {'ic': 'rba'}, 'replace each other'),
                              (None, {'ic': {'rule': 'rba', 'lr': 1}}, "a key of the 'sa' rule")):
        with pytest.raises(ValueError, match=msg):
            chk(bad_w, bad_a)
    with pytest.raises(ValueError, match="no 'ic' part"):
        chk(None, {'ic': 'rba'}, td=False)
    with pytest.raises(NotImplementedError, match='with a hard-constraint ansatz'):
        VarNet._check_bic_weights(None, 'rba', False, False, False, True, True)


def test_registration_follows_the_rows_and_the_state_is_carried(cpu_engine):
    vn = VarNet(_pde(), bicWeights={'bc': lambda x, t: 1.0 + t[:, 0]}, bicAdapt={'ic': {'rule': 'sa', 'lr': 0.01}}, **NET)
    eng = vn.engine
    td = vn._build_tdata()
    td.select_mor(0)
    assert eng.bic_parts() == {'bc': 'static', 'ic': adapt_ref.spec_of('sa', lr=0.01)}
    w = vn.bicRowWeights(td)
    nbc, nic = eng.bic_rows('bc'), eng.bic_rows('ic')
    assert w['bc']['x'].shape == (nbc, 2) and w['ic']['x'].shape == (nic, 2)
    assert np.allclose(w['bc']['omega'], 1.0 + w['bc']['x'][:, 1]) and np.all(w['ic']['omega'] == 1.0)
    # the training set's state survives another set's use of the engine (a monitor on the uniform set) and comes back with it
    eng.set_bic_adapt_state('ic', np.full(nic, 2.5, np.float32), np.full((2, nic), 0.25, np.float32), 7)
    other = vn._build_tdata()
    other.select_mor(0)
    s = eng.bic_adapt('ic')
    assert s['stats']['tau'] == 0.0 and np.all(s['lambda'] == 1.0)
    td.select_mor(0)
    s = eng.bic_adapt('ic')
    assert np.all(s['lambda'] == 2.5) and np.all(s['slots'] == 0.25) and s['stats']['tau'] == 7.0
    # setBicAdapt: another rule from its initial state on the last training set, then off
    vn.tData = td
    vn.setBicAdapt({'bc': 'rba', 'ic': 'rba'})
    assert eng.bic_parts() == {'bc': adapt_ref.RBA, 'ic': adapt_ref.RBA} and eng.bic_adapt('ic')['stats']['tau'] == 0.0
    vn.setBicAdapt(None)
    assert eng.bic_parts() == {} and vn.bicAdapt is None and vn.bicWeights is None
    with pytest.raises(ValueError, match='the rows carry no weights'):
        vn.bicRowWeights()


def test_train_history_case_file_and_checkpoint_round_trip(cpu_engine, tmp_path):
    vn = VarNet(_pde(), bicAdapt={'ic': {'rule': 'rba', 'eta': 0.5, 'gamma': 0.9}}, **NET)
    res = vn.train(str(tmp_path), epochNum=4, tol=0.0, saveFreq=2, verbose=False, lossLag=0)
    case = open(os.path.join(str(tmp_path), 'caseData.txt')).read()
    assert 'Weights on the boundary and initial rows: ic: rule rba, eta = 0.5, every = 1, gamma = 0.9' in case
    assert [e for e, _ in res.bicAdaptHist] == [2, 4]
    st = res.bicAdaptHist[-1][1]
    assert set(st) == {'ic'} and set(st['ic']) == {'min', 'max', 'mean', 'share', 'Z', 'tau'} and st['ic']['tau'] == 4.0
    assert st['ic']['max'] > st['ic']['min'] and 0.0 < st['ic']['share'] < 1.0               # the weights moved apart
    w = vn.bicRowWeights()
    assert set(w) == {'ic'} and w['ic']['l'].shape == w['ic']['omega'].shape and np.any(w['ic']['l'] > 0)
    arrays = vn.checkpoint_arrays()
    assert str(arrays['bicadapt_ic_rule']) == 'rba' and int(arrays['bicadapt_ic_tau']) == 4 and 'bicadapt_ic_slots' not in arrays
    lam = arrays['bicadapt_ic_lambda'].copy()
    vn.engine.set_bic_adapt_state('ic', np.ones_like(lam), None, 0)
    vn.restore_arrays(arrays)
    s = vn.engine.bic_adapt('ic')
    assert np.array_equal(s['lambda'], lam) and s['stats']['tau'] == 4.0
    plain = VarNet(_pde(), **NET)
    assert not any(k.startswith('bicadapt') for k in plain.checkpoint_arrays())
    assert plain.train(str(tmp_path / 'plain'), epochNum=2, tol=0.0, saveFreq=1, verbose=False).bicAdaptHist == []


def test_refusals(cpu_engine, tmp_path):
    with pytest.raises(ValueError, match=r"bicAdapt=.* with optimizer='lbfgs'"):
        VarNet(_pde(), bicAdapt='rba', optimizer='lbfgs', **NET)
    VarNet(_pde(), bicWeights={'ic': lambda x, t: 2.0}, optimizer='lbfgs', **NET)          # static weights work with L-BFGS
    with pytest.raises(NotImplementedError, match=r'bicWeights= / bicAdapt= with towers'):
        VarNet(_pde(), bicAdapt='sa', processors=['GPU:0', 'GPU:1'], **NET)
    diffFun = lambda x, t=0, D=1.0: D * np.ones_like(np.asarray(x, dtype=float))
    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    pde = ADPDE(Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x), MORvar=mor)
    with pytest.raises(NotImplementedError, match=r'bicWeights= / bicAdapt= with model-order reduction'):
        VarNet(pde, layerWidth=[5], discNum=6, bDiscNum=None, tDiscNum=4, MORdiscScheme=[3], bicAdapt='rba')
    obs = (np.array([[0.2, 0.1], [0.4, 0.2], [-0.6, 0.3]]), np.array([0.1, 0.2, 0.3]))
    with pytest.raises(NotImplementedError, match=r'learnSource with bicWeights= / bicAdapt='):
        VarNet(_pde(sourceBasis=[lambda x, t: np.sin(pi * x)]), bicAdapt='rba', observations=obs, learnSource=True, **NET)
    vn = VarNet(_pde(), bicAdapt='rba', **NET)
    with pytest.raises(NotImplementedError, match='bicWeights= / bicAdapt= with shuffleData=True'):
        vn.train(str(tmp_path), epochNum=2, batchNum=2, shuffleData=True, verbose=False)
    with pytest.raises(ValueError, match='replace each other'):
        vn.setBicAdapt({'ic': 'rba'}, bicWeights={'ic': [1.0]})
