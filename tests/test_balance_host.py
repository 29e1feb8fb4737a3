"""
CPU tier of the adaptive loss balancing (vn_term_stats, vn_term_grads, `VarNet.train(balance=...)`, `VarNet.termGradients`): the
two rules of varnet_amd/balance.py against the worked numbers of DESIGN.md §33 and against tests/balance_ref.py, the declaration and
binding of the two entry points, and the host layer of `VarNet.train` through a stand-in engine that forms the per-term gradients
by one-hot evaluations of the oracle: where the probes sit, the read-back schedule, the re-draw, the per-feed scaling, the term
count and the refusals.
"""
import os
import re

import numpy as np
import pytest

from tests import balance_ref
from tests.test_obs_host import ObsOracleEngine
from varnet_amd import balance
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pi = np.pi


# ---- the rules ----------------------------------------------------------------------------------------------------
def test_worked_pin_gradnorm():
    n = np.array([4.0, 1.0, 0.5, 0.0])
    act = [True, True, True, False]
    hat = balance.targets('gradnorm', [1, 1, 1, 0], [1, 1, 1, 0], act, n, np.zeros(4), np.zeros(4))
    np.testing.assert_allclose(hat[:3], [1.375, 5.5, 11.0], rtol=1e-15)
    w, skipped = balance.update('gradnorm', [1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0], act, n * n, np.zeros(4), np.zeros(4),
                                [0.2, 0.1, 1.0, 0.0], alpha=0.9, cap=1e30, keepLoss=False)
    assert not skipped
    np.testing.assert_allclose(w[:3], [1.0375, 1.45, 2.0], rtol=1e-15)
    w, skipped = balance.update('gradnorm', [1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0], act, n * n, np.zeros(4), np.zeros(4),
                                [0.2, 0.1, 1.0, 0.0], alpha=0.9, cap=1e30, keepLoss=True)
    c = 1.3 / 2.3525
    np.testing.assert_allclose(w[:3], np.array([1.0375, 1.45, 2.0]) * c, rtol=1e-15)
    np.testing.assert_allclose(w[:3], [0.573326, 0.801275, 1.105207], atol=5e-7)
    assert w[3] == 0.0


def test_maxmean_on_hand_numbers():
    # w_var = 2, mx_var = 0.5; mean_bc = 0.01, mean_ic = 0.25, rho = (3, 1, 1): targets (3 * 2 * 0.5 / 0.01, 2 * 0.5 / 0.25, 2)
    w = [1.0, 1.0, 2.0, 0.0]
    act = [True, True, True, False]
    hat = balance.targets('maxmean', w, [3.0, 1.0, 1.0, 0.0], act, np.ones(4), [9.0, 9.0, 0.5, 0.0], [0.01, 0.25, 0.125, 0.0])
    np.testing.assert_allclose(hat, [300.0, 4.0, 2.0, 0.0], rtol=1e-15)
    new, skipped = balance.update('maxmean', w, w, [3.0, 1.0, 1.0, 0.0], act, np.ones(4), [9.0, 9.0, 0.5, 0.0],
                                  [0.01, 0.25, 0.125, 0.0], [1.0, 1.0, 1.0, 0.0], alpha=0.5, cap=1e4, keepLoss=False)
    assert not skipped
    np.testing.assert_allclose(new, [150.5, 2.5, 2.0, 0.0], rtol=1e-15)


@pytest.mark.parametrize('rule', balance.RULES)
def test_rules_agree_with_the_reference(rule):
    rng = np.random.default_rng(5)
    for trial in range(20):
        act = np.array([True, trial % 3 != 0, True, trial % 2 == 0])
        w = rng.uniform(0.1, 10.0, 4) * act
        w0 = w * rng.uniform(0.5, 2.0, 4)
        rho = rng.uniform(0.1, 10.0, 4)
        rho[2] = 1.0
        norm, mx = rng.uniform(1e-3, 1e3, 4), rng.uniform(1e-3, 1e3, 4)
        mean = mx * rng.uniform(0.01, 1.0, 4)
        L = rng.uniform(1e-4, 1e2, 4)
        cap = [1e4, 1.5][trial % 2]
        keep = trial % 4 < 2
        got, sk = balance.update(rule, w, w0, rho, act, norm * norm, mx, mean, L, alpha=0.7, cap=cap, keepLoss=keep)
        want, sk_ref = balance_ref.rule(rule, list(w), list(w0), list(rho), list(act), list(norm), list(mx), list(mean), list(L),
                                        0.7, cap, keep)
        assert sk == sk_ref is False
        np.testing.assert_allclose(got, want, rtol=1e-12)


def test_clamp_and_keep_loss_continuity():
    act = [True, True, True, False]
    n = np.array([1e6, 1.0, 1e-6, 0.0])
    w0 = np.array([1.0, 2.0, 4.0, 0.0])
    new, _ = balance.update('gradnorm', w0, w0, [0.01, 1, 1, 0], act, n * n, np.zeros(4), np.zeros(4), [1, 1, 1, 0], alpha=0.0,
                            cap=10.0, keepLoss=False)
    np.testing.assert_allclose(new[:3], [0.1, 20.0, 40.0], rtol=1e-15)          # targets 0.01 (below w0 / 10), 1e6 and 1e12 (above 10 w0)
    L = np.array([0.3, 0.02, 5.0, 0.0])
    new, _ = balance.update('gradnorm', w0, w0, [1, 1, 1, 0], act, n * n, np.zeros(4), np.zeros(4), L, alpha=0.5, cap=10.0,
                            keepLoss=True)
    np.testing.assert_allclose(np.sum(new * L), np.sum(w0 * L), rtol=1e-14)     # the weighted loss is continuous at the probe
    raw, _ = balance.update('gradnorm', w0, w0, [1, 1, 1, 0], act, n * n, np.zeros(4), np.zeros(4), L, alpha=0.5, cap=10.0,
                            keepLoss=False)
    np.testing.assert_allclose(new[:3] / raw[:3], np.full(3, new[0] / raw[0]), rtol=1e-14)    # one common factor


@pytest.mark.parametrize('bad', [0.0, float('nan'), float('inf')])
def test_a_zero_or_non_finite_norm_skips_the_probe(bad):
    w = np.array([1.0, 2.0, 3.0, 0.0])
    for rule in balance.RULES:
        new, skipped = balance.update(rule, w, w, [1, 1, 1, 0], [True, True, True, False], [4.0, bad, 1.0, 0.0], np.ones(4), np.ones(4),
                                      np.ones(4))
        assert skipped and np.array_equal(new, w)
    # ... but not when the bad figure belongs to an inactive term
    new, skipped = balance.update('gradnorm', w, w, [1, 1, 1, 0], [True, True, True, False], [4.0, 1.0, 1.0, bad], np.ones(4),
                                  np.ones(4), np.ones(4))
    assert not skipped


def test_option_parsing():
    assert balance.parse_balance(None) is None
    assert balance.parse_balance('gradnorm') == {'rule': 'gradnorm', 'freq': 1000, 'alpha': 0.9, 'cap': 1e4, 'keepLoss': True}
    assert balance.parse_balance({'rule': 'maxmean', 'freq': 5})['freq'] == 5
    for bad, msg in (('fast', 'rule must be'), ({'freq': 3}, 'rule must be'), ({'rule': 'gradnorm', 'freq': 0}, 'freq must be'),
                     ({'rule': 'gradnorm', 'freq': 2.5}, 'freq must be'), ({'rule': 'gradnorm', 'alpha': 1.0}, 'alpha must be'),
                     ({'rule': 'gradnorm', 'alpha': -0.1}, 'alpha must be'), ({'rule': 'gradnorm', 'cap': 0.5}, 'cap must be'),
                     ({'rule': 'gradnorm', 'every': 3}, 'unknown key'), (3, 'balance must be')):
        with pytest.raises(ValueError, match=msg):
            balance.parse_balance(bad)


def test_reference_statistics_by_hand():
    T = np.array([[3.0, -4.0, 0.0], [1.0, 1.0, 2.0]], dtype=np.float32)
    st, gram, absgram = balance_ref.stats(T)
    np.testing.assert_array_equal(st, [[25.0, 7.0, 4.0], [6.0, 4.0, 2.0]])
    np.testing.assert_array_equal(gram, [[25.0, -1.0], [-1.0, 6.0]])
    assert absgram[0, 1] == 7.0
    np.testing.assert_allclose(balance.cosines(gram), [[1.0, -1.0 / np.sqrt(150.0)], [-1.0 / np.sqrt(150.0), 1.0]], rtol=1e-15)


# ---- ABI --------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound():
    from varnet_amd import engine as vengine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    assert re.search(r'int\s+vn_term_stats\s*\(\s*vn_engine\s*\*\s*h,\s*const\s+float\s*\*\s*T_dev,\s*int32_t\s+K,\s*int64_t\s+n,'
                     r'\s*double\s*\*\s*stats,\s*double\s*\*\s*gram\s*\)\s*;', hdr)
    assert re.search(r'int\s+vn_term_grads\s*\(\s*vn_engine\s*\*\s*h,\s*const\s+int32_t\s*\*\s*batches,\s*int32_t\s+n,'
                     r'\s*uint32_t\s+term_mask,', hdr)
    for name, val in (('VN_TERM_BC', 0), ('VN_TERM_IC', 1), ('VN_TERM_VAR', 2), ('VN_TERM_OBS', 3), ('VN_TERM_N', 4)):
        assert re.search(r'#define\s+%s\s+%d\b' % (name, val), hdr)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr) and vengine.VN_ABI_VERSION == 7
    assert vengine.TERMS == balance.TERMS == ('bc', 'ic', 'var', 'obs')
    for name, method in (('vn_term_stats', 'term_stats'), ('vn_term_grads', 'term_grads')):
        assert name in vengine.ABI_SYMBOLS
        assert callable(getattr(vengine.VNEngine, method))
        if os.path.exists(vengine.LIB_PATH):                   # (needs the built library)
            assert hasattr(vengine.load_library(), name)
    mk = open(os.path.join(ROOT, 'varnet_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*=.*\bvn_balance\.hip\b', mk, re.M) and re.search(r'^HDRS\s*=.*\bvn_balance\.h\b', mk, re.M)


# ---- VarNet host layer through a stand-in engine ----------------------------------------------------------------------
class BalanceOracleEngine(ObsOracleEngine):
    """The oracle engine with vn_term_grads: one evaluation per term under its one-hot weights, summed over the batches; it keeps
    what every probe returned and the weights of every gradient evaluation of the training loop."""

    def term_grads(self, batches=(0,), terms=None, grads=False):
        self.__dict__.setdefault('probes', [])
        names = balance.TERMS if terms is None else tuple(terms)
        rows = (True, self.td, True, self.obs is not None)
        w_user, lam_user = self.w.copy(), self.lam
        G, value = np.zeros((4, self.P)), np.zeros(4)
        for k, t in enumerate(balance.TERMS):
            if t not in names or not rows[k]:
                continue
            self.w = np.array([float(j == k) for j in range(3)])
            self.lam = 1.0 if k == 3 else 0.0
            for b in batches:
                res, g = self._eval(b)
                G[k] += g
                value[k] += (res['BCloss'], res['ICloss'], res['varLoss'])[k] if k < 3 else self.misfit
        self.w, self.lam = w_user, lam_user
        out = {'terms': balance.TERMS, 'sumsq': np.sum(G * G, axis=1), 'norm2': np.sqrt(np.sum(G * G, axis=1)),
               'mean_abs': np.mean(np.abs(G), axis=1), 'max_abs': np.max(np.abs(G), axis=1), 'value': value, 'gram': G @ G.T}
        self.probes.append({'batches': tuple(batches), 'terms': names, 'step': self.adam.t, 'out': out})
        return out

    def grad(self, batch=0):
        self.__dict__.setdefault('seen', []).append((self.adam.t, self.w.copy(), self.lam))
        super().grad(batch)


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return BalanceOracleEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                                   isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                                   learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


def _pde(**kw):
    return ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, vel=0.5, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x), **kw)


def _vn(**kw):
    np.random.seed(0)
    return VarNet(_pde(), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6, **kw)


def test_weights_change_at_probe_epochs_and_at_no_other(tmp_path):
    vn = _vn()
    res = vn.train(str(tmp_path), epochNum=8, saveFreq=100, verbose=False, lossLag=0, balance={'rule': 'gradnorm', 'freq': 3})
    hist = res.balanceHist
    assert [h[0] for h in hist] == [1, 4, 7] and not any(h[4] for h in hist)
    assert [p['step'] for p in vn.engine.probes] == [0, 3, 6]                   # BEFORE the epoch
    assert all(list(p['terms']) == ['bc', 'ic', 'var'] and p['batches'] == (0,) for p in vn.engine.probes)
    seen = vn.engine.seen[-8:]                                                  # the eight epochs' evaluations
    assert [t for t, _, _ in seen] == list(range(8))
    for e, (t, w, _) in enumerate(seen):
        np.testing.assert_array_equal(w, hist[e // 3][1][:3])                   # batchNum 1: the engine weights are the train weights
    assert not np.array_equal(hist[0][1], hist[1][1]) and not np.array_equal(hist[1][1], hist[2][1])
    for h in hist:
        assert h[1].shape == (4,) and h[2].shape == (4,) and h[3].shape == (4, 4) and h[1][3] == 0.0
        np.testing.assert_allclose(np.diag(h[3])[:3], 1.0, rtol=1e-12)
    lines = [ln for ln in open(str(tmp_path / 'caseData.txt')) if ': balance (' in ln]
    assert len(lines) == 3 and lines[0].startswith('epoch 1: balance (gradnorm) weights')
    head = [ln for ln in open(str(tmp_path / 'caseData.txt')) if 'rebalanced' in ln]
    assert head == ['\tweights rebalanced from per-term gradient norms: rule gradnorm, every 3 epochs, alpha 0.9, cap 10000.0, '
                    'keepLoss True\n']


@pytest.mark.parametrize('rule', balance.RULES)
def test_loss_lag_is_only_a_readback_schedule_with_balance(tmp_path, rule):
    runs = []
    for lag in (0, 8):
        vn = _vn()
        res = vn.train(str(tmp_path / ('lag%d' % lag)), epochNum=11, saveFreq=5, verbose=False, lossLag=lag, tol=1e-9,
                       balance={'rule': rule, 'freq': 4})
        runs.append((np.array(res.lossAll), [h[0] for h in res.balanceHist], np.array([h[1] for h in res.balanceHist]),
                     vn.engine.theta.copy(), vn.engine.step))
    assert runs[0][1] == [1, 5, 9] and runs[0][4] == 11
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a, b)


def test_a_redraw_restarts_the_moving_average(tmp_path):
    """saveFreq 4, trainUpdelay 7: the set is re-drawn after epoch 7 (adjustWeight: BC / IC x 5, trainWeight on the new set).  The
    probe of epoch 9 averages from the weights of that re-draw, not from the average the probes of epochs 1 and 5 had reached."""
    np.random.seed(77)
    vn = VarNet(ADPDE(Domain1D(), diff=0.1 / pi, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x)),
                layerWidth=[6, 5], discNum=5, bDiscNum=None, tDiscNum=6)
    res = vn.train(str(tmp_path), weight=[10., 10., 1.], smpScheme='optimal', adjustWeight=True, epochNum=12, saveFreq=4,
                   trainUpdelay=7, tolUpd=1e9, verbose=False, lossLag=0,
                   balance={'rule': 'gradnorm', 'freq': 4, 'alpha': 0.5, 'cap': 1e30, 'keepLoss': False})
    hist = res.balanceHist
    assert res.inpIter == [7] and [h[0] for h in hist] == [1, 5, 9] and not any(h[4] for h in hist)
    w8 = vn.engine.seen[-5][1]                                       # epochs 8..12 are the last five evaluations (batchNum 1)
    assert not np.allclose(w8, hist[1][1][:3], rtol=1e-3)            # epoch 8 runs on the re-draw's weights, not on probe 2's
    np.testing.assert_allclose(w8[0] / w8[2], 50.0, rtol=1e-12)      # 5 x 10 : 1
    raw = vn.engine.probes[2]['out']
    n = np.sqrt(raw['sumsq'][:3])
    rho = np.array([50.0, 50.0, 1.0])                                # the user's preference follows adjustWeight
    want = 0.5 * w8 + 0.5 * rho * n.sum() / n
    np.testing.assert_allclose(hist[2][1][:3], want, rtol=1e-12)


def test_batchnum_three_scales_the_repeated_terms(tmp_path):
    vn = _vn()
    res = vn.train(str(tmp_path), weight=[2.0, 3.0, 1.0], epochNum=1, saveFreq=100, verbose=False, batchNum=3,
                   balance={'rule': 'gradnorm', 'freq': 1, 'alpha': 0.5})
    assert vn.tData.batchNum == 3
    probe = vn.engine.probes[0]
    assert probe['batches'] == (0, 1, 2)
    raw = probe['out']
    sc = np.array([1 / 3.0, 1 / 3.0, 1.0, 1 / 3.0])
    epoch, w, norms, cosines, skipped = res.balanceHist[0]
    np.testing.assert_allclose(norms, np.sqrt(raw['sumsq']) * sc, rtol=1e-14)
    w_feed = np.asarray(res.trainWeight)                                         # per feed: BC / IC divided by 3
    w0 = np.array([w_feed[0] * 3, w_feed[1] * 3, w_feed[2], 0.0])
    want, _ = balance_ref.rule('gradnorm', list(w0), list(w0), [2.0, 3.0, 1.0, 0.0], [True, True, True, False],
                               list(np.sqrt(raw['sumsq']) * sc), list(raw['max_abs'] * sc), list(raw['mean_abs'] * sc),
                               list(raw['value'] * sc), 0.5, 1e4, True)
    np.testing.assert_allclose(w, want, rtol=1e-12)
    np.testing.assert_allclose(vn.engine.w, [w[0] / 3, w[1] / 3, w[2]], rtol=1e-15)      # towerWeights on the way to the engine
    np.testing.assert_allclose(np.sum(w * raw['value'] * sc), np.sum(w0 * raw['value'] * sc), rtol=1e-12)


def test_observations_make_four_terms_and_a_steady_problem_two(tmp_path):
    X4 = np.array([[0.2, 0.1], [0.4, 0.2], [0.6, 0.3], [0.8, 0.4]])
    C4 = np.array([0.1, 0.2, 0.3, 0.4])
    heat = ADPDE(Domain1D(np.array([0.0, 1.0])), diff=0.1, vel=0.0, tInterval=[0, 0.5], IC=lambda x: np.zeros([len(x), 1]))
    vn = VarNet(heat, layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, observations=(X4, C4), obsWeight=2.0)
    vn.engine.set_params(vn.engine.get_params() + 0.05)
    res = vn.train(str(tmp_path / 'obs'), weight=[1.0, 1.0, 4.0], epochNum=2, saveFreq=100, verbose=False, batchNum=2,
                   balance={'rule': 'maxmean', 'freq': 1})
    assert list(vn.engine.probes[0]['terms']) == ['bc', 'ic', 'var', 'obs']
    w = res.balanceHist[-1][1]
    assert np.all(w > 0.0) and res.balanceHist[0][3].shape == (4, 4)
    np.testing.assert_allclose(vn.engine.lam, w[3] / 2.0, rtol=1e-14)           # per feed, like the BC / IC weights
    np.testing.assert_allclose(vn.engine.w, [w[0] / 2.0, w[1] / 2.0, w[2]], rtol=1e-14)
    vn.setObsWeight(2.0)                                                         # the factor of the last probe survives train()
    np.testing.assert_allclose(vn.engine.lam, w[3], rtol=1e-14)
    d = vn.termGradients()
    assert d['terms'] == balance.TERMS and np.all(d['norms'] > 0.0) and d['cosines'].shape == (4, 4)
    np.testing.assert_allclose(np.diag(d['cosines']), 1.0, rtol=1e-12)

    steady = ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=1.0, vel=0.0, source=1.0)
    vs = VarNet(steady, layerWidth=[5], discNum=8, bDiscNum=None)
    rs = vs.train(str(tmp_path / 'steady'), epochNum=1, saveFreq=100, verbose=False, balance='gradnorm')
    assert list(vs.engine.probes[0]['terms']) == ['bc', 'var']
    w = rs.balanceHist[0][1]
    assert w[1] == 0.0 and w[3] == 0.0 and w[0] > 0.0 and w[2] > 0.0
    assert rs.balanceHist[0][2][1] == 0.0


def test_refusals(tmp_path):
    vn = _vn()
    for bad, msg in (('fast', 'rule must be'), ({'rule': 'gradnorm', 'freq': 0}, 'freq must be'),
                     ({'rule': 'gradnorm', 'alpha': 1.0}, 'alpha must be'), ({'rule': 'gradnorm', 'cap': 0.9}, 'cap must be'),
                     ({'rule': 'gradnorm', 'period': 2}, 'unknown key')):
        with pytest.raises(ValueError, match=msg):
            vn.train(str(tmp_path / 'a'), epochNum=1, verbose=False, balance=bad)
    with pytest.raises(ValueError, match='at least two active terms'):
        vn.train(str(tmp_path / 'b'), weight=[0.0, 0.0, 1.0], epochNum=1, verbose=False, balance='gradnorm')
    with pytest.raises(NotImplementedError, match=r'updateWeights=True is broken in the reference \(VarNet.py:1373\)'):
        vn.train(str(tmp_path / 'c'), epochNum=1, verbose=False, updateWeights=True)
    vl = VarNet(_pde(), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6, optimizer='lbfgs')
    with pytest.raises(NotImplementedError, match='lbfgs'):
        vl.train(str(tmp_path / 'd'), epochNum=1, verbose=False, balance='gradnorm')
    with pytest.raises(NotImplementedError, match='lbfgs'):
        vl.termGradients()

    def diffFun(x, t=0, D=0.01):
        return D * np.ones([len(x), 1])
    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    pde = ADPDE(Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x), MORvar=mor)
    vm = VarNet(pde, layerWidth=[5], discNum=6, bDiscNum=None, tDiscNum=4, MORdiscScheme=[3])
    with pytest.raises(NotImplementedError, match='model-order reduction'):
        vm.train(str(tmp_path / 'e'), epochNum=1, verbose=False, balance='maxmean')
    vt = _vn()
    vt._towers = object()                                                        # (a controller of forked towers)
    with pytest.raises(NotImplementedError, match='towers'):
        vt.train(str(tmp_path / 'f'), epochNum=1, verbose=False, balance='gradnorm')


def test_without_balance_the_new_entry_points_are_never_called(tmp_path):
    vn = _vn()
    res = vn.train(str(tmp_path), epochNum=3, saveFreq=2, verbose=False)
    assert not hasattr(vn.engine, 'probes') and res.balanceHist == []
    assert not any('balance' in ln for ln in open(str(tmp_path / 'caseData.txt')))
