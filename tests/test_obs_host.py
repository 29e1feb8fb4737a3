"""
CPU tier of the observation term (vn_set_observations, `VarNet(..., observations=..., obsWeight=...)`): the validation of every
malformed input, the scaling of obsWeight by train(), its division per feed, the C ABI's declarations, the restatement
(tests/obs_ref.py) against central differences of its own loss, and the input conditions of the GPU parity cases
(tests/test_obs_gpu.py), asserted from the reference alone.
"""
import os
import re

import numpy as np
import pytest

from oracle import tf1_graph as og
from tests import obs_cases, obs_ref
from tests.gradcheck import block_errors
from tests.oracle_engine import OracleEngine
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

pi = np.pi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ObsOracleEngine(OracleEngine):
    """The oracle engine with vn_set_observations / vn_set_obs_weight / vn_get_obs_misfit: lambda times the misfit of
    tests/obs_ref.py added to the loss and the gradient, BC / IC / var untouched."""
    obs = None
    lam = None
    misfit = None

    def set_observations(self, X=None, value=None, q=None, dir=None, rowptr=None, wgt=None, weight=1.0):
        self.obs = None if X is None or len(X) == 0 else dict(X=X, value=value, q=q, dir=dir, rowptr=rowptr, wgt=wgt)
        self.lam = float(weight)

    def set_obs_weight(self, weight):
        self.lam = float(weight)

    def obs_misfit(self):
        return self.misfit

    def _eval(self, batch):
        res, g = super()._eval(batch)
        if self.obs is None:
            return res, g
        o = self.obs
        O, gO, _ = obs_ref.obs_term(self.theta.astype(np.float64), self.inpDim, self.layerWidth, self.dim, o['X'], o['value'],
                                    o['q'], o['dir'], o['rowptr'], o['wgt'])
        self.misfit = O
        res = dict(res)
        res['loss'] = res['loss'] + self.lam * O
        return res, g + self.lam * gO


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return ObsOracleEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                               isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                               learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


def heat(t=True):
    return ADPDE(Domain1D(np.array([0.0, 1.0])), diff=0.1, vel=0.0, tInterval=[0, 0.5] if t else None,
                 IC=(lambda x: np.zeros([len(x), 1])) if t else None)


def make(obs, t=True, **kw):
    return VarNet(heat(t), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4 if t else [], observations=obs, **kw)


X4 = np.array([[0.2, 0.1], [0.4, 0.2], [0.6, 0.3], [0.8, 0.4]])
C4 = np.array([0.1, 0.2, 0.3, 0.4])
FUN = dict(X=X4, value=[0.5, -0.5], rowptr=np.array([0, 1, 4]), q=[1.0, 0.3, 0.4, 0.3], dir=[[0.1], [0.0], [0.2], [0.0]],
           sigma=[0.5, 2.0])


# ---- validation --------------------------------------------------------------------------------------------------------------
def test_point_sensors_and_functionals_are_assembled_in_fp64():
    vn = make((X4, C4, 0.5))
    r = vn.obsRows
    assert r['rowptr'] is None and r['q'] is None and r['dir'] is None
    assert r['X'].dtype == np.float64 and np.array_equal(r['X'], X4) and np.array_equal(r['value'], C4)
    np.testing.assert_array_equal(r['wgt'], np.full(4, 1.0 / 0.25))
    assert vn.obsWeight == 1.0 and vn.engine.lam == 1.0
    assert make((X4, C4)).obsRows['wgt'] is None
    vn = make(FUN, obsWeight=3.0)
    r = vn.obsRows
    assert r['rowptr'].dtype == np.int32 and r['rowptr'].tolist() == [0, 1, 4]
    np.testing.assert_array_equal(r['wgt'], 1.0 / np.array([0.5, 2.0]) ** 2)
    assert r['dir'].shape == (4, 1) and r['q'].shape == (4,)
    assert vn.engine.lam == 3.0 and vn.engine.obs['rowptr'] is r['rowptr']
    # a steady problem: rows are [x]
    vn = make((X4[:, :1], C4), t=False)
    assert vn.obsRows['X'].shape == (4, 1)


@pytest.mark.parametrize('obs,field', [
    ((X4[:, :1], C4), 'X has shape'),                                   # missing the time column
    ((X4.reshape(2, 2, 2), C4), 'X has shape'),
    ((np.zeros((0, 2)), []), 'X has shape'),
    ((np.where(X4 > 0.7, np.nan, X4), C4), 'X has non-finite'),
    ((X4, C4[:3]), 'value has 3 entries'),
    ((X4, [0.1, np.inf, 0.3, 0.4]), 'value has non-finite'),
    ((X4, 'abcd'), 'value must be a numeric array'),
    ((X4, C4, [1.0, 1.0]), 'sigma has 2 entries'),
    ((X4, C4, 0.0), 'sigma must be positive'),
    ((X4, C4, [1.0, -1.0, 1.0, 1.0]), 'sigma must be positive'),
    ((X4, C4, np.nan), 'sigma has non-finite'),
    ((X4, C4, 1e-200), 'sigma is too small'),
    ((X4,), 'must be (X, c)'),
    ('x', 'must be (X, c)'),
    (dict(FUN, rowptr=[0, 1, 3]), 'rowptr must increase strictly from 0 to 4'),
    (dict(FUN, rowptr=[1, 2, 4]), 'rowptr must increase strictly from 0 to 4'),
    (dict(FUN, rowptr=[0, 4, 4]), 'rowptr must increase strictly'),      # an empty segment
    (dict(FUN, rowptr=[0, 3, 1]), 'rowptr must increase strictly'),
    (dict(FUN, rowptr=[0, 4]), 'rowptr must hold 3 integers'),
    (dict(FUN, rowptr=[0.0, 1.0, 4.0]), 'rowptr must hold 3 integers'),
    (dict(FUN, rowptr=None), 'field rowptr is required'),
    (dict(FUN, q=[1.0, 2.0]), 'q has 2 entries'),
    (dict(FUN, q=[1.0, np.nan, 1.0, 1.0]), 'q has non-finite'),
    (dict(FUN, dir=[[0.1, 0.2]] * 4), 'dir has 8 entries'),
    (dict(FUN, dir=[[np.inf]] * 4), 'dir has non-finite'),
    (dict(FUN, sigma=[1.0, 0.0]), 'sigma must be positive'),
    (dict(FUN, weights=[1.0, 1.0]), 'unknown field'),
], ids=lambda v: v.replace(' ', '_') if isinstance(v, str) else 'obs')
def test_malformed_observations_name_the_field(obs, field):
    with pytest.raises(ValueError, match='observations.*' + re.escape(field)):
        make(obs)


def test_obs_weight_refusals():
    with pytest.raises(ValueError, match='obsWeight=2.0 is an option of observations'):
        make(None, obsWeight=2.0)
    for bad in (-1.0, float('nan'), float('inf'), 'x', [1.0], True):
        with pytest.raises(ValueError, match='obsWeight=.* must be a finite number >= 0'):
            make((X4, C4), obsWeight=bad)
    vn = make((X4, C4))
    with pytest.raises(ValueError, match='obsWeight=.* must be a finite number >= 0'):
        vn.setObsWeight(-2.0)
    with pytest.raises(ValueError, match='no observations'):
        make(None).setObsWeight(1.0)
    with pytest.raises(ValueError, match='no observations'):
        make(None).obsMisfit()


def test_mor_with_observations_raises():
    def diffFun(x, t=0, D=0.01):
        return D * np.ones([len(x), 1])

    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    pde = ADPDE(Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x), MORvar=mor)
    with pytest.raises(NotImplementedError, match='observations with model-order reduction'):
        VarNet(pde, layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, MORdiscScheme=[3], observations=(X4, C4))


# ---- the weight --------------------------------------------------------------------------------------------------------------
def test_train_scales_obs_weight_like_the_variational_weight(tmp_path):
    vn = make((X4, C4, 0.5), obsWeight=2.0)
    res = vn.train(str(tmp_path / 'a'), weight=[10.0, 1.0, 4.0], epochNum=1, saveFreq=1, verbose=False)
    tW = np.asarray(res.trainWeight)                                     # per feed: one feed, so trainWeight's own values
    factor = tW[2] / 4.0
    assert factor != 1.0
    np.testing.assert_allclose(vn.engine.lam, 2.0 * factor, rtol=1e-15)
    np.testing.assert_allclose(tW[0] / 10.0, factor, rtol=1e-12)         # the same factor as on the other weights
    # between train() calls
    vn.setObsWeight(5.0)
    np.testing.assert_allclose(vn.engine.lam, 5.0 * factor, rtol=1e-15)
    # useOriginalW: unscaled
    vn.train(str(tmp_path / 'b'), weight=[10.0, 1.0, 4.0], epochNum=1, saveFreq=1, verbose=False, useOriginalW=True)
    assert vn.engine.lam == 5.0
    # a zero variational weight is refused
    with pytest.raises(ValueError, match='observations with a zero variational weight'):
        vn.train(str(tmp_path / 'c'), weight=[10.0, 1.0, 0.0], epochNum=1, saveFreq=1, verbose=False)
    # one caseData.txt line
    lines = [ln for ln in open(str(tmp_path / 'b' / 'caseData.txt')) if 'Observations' in ln]
    assert lines == ['\tObservations: 4 (4 points), weight 5.0\n']
    assert not any('Observations' in ln for ln in open(str(tmp_path / 'c' / 'caseData.txt'))) \
        if os.path.exists(str(tmp_path / 'c' / 'caseData.txt')) else True


def test_obs_weight_is_divided_per_feed(tmp_path):
    """The observed points are replicated in every feed like the Dirichlet rows: lambda takes the division of w[0:2], and the
    gradients of the feeds sum to the single-feed one."""
    vn = make((X4, C4), obsWeight=3.0)
    res = vn.train(str(tmp_path / 'a'), weight=[1.0, 1.0, 1.0], epochNum=1, saveFreq=1, verbose=False, useOriginalW=True, batchNum=2)
    assert vn.tData.batchNum == 2
    assert vn.engine.lam == 1.5
    np.testing.assert_allclose(np.asarray(res.trainWeight), [0.5, 0.5, 1.0])
    eng = vn.engine
    gb = eng.bind_grad_buffer()
    g = np.zeros(eng.P)
    for bi in range(2):
        eng.grad(vn.tData.engine_batch(0, bi))
        g += gb[:eng.P].numpy()
    one = make((X4, C4), obsWeight=3.0)
    one.engine.theta = eng.theta.copy()                                  # (get_params rounds to fp32)
    one.train(str(tmp_path / 'b'), weight=[1.0, 1.0, 1.0], epochNum=0, saveFreq=1, verbose=False, useOriginalW=True)
    assert one.engine.lam == 3.0
    one.engine.grad(one.tData.engine_batch(0, 0))
    np.testing.assert_allclose(g, one.engine.bind_grad_buffer()[:eng.P].numpy(), rtol=1e-9, atol=1e-13)


def test_misfit_and_components():
    vn = make(FUN, obsWeight=2.0)
    eng = vn.engine
    eng.set_params(eng.get_params() + 0.1)
    td = vn._build_tdata()
    O = vn.obsMisfit()
    r = vn.obsRows
    want, _, res = obs_ref.obs_term(eng.theta, 2, [5], 1, r['X'], r['value'], r['q'], r['dir'], r['rowptr'], r['wgt'])
    assert O == want and O > 0
    # by hand on the first observation: a point sensor with a derivative part 0.1 du/dx
    fwd = lambda z: float(eng.forward(z)[0])
    h = 1e-6
    xp, xm = X4[:1].copy(), X4[:1].copy()
    xp[0, 0] += h
    xm[0, 0] -= h
    assert abs(res[0] - (fwd(X4[:1]) + 0.1 * (fwd(xp) - fwd(xm)) / (2 * h) - 0.5)) < 1e-8
    # the components are those of the same engine without its observations; the loss gains lambda O
    comp, _, _ = vn.splitLoss(td)
    out = eng.eval_loss(0)[0]
    kept, eng.obs = eng.obs, None
    comp0, _, _ = vn.splitLoss(td)
    out0 = eng.eval_loss(0)[0]
    eng.obs = kept
    np.testing.assert_array_equal(comp, comp0)
    assert out[1:] == out0[1:]
    np.testing.assert_allclose(out[0], out0[0] + 2.0 * O, rtol=1e-14)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entry_points():
    import ctypes as C
    from varnet_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'int\s+vn_set_observations\s*\(\s*vn_engine\s*\*\s*h\s*,\s*const\s+float\s*\*\s*X_dev\s*,\s*const\s+float\s*\*\s*q_dev\s*,'
                     r'\s*const\s+float\s*\*\s*dir_dev\s*,\s*const\s+int32_t\s*\*\s*rowptr_dev\s*,\s*const\s+float\s*\*\s*value_dev\s*,'
                     r'\s*const\s+float\s*\*\s*wgt_dev\s*,\s*int64_t\s+n\s*,\s*int64_t\s+nO\s*,\s*double\s+lambda\s*\)\s*;', code)
    assert re.search(r'int\s+vn_set_obs_weight\s*\(\s*vn_engine\s*\*\s*h\s*,\s*double\s+lambda\s*\)\s*;', code)
    assert re.search(r'int\s+vn_get_obs_misfit\s*\(\s*vn_engine\s*\*\s*h\s*,\s*double\s*\*\s*misfit\s*\)\s*;', code)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr)            # additive: the version stays
    for name in ('vn_set_observations', 'vn_set_obs_weight', 'vn_get_obs_misfit'):
        assert name in engine.ABI_SYMBOLS
    res, args = engine._SIGS['vn_set_observations']
    assert res is C.c_int and args == [C.c_void_p] * 7 + [C.c_int64, C.c_int64, C.c_double]
    for name in ('set_observations', 'set_obs_weight', 'obs_misfit'):
        assert callable(getattr(engine.VNEngine, name))


# ---- the restatement checks itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['points', 'functionals', 'functionals_dir'])
def test_reference_gradient_against_central_differences(form):
    d_in, dim, widths = 3, 2, [5]
    rng = np.random.default_rng(4)
    flat = og.glorot_init(d_in, widths, 1).astype(np.float64) + 0.3 * rng.standard_normal(og.param_count(d_in, widths))
    lens = np.ones(6, dtype=int) if form == 'points' else np.array([1, 3, 7, 2, 1, 4])
    n, nO = int(lens.sum()), len(lens)
    X = rng.uniform(-1, 1, (n, d_in))
    kw = dict(value=rng.standard_normal(nO))
    if form != 'points':
        kw.update(q=rng.uniform(0.5, 1.5, n), rowptr=np.concatenate([[0], np.cumsum(lens)]), wgt=rng.uniform(0.25, 4.0, nO))
    if form == 'functionals_dir':
        kw['dirs'] = 0.5 * rng.standard_normal((n, dim))
    f = lambda th: obs_ref.obs_term(th, d_in, widths, dim, X, activation='tanh', **kw)
    O, g, r = f(flat)
    assert O > 0 and r.shape == (nO,)
    np.testing.assert_allclose(O, np.mean(kw.get('wgt', 1.0) * r ** 2), rtol=1e-14)
    h = 1e-6
    fd = np.zeros_like(flat)
    for p in range(flat.size):
        e = np.zeros_like(flat)
        e[p] = h
        fd[p] = (f(flat + e)[0] - f(flat - e)[0]) / (2 * h)
    err = np.max(np.abs(fd - g)) / np.max(np.abs(g))
    print('obs_ref %s: gradient vs central differences, relative error %.3e' % (form, err))
    assert err <= 1e-6


# ---- input conditions of the GPU parity cases --------------------------------------------------------------------------------
@pytest.mark.parametrize('with_dir', [False, True], ids=['values', 'dir'])
@pytest.mark.parametrize('ci', range(len(obs_cases.CASES)), ids=obs_cases.IDS)
def test_parity_cases_feel_the_term(ci, with_dir):
    """Leaving the term out moves the loss by >= 100 LOSS_RTOL and every gradient block by >= 100 GRAD_RTOL: a kernel that
    dropped the term, or a block of its gradient, cannot pass the parity bars.  From the reference alone."""
    case = obs_cases.CASES[ci]
    flat, obs, lam, ref, gref, ref0, gref0 = obs_cases.ref_of(ci, with_dir)
    assert lam == float(np.float32(lam)) and lam > 0
    share = lam * ref['obs'] / ref['loss']
    moved = block_errors(gref0, gref, case[0], case[2], case[1], case[8])
    least = min(moved, key=moved.get)
    print('obs %s %s: lambda %.6g, O %.6e, share of the loss %.3f, least-moved block %s %.3e'
          % (obs_cases.IDS[ci], 'dir' if with_dir else 'values', lam, ref['obs'], share, least, moved[least]))
    assert abs(share - 0.5) < 1e-6
    assert abs(ref['loss'] - ref0['loss']) >= 100 * LOSS_RTOL * abs(ref['loss'])
    assert moved[least] >= 100 * GRAD_RTOL, (least, moved[least])
    for key in ('BCloss', 'ICloss', 'varLoss'):
        assert ref[key] == ref0[key]
    if with_dir:                                                        # the derivative part is a real part of the functionals
        O_values = obs_cases.reference(ci, flat, obs_cases.case_data(ci), dict(obs, dir=None), lam)[0]['obs']
        assert abs(O_values - ref['obs']) > 1e-3 * ref['obs']
