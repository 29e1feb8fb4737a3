"""
CPU tier of source identification (vn_set_source_basis, vn_set_source_learn, `ADPDE(sourceBasis=..., sourceAmp=...)`,
`VarNet(..., learnSource=..., sourceLr=..., sourceBounds=...)`): the reference tests/source_ref.py against tests/nldiff_ref.py and
against central differences, the input condition of the GPU cases from the CPU numbers alone, the host fold of the amplitudes
without learnSource, the validation of every option, the refusals, the C header, and the checkpoint round trip on a stub engine.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import nldiff_ref
from tests import source_cases as sc
from tests.oracle_engine import OracleEngine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

pi = np.pi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _presummed_loss(i, J, amp=None):
    """nldiff_ref's loss of case i with the source s0 + Phi^T a summed beforehand."""
    nldiff, nlflux, reaction = sc.terms_of(i)
    f64 = lambda t: (None if t[0] is None else t[0].astype(np.float64), t[1])
    kw = sc.ref_kw(i)
    kw['source'], kw['is_source'] = sc.mixed(i, J, amp), True
    return nldiff_ref.loss_and_grad(sc.theta(i).astype(np.float64), sc.case(i)[0], sc.case(i)[2], f64(nldiff), f64(nlflux), f64(reaction),
                                    torch.float64, **kw)


@pytest.mark.parametrize('i', range(sc.N_CASES), ids=sc.IDS)
def test_reference_restates_nldiff_ref(i):
    """Loss pieces, lossVec and theta-gradient equal tests/nldiff_ref.loss_and_grad with the pre-summed source to 1e-13; the
    amplitude gradient agrees with central differences of that loss to 1e-6 of S_j (the loss is quadratic in the amplitudes: the
    difference quotient carries rounding only)."""
    J = 3
    res, g, ga, S = sc.reference64(i, J)
    want, gw = _presummed_loss(i, J)
    for k in ('loss', 'BCloss', 'ICloss', 'varLoss'):
        assert abs(res[k] - want[k]) <= 1e-13 * abs(want[k]), (k, res[k], want[k])
    assert np.max(np.abs(res['lossVec'] - want['lossVec'])) <= 1e-13 * np.max(np.abs(want['lossVec']))
    assert np.max(np.abs(g - gw)) <= 1e-13 * np.max(np.abs(gw))
    a0 = sc.basis(i, J)[1]
    for j in range(J):
        h = 1e-3
        ap, am = a0.copy(), a0.copy()
        ap[j] += h
        am[j] -= h
        fd = (_presummed_loss(i, J, ap)[0]['loss'] - _presummed_loss(i, J, am)[0]['loss']) / (2 * h)
        print('%s a%d: g %.6e fd %.6e S %.3e dev/S %.2e' % (sc.IDS[i], j, ga[j], fd, S[j], abs(ga[j] - fd) / S[j]))
        assert abs(ga[j] - fd) <= 1e-6 * S[j], (sc.IDS[i], j, ga[j], fd, S[j])


def test_gpu_cases_condition():
    """From the CPU numbers alone: every component is non-zero, the conditioning floor 0.01 S_j is the binding branch of the bar
    for at most 5 % of all components over all (case, J), and the reference evaluated in fp32 stays within the bar -- a change of
    the cases or of the basis cannot quietly widen it."""
    binding, total = [], 0
    for i, J in sc.PAIRS:
        _, _, g64, S = sc.reference64(i, J)
        assert np.all(g64 != 0.0) and np.all(S > 0.0), (sc.IDS[i], J)
        total += J
        for j in range(J):
            if abs(g64[j]) < sc.COND_FLOOR * S[j]:
                binding.append((sc.IDS[i], J, j, abs(g64[j]) / S[j]))
        g32 = sc.evaluate(i, J, dtype=torch.float32)[2]
        rel = np.abs(g32 - g64) / sc.bars(g64, S)
        print('%s J=%d: fp32 restatement worst err/bar %.3f' % (sc.IDS[i], J, rel.max()))
        assert np.all(rel <= 1.0), (sc.IDS[i], J, rel)
    print('floor binding: %d of %d' % (len(binding), total), binding)
    assert len(binding) <= sc.BINDING_FRAC * total, binding


def test_cases_reach_both_row_paths():
    """nT % 4 == 2 on case 6 (one row per thread), a multiple of 4 elsewhere and on the cut case (four rows per thread)."""
    assert sc.inputs(6)['Input'].shape[0] % 4 == 2
    assert sc.inputs(sc.N_CASES - 1)['Input'].shape[0] % 4 == 0 and sc.inputs(0)['Input'].shape[0] % 4 == 0
    assert sorted({sc.case(i)[3] for i in range(sc.N_CASES)}) == [6, 8, 16, 36, 64, 100, 216, 256]
    assert {sc.case(i)[8] for i in range(sc.N_CASES)} == {True, False}
    for J in (1, 3, 5, 64):
        Phi = sc.basis(0, J)[0]
        assert Phi.shape[0] == J and (Phi.min(axis=1) < 0).any()            # at least one sign-changing stream


# ---- the Python surface on a stub engine -----------------------------------------------------------------------------------------
class SourceStubEngine(OracleEngine):
    """The oracle engine plus the registrations the constructor makes: observations and the amplitudes are only stored."""
    src_reg = None
    amps = None

    def set_observations(self, *a, **kw):
        pass

    def set_coef_learn(self, *a, **kw):
        pass

    def set_source_learn(self, mask=None, init=None, lo=None, hi=None, lr=None):
        self.src_reg = None if mask is None else dict(mask=list(mask), lo=np.array(lo), hi=np.array(hi), lr=lr)
        self.amps = None if mask is None else np.asarray(init, dtype=np.float32).astype(np.float64)

    def get_source_amps(self, grad=False, J=None):
        assert J is None or J == self.amps.size
        return (self.amps.copy(), np.arange(float(self.amps.size))) if grad else self.amps.copy()

    def set_source_amps(self, amp):
        self.amps = np.asarray(amp, dtype=np.float32).astype(np.float64)


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return SourceStubEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                                isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                                learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


X4 = np.array([[0.2, 0.1], [0.4, 0.2], [0.6, 0.3], [0.8, 0.4]])
C4 = np.array([0.1, 0.2, 0.3, 0.4])
BASIS = [lambda x, t, j=j: np.sin(j * pi * x) * (1.0 + t) for j in (1, 2, 3)]


def pde(**kw):
    return ADPDE(Domain1D(np.array([0.0, 1.0])), diff=0.1, vel=0.0, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x), **kw)


FULL = dict(sourceBasis=BASIS, sourceAmp=[0.5, -1.0, 2.0])


def make(p=None, obs=(X4, C4), **kw):
    return VarNet(pde(**FULL) if p is None else p, layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, observations=obs, **kw)


def test_amplitudes_fold_into_the_source_without_learning():
    """Without learnSource the engine sees a plain source: s0 + Phi^T a at the rows, also when `source` itself is 0."""
    X = np.column_stack([np.linspace(0.05, 0.95, 7), np.linspace(0.0, 0.5, 7)])
    want = sum(a * f(X[:, :1], X[:, 1:2]) for a, f in zip(FULL['sourceAmp'], BASIS))
    vn = make()
    assert vn.lossOpt['isSource'] is True and vn.srcLearn is None and vn.engine.src_reg is None
    np.testing.assert_allclose(vn.PDEinpData(X)[2], want, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(vn.PDEinpData(X, basis=False)[2], np.zeros((7, 1)))
    np.testing.assert_array_equal(vn.sourceAmplitudes(), [0.5, -1.0, 2.0])
    s0 = lambda x, t: 3.0 * x + t
    vn = make(pde(source=s0, **FULL))
    np.testing.assert_allclose(vn.PDEinpData(X)[2], s0(X[:, :1], X[:, 1:2]) + want, rtol=0, atol=1e-15)
    # sourceAmp defaults to zeros; without a basis nothing changes
    vn = make(pde(sourceBasis=BASIS))
    np.testing.assert_array_equal(vn.sourceAmplitudes(), np.zeros(3))
    np.testing.assert_array_equal(vn.PDEinpData(X)[2], np.zeros((7, 1)))
    vn = make(pde())
    assert vn.lossOpt['isSource'] is False
    with pytest.raises(ValueError, match='the PDE has no source basis'):
        vn.sourceAmplitudes()
    for f in (vn.sourceGrad, lambda: vn.setSourceAmplitudes([1.0])):
        with pytest.raises(ValueError, match='learns no source amplitudes'):
            f()


def test_registration_and_accessors():
    vn = make(learnSource=[True, False, True], sourceLr=0.05, sourceBounds=[(0.0, None), None, (None, 4.0)])
    reg = vn.engine.src_reg
    assert reg['mask'] == [1, 0, 1] and reg['lr'] == 0.05
    assert reg['lo'][0] == 0.0 and reg['hi'][0] == np.inf and reg['lo'][2] == -np.inf and reg['hi'][2] == 4.0
    assert reg['lo'][1] == -np.inf and reg['hi'][1] == np.inf
    np.testing.assert_array_equal(vn.sourceAmplitudes(), [0.5, -1.0, 2.0])
    np.testing.assert_array_equal(vn.sourceGrad(), [0.0, 1.0, 2.0])
    vn.setSourceAmplitudes([1.0, 2.0, 3.0])
    np.testing.assert_array_equal(vn.engine.amps, [1.0, 2.0, 3.0])
    # the residual and the monitors see the source at the current amplitudes; the training streams keep s0 and the basis apart
    X = np.column_stack([np.linspace(0.05, 0.95, 7), np.linspace(0.0, 0.5, 7)])
    want = sum(a * f(X[:, :1], X[:, 1:2]) for a, f in zip([1.0, 2.0, 3.0], BASIS))
    np.testing.assert_allclose(vn.PDEinpData(X)[2], want, rtol=0, atol=1e-15)
    # one pair bounds every learnt amplitude; sourceLr defaults to the network's learning rate; True selects all
    vn = make(pde(sourceBasis=BASIS), learnSource=True, learning_rate=0.01, sourceBounds=(0, None))
    reg = vn.engine.src_reg
    assert reg['mask'] == [1, 1, 1] and reg['lr'] == 0.01 and np.all(reg['lo'] == 0.0) and np.all(np.isinf(reg['hi']))
    vn = make(learnSource=[1, 0, 1], sourceBounds=(-5.0, 5.0))
    assert list(vn.engine.src_reg['lo']) == [-5.0, -np.inf, -5.0]


@pytest.mark.parametrize('kw, msg', [
    (dict(sourceBasis=[np.sin, 3.0]), r'sourceBasis\[1\] must be callable'),
    (dict(sourceBasis=[]), 'sourceBasis must be a non-empty list'),
    (dict(sourceBasis=np.sin), 'sourceBasis must be a non-empty list'),
    (dict(sourceBasis=BASIS, sourceAmp=[1.0, 2.0]), 'sourceAmp holds 2 values for the 3 functions of sourceBasis'),
    (dict(sourceBasis=BASIS * 22), 'sourceBasis holds 66 functions, at most 64'),
    (dict(sourceBasis=BASIS, sourceAmp=[1.0, np.inf, 0.0]), 'sourceAmp must be finite'),
    (dict(sourceBasis=BASIS, sourceAmp=[1.0, np.nan, 0.0]), 'sourceAmp must be finite'),
    (dict(sourceBasis=BASIS, sourceAmp='abc'), 'sourceAmp must be a list of 3 numbers'),
    (dict(sourceAmp=[1.0]), 'sourceAmp is an option of sourceBasis'),
])
def test_malformed_pde_arguments_name_the_field(kw, msg):
    with pytest.raises(ValueError, match=msg):
        pde(**kw)


@pytest.mark.parametrize('kw, msg', [
    (dict(learnSource=[True, False]), 'learnSource must be True or a mask of 3 booleans'),
    (dict(learnSource=[1, 0, 2]), 'learnSource must be True or a mask of 3 booleans'),
    (dict(learnSource='all'), 'learnSource must be True or a mask of 3 booleans'),
    (dict(learnSource=[False] * 3), 'learnSource selects no amplitude'),
    (dict(sourceLr=0.1), 'sourceLr=0.1 is an option of learnSource'),
    (dict(sourceBounds=(0, 1)), 'sourceBounds is an option of learnSource'),
    (dict(learnSource=True, sourceLr=0.0), 'sourceLr=0.0 must be a finite number > 0'),
    (dict(learnSource=True, sourceLr=float('nan')), 'sourceLr=nan must be a finite number > 0'),
    (dict(learnSource=True, sourceLr='x'), 'sourceLr=.* must be a finite number > 0'),
    (dict(learnSource=True, sourceBounds=[(0, 1)]), r'sourceBounds must be \(lo, hi\) or a list of 3 entries'),
    (dict(learnSource=True, sourceBounds={'a': 1}), r'sourceBounds must be \(lo, hi\) or a list of 3 entries'),
    (dict(learnSource=True, sourceBounds=[1.0, None, None]), r'sourceBounds\[0\] must be None or \(lo, hi\)'),
    (dict(learnSource=True, sourceBounds=[('a', 1), None, None]), r'sourceBounds\[0\] must hold numbers or None'),
    (dict(learnSource=True, sourceBounds=[(5.0, 4.0), None, None]), 'lower bound 5.0 above upper bound 4.0'),
    (dict(learnSource=True, sourceBounds=[(1.0, None), None, None]), r'sourceBounds\[0\] = .* excludes the initial guess 0.5'),
    (dict(learnSource=True, sourceBounds=(0.0, None)), r'sourceBounds\[1\] = .* excludes the initial guess -1.0'),
    (dict(learnSource=[1, 0, 0], sourceBounds=[None, (-2, 1), None]), 'bounds an amplitude that learnSource does not select'),
])
def test_malformed_options_name_the_field(kw, msg):
    with pytest.raises(ValueError, match=msg):
        make(**kw)


def test_refusals():
    with pytest.raises(ValueError, match='learnSource: the PDE has no source basis'):
        make(pde(), learnSource=True)
    with pytest.raises(ValueError, match='learnSource needs observations=.*every amplitude admits a solution'):
        make(obs=None, learnSource=True)
    for opt in ('lbfgs', 'rmsprop', 'rms'):
        with pytest.raises(NotImplementedError, match='learnSource with optimizer='):
            make(learnSource=True, optimizer=opt)
    with pytest.raises(NotImplementedError, match='learnSource with causal=1.0'):
        make(learnSource=True, causal=1.0)
    with pytest.raises(NotImplementedError, match='learnSource with towers'):
        make(learnSource=True, processors=['GPU:0', 'GPU:1'])
    vn = make(learnSource=True)
    for bad in ([1.0, 2.0], [1.0, np.nan, 0.0], 'abc'):
        with pytest.raises(ValueError, match='setSourceAmplitudes takes 3 finite numbers'):
            vn.setSourceAmplitudes(bad)


def test_mor_is_refused():
    def diffFun(x, t=0, D=0.01):
        return D * np.ones([len(x), 1])

    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    kw = dict(diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x), MORvar=mor)
    with pytest.raises(NotImplementedError, match='a source basis with model-order reduction is not supported'):
        ADPDE(Domain1D(), sourceBasis=BASIS, **kw)
    with pytest.raises(NotImplementedError, match='learnSource with model-order reduction'):
        VarNet(ADPDE(Domain1D(), **kw), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, MORdiscScheme=[3], observations=(X4, C4),
               learnSource=True)


def test_learning_and_coefficient_learning_together():
    vn = make(pde(reaction=(1.0, [-1.0]), **FULL), learnSource=True, learnCoef={'reaction': [1, 0, 0]})
    assert vn.srcLearn is not None and vn.coefLearn is not None and vn.engine.src_reg['mask'] == [1, 1, 1]


def test_checkpoint_round_trip_of_the_amplitudes():
    vn = make(learnSource=[1, 0, 1])
    vn.engine.amps = np.array([-1.25, -1.0, 0.125])
    arrays = vn.checkpoint_arrays()
    np.testing.assert_array_equal(arrays['source_amplitudes'], vn.engine.amps)
    other = make(learnSource=[1, 0, 1])
    np.testing.assert_array_equal(other.sourceAmplitudes(), [0.5, -1.0, 2.0])
    other.restore_arrays(arrays)
    np.testing.assert_array_equal(other.engine.amps, vn.engine.amps)
    assert 'source_amplitudes' not in make().checkpoint_arrays()           # without learnSource the checkpoint is what it was


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entry_points():
    import ctypes as C
    from varnet_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    h = r'\s*vn_engine\s*\*\s*h\s*,\s*'
    assert re.search(r'int\s+vn_set_source_basis\s*\(' + h + r'int32_t\s+batch\s*,\s*const\s+float\s*\*\s*phi_dev\s*,\s*int32_t\s+J\s*\)\s*;', code)
    assert re.search(r'int\s+vn_set_source_learn\s*\(' + h + r'int32_t\s+J\s*,\s*const\s+int32_t\s*\*\s*mask\s*,\s*const\s+double\s*\*\s*init\s*,'
                     r'\s*const\s+double\s*\*\s*lo\s*,\s*const\s+double\s*\*\s*hi\s*,\s*double\s+lr\s*\)\s*;', code)
    assert re.search(r'int\s+vn_get_source_amps\s*\(' + h + r'double\s*\*\s*amp\s*,\s*double\s*\*\s*grad\s*,\s*int32_t\s+J\s*\)\s*;', code)
    assert re.search(r'int\s+vn_set_source_amps\s*\(' + h + r'const\s+double\s*\*\s*amp\s*,\s*int32_t\s+J\s*\)\s*;', code)
    assert re.search(r'#define\s+VN_SRC_MAX\s+64\b', hdr)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr)            # additive: the version stays
    for name in ('vn_set_source_basis', 'vn_set_source_learn', 'vn_get_source_amps', 'vn_set_source_amps'):
        assert name in engine.ABI_SYMBOLS
    pd = C.POINTER(C.c_double)
    assert engine._SIGS['vn_set_source_basis'] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32])
    assert engine._SIGS['vn_set_source_learn'] == (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), pd, pd, pd, C.c_double])
    assert engine._SIGS['vn_get_source_amps'] == (C.c_int, [C.c_void_p, pd, pd, C.c_int32])
    assert engine._SIGS['vn_set_source_amps'] == (C.c_int, [C.c_void_p, pd, C.c_int32])
    for name in ('set_source_basis', 'set_source_learn', 'get_source_amps', 'set_source_amps'):
        assert callable(getattr(engine.VNEngine, name))
