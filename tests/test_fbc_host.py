"""
CPU tier of flux boundary identification (vn_set_fluxbc_basis, vn_set_fluxbc_learn, `ADPDE(fluxBasis=..., fluxAmp=...,
robinBasis=..., robinAmp=...)`, `VarNet(..., learnFluxBC=..., fluxBCLr=..., fluxBCBounds=...)`): the reference tests/fbc_ref.py
against tests/flux_ref.py and against central differences, the input condition of the GPU cases from the CPU numbers alone, the
host fold of the amplitudes without learnFluxBC, the validation of every option, the refusals, the C header, the checkpoint round
trip on a stub engine, and the restatement of the mix.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import fbc_cases as fc
from tests import flux_ref
from tests.oracle_engine import OracleEngine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

pi = np.pi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _presummed(i, Jl, Jc, amp=None):
    """flux_ref's term of case i with coef and label summed beforehand: (F, dF/dtheta)."""
    c = fc.case(i)
    fx = fc.inputs(i)[1]
    coef, label = fc.mixed(i, Jl, Jc, amp)
    F, g, _ = flux_ref.flux_term(fc.theta(i).astype(np.float64), c[0], c[2], c[1], fx['X'].astype(np.float64), fx['normal'].astype(np.float64),
                                 coef, label, fc.BI_DIM_VAL, c[9])
    return F, g


@pytest.mark.parametrize('i', range(fc.N_CASES), ids=fc.IDS)
def test_reference_restates_flux_ref(i):
    """The flux mean and its theta-gradient equal tests/flux_ref.flux_term at the pre-summed coef and label to 1e-13; the amplitude
    gradient agrees with central differences of w0 F to 1e-6 of S_j (the loss is quadratic in the amplitudes: the difference
    quotient carries rounding only)."""
    Jl, Jc = 2, 1
    F, g, ga, S = fc.reference64(i, Jl, Jc)
    Fw, gw = _presummed(i, Jl, Jc)
    assert abs(F - Fw) <= 1e-13 * abs(Fw), (F, Fw)
    assert np.max(np.abs(g - gw)) <= 1e-13 * np.max(np.abs(gw))
    a0, w0 = fc.basis(i, Jl, Jc)[1], float(fc.inputs(i)[0]['w'][0])
    for j in range(Jl + Jc):
        h = 1e-3
        ap, am = a0.copy(), a0.copy()
        ap[j] += h
        am[j] -= h
        fd = w0 * (_presummed(i, Jl, Jc, ap)[0] - _presummed(i, Jl, Jc, am)[0]) / (2 * h)
        print('%s a%d: g %.6e fd %.6e S %.3e dev/S %.2e' % (fc.IDS[i], j, ga[j], fd, S[j], abs(ga[j] - fd) / S[j]))
        assert abs(ga[j] - fd) <= 1e-6 * S[j], (fc.IDS[i], j, ga[j], fd, S[j])


def test_gpu_cases_condition():
    """From the CPU numbers alone: every component is non-zero, the conditioning floor 0.01 S_j is the binding branch of the bar
    for at most 5 % of all components over all (case, J_l, J_c), and the reference evaluated in fp32 stays within the bar -- a
    change of the cases or of the basis cannot quietly widen it."""
    binding, total, least = [], 0, np.inf
    for i, Jl, Jc in fc.PAIRS:
        _, _, g64, S = fc.reference64(i, Jl, Jc)
        assert np.all(g64 != 0.0) and np.all(S > 0.0), (fc.IDS[i], Jl, Jc)
        total += Jl + Jc
        least = min(least, float(np.min(np.abs(g64) / S)))
        for j in range(Jl + Jc):
            if abs(g64[j]) < fc.COND_FLOOR * S[j]:
                binding.append((fc.IDS[i], Jl, Jc, j, abs(g64[j]) / S[j]))
        g32 = fc.evaluate(i, Jl, Jc, dtype=torch.float32)[2]
        rel = np.abs(g32 - g64) / fc.bars(g64, S)
        print('%s J=(%d, %d): fp32 restatement worst err/bar %.3f' % (fc.IDS[i], Jl, Jc, rel.max()))
        assert np.all(rel <= 1.0), (fc.IDS[i], Jl, Jc, rel)
    print('floor binding: %d of %d (least |g64| / S %.4f)' % (len(binding), total, least), binding)
    assert total == 8 * 3 + 2 * (1 + 1 + 64 + 64 + 9)
    assert len(binding) <= fc.BINDING_FRAC * total, binding


@pytest.mark.parametrize('i, Jl, Jc', fc.BIG_PAIRS, ids=['%s-%d+%d' % (fc.case_id(i), Jl, Jc) for i, Jl, Jc in fc.BIG_PAIRS])
def test_capped_grid_cases_condition(i, Jl, Jc):
    """The large-row cases, before any device is looked at: |g64| / S of the learnt entries is printed and above the floor's
    reach (non-zero, S > 0), and the fp32 restatement stays within the bar."""
    _, _, g64, S = fc.reference64(i, Jl, Jc)
    m = np.array(fc.mask_of(i, Jl, Jc), dtype=bool)
    assert np.all(g64[m] != 0.0) and np.all(S[m] > 0.0)
    print('%s (%d, %d): |g64| / S of the learnt entries %s' % (fc.case_id(i), Jl, Jc, np.abs(g64[m]) / S[m]))
    g32 = fc.evaluate(i, Jl, Jc, dtype=torch.float32)[2]
    rel = (np.abs(g32 - g64) / fc.bars(g64, S))[m]
    print('fp32 restatement worst err/bar %.3f' % rel.max())
    assert np.all(rel <= 1.0), rel


def test_cases_reach_the_row_counts():
    assert [fc.case(i)[7] for i in range(fc.N_CASES)] == [1, 30, 40, 60, 25, 2, 33, 257]
    assert [fc.case(fc.N_CASES + k)[7] for k in range(2)] == [65538, 262152] and fc.case(fc.N_CASES)[2] == [24, 31]
    assert 65538 > 256 * 256 and 65538 % 4 == 2 and 262152 > 4 * 256 * 256 and 262152 % 4 == 0
    assert 40 + 24 == 64 and 37 + 27 == 64 and 37 % 8 != 0 and 5 % 8 != 0    # the cap; the part boundary inside a group of eight
    for Jl, Jc in [(2, 1)] + fc.VARIANTS:
        S = fc.basis(1, Jl, Jc)[0]
        assert S.shape == (Jl + Jc, 30)


def test_fma_mix_restates_the_sum():
    """The fp32 mix, restated without the device: one fused multiply-add per stream from the base, within the fp32 rounding of
    the fp64 sum (J + 1 roundings of values bounded by sum |a_j S_j| + |base|); a part without streams is the base itself."""
    for i, Jl, Jc in [(1, 2, 1), (2, 40, 24), (2, 5, 4), (1, 1, 0), (1, 0, 1)]:
        S, a = fc.basis(i, Jl, Jc)
        coef32, label32 = fc.fma_mixed(i, Jl, Jc, a)
        coef64, label64 = fc.mixed(i, Jl, Jc)
        fx = fc.inputs(i)[1]
        eps = float(np.finfo(np.float32).eps)
        magl = np.abs(fx['label']).astype(np.float64) + np.abs(a[:Jl]) @ np.abs(S[:Jl]).astype(np.float64)
        magc = np.abs(fx['coef']).astype(np.float64) + np.abs(a[Jl:]) @ np.abs(S[Jl:]).astype(np.float64)
        assert coef32.dtype == np.float32 and label32.dtype == np.float32
        assert np.all(np.abs(label32 - label64) <= (Jl + 1) * eps * magl)
        assert np.all(np.abs(coef32 - coef64) <= (Jc + 1) * eps * magc)
        if Jl == 0:
            np.testing.assert_array_equal(label32, fx['label'])
        if Jc == 0:
            np.testing.assert_array_equal(coef32, fx['coef'])


# ---- the Python surface on a stub engine -----------------------------------------------------------------------------------------
class FbcStubEngine(OracleEngine):
    """The oracle engine plus the registrations the constructor makes: flux rows, observations, the amplitudes and the basis are
    only stored."""
    fbc_reg = None
    amps = None
    flux = None
    fbasis = None

    def set_observations(self, *a, **kw):
        pass

    def set_flux_bc(self, X=None, normal=None, coef=None, label=None, biDimVal=1.0):
        self.fbasis = None
        self.flux = None if X is None else dict(X=np.asarray(X), normal=np.asarray(normal), coef=np.asarray(coef), label=np.asarray(label))

    def set_fluxbc_basis(self, S=None, J_flux=0):
        self.fbasis = None if S is None else (np.asarray(S).copy(), int(J_flux))

    def set_fluxbc_learn(self, mask=None, init=None, lo=None, hi=None, lr=None):
        self.fbc_reg = None if mask is None else dict(mask=list(mask), lo=np.array(lo), hi=np.array(hi), lr=lr)
        self.amps = None if mask is None else np.asarray(init, dtype=np.float32).astype(np.float64)

    def get_fluxbc_amps(self, grad=False, J=None):
        assert J is None or J == self.amps.size
        return (self.amps.copy(), np.arange(float(self.amps.size))) if grad else self.amps.copy()

    def set_fluxbc_amps(self, amp):
        self.amps = np.asarray(amp, dtype=np.float32).astype(np.float64)

    def set_bic_learn(self, *a, **kw):
        pass

    def set_bic_basis(self, *a, **kw):
        pass

    def set_source_learn(self, *a, **kw):
        pass

    def set_source_basis(self, *a, **kw):
        pass

    def set_field_learn(self, *a, **kw):
        pass

    def set_field_basis(self, *a, **kw):
        pass

    def set_coef_learn(self, *a, **kw):
        pass


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return FbcStubEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                             isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                             learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


X4 = np.array([[0.2, 0.1], [0.4, 0.2], [0.6, 0.3], [0.8, 0.4]])
C4 = np.array([0.1, 0.2, 0.3, 0.4])
GAMMA = [(1, lambda x, t: 1.0 + t), (1, lambda x, t: np.sin(3.0 * t))]
ETA = [(1, lambda x, t: 1.0 + 0.0 * t), (0, lambda x, t: t * t)]
G0 = lambda x, t: 0.25 * np.cos(t)
IC0 = lambda x: np.sin(pi * x)
ROBIN = [[2.0, 0.0, lambda x, t: 0.0 * t], [2.0, 3.0, G0]]          # edge 0 Neumann (a = 2, b = 0), edge 1 Robin (a = 2, b = 3)


def pde(**kw):
    kw.setdefault('BCs', ROBIN)
    return ADPDE(Domain1D(np.array([0.0, 1.0])), diff=0.1, vel=0.0, tInterval=[0, 0.5], IC=IC0, **kw)


FULL = dict(fluxBasis=GAMMA, fluxAmp=[0.5, -1.0], robinBasis=ETA, robinAmp=[1.5, -0.25])


def make(p=None, obs=(X4, C4), fluxBC=True, **kw):
    return VarNet(pde(**FULL) if p is None else p, layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, observations=obs,
                  fluxBC=fluxBC, **kw)


def _want(rows, fluxAmp, robinAmp):
    """(coef, label) restated from the callables: edge 0 rows first (b/a = 0, g/a = 0), then edge 1 (b/a = 1.5, g/a = G0 / 2)."""
    (b0, t0, n0), (b1, t1, n1) = rows['edges']
    assert (b0, t0, b1, t1) == (0, 'Neumann', 1, 'Robin')
    x, t = rows['X'][:, :1], rows['X'][:, 1:2]
    coef, label = np.zeros(n0 + n1), np.zeros(n0 + n1)
    coef[n0:] = 1.5
    label[n0:] = (G0(x[n0:], t[n0:]) / 2.0).reshape(-1)
    label[n0:] += (fluxAmp[0] * GAMMA[0][1](x[n0:], t[n0:]) + fluxAmp[1] * GAMMA[1][1](x[n0:], t[n0:])).reshape(-1)
    coef[n0:] += (robinAmp[0] * ETA[0][1](x[n0:], t[n0:])).reshape(-1)
    coef[:n0] += (robinAmp[1] * ETA[1][1](x[:n0], t[:n0])).reshape(-1)
    return coef, label


def test_amplitudes_fold_into_coef_and_label_without_learning():
    """Without learnFluxBC the engine sees plain arrays: coef0 + H^T a and label0 + Gamma^T a at the constructor's amplitudes, and
    no basis; a stream is zero on the rows of other indicators; a robinBasis on a Neumann indicator is allowed."""
    vn = make()
    assert vn.fbcLearn is None and vn.engine.fbc_reg is None and vn.engine.fbasis is None
    rows = vn.fluxRows
    n0 = rows['edges'][0][2]
    coef, label = _want(rows, FULL['fluxAmp'], FULL['robinAmp'])
    np.testing.assert_allclose(rows['coef'], coef, rtol=0, atol=1e-15)
    np.testing.assert_allclose(rows['label'], label, rtol=0, atol=1e-15)
    np.testing.assert_allclose(vn.engine.flux['coef'], coef, rtol=0, atol=1e-15)
    np.testing.assert_allclose(vn.engine.flux['label'], label, rtol=0, atol=1e-15)
    assert rows['basis'] is None and rows['J_flux'] == 2
    got = vn.fluxBCAmplitudes()
    np.testing.assert_array_equal(got['flux'], [0.5, -1.0])
    np.testing.assert_array_equal(got['robin'], [1.5, -0.25])
    # amplitudes default to zeros; without a basis nothing changes
    vn0 = make(pde(fluxBasis=GAMMA, robinBasis=ETA))
    np.testing.assert_array_equal(vn0.fluxBCAmplitudes()['robin'], np.zeros(2))
    plain = make(pde())
    for k in ('coef', 'label', 'X', 'normal'):
        np.testing.assert_array_equal(vn0.fluxRows[k], plain.fluxRows[k])
    assert 'basis' not in plain.fluxRows
    with pytest.raises(ValueError, match='the PDE has no flux or Robin basis'):
        plain.fluxBCAmplitudes()
    for f in (plain.fluxBCGrad, lambda: plain.setFluxBCAmplitudes({'flux': [1.0]})):
        with pytest.raises(ValueError, match='learns no flux or Robin amplitudes'):
            f()
    assert n0 > 0


def test_registration_and_accessors():
    vn = make(learnFluxBC={'flux': [True, False], 'robin': True}, fluxBCLr=0.05,
              fluxBCBounds={'flux': [(0.0, None), None], 'robin': (-2.0, 2.0)})
    reg = vn.engine.fbc_reg
    assert reg['mask'] == [1, 0, 1, 1] and reg['lr'] == 0.05
    assert reg['lo'][0] == 0.0 and reg['hi'][0] == np.inf and reg['lo'][1] == -np.inf
    assert list(reg['lo'][2:]) == [-2.0, -2.0] and list(reg['hi'][2:]) == [2.0, 2.0]
    np.testing.assert_array_equal(vn.engine.amps, [0.5, -1.0, 1.5, -0.25])                 # one vector: flux, then robin
    g = vn.fluxBCGrad()
    np.testing.assert_array_equal(g['flux'], [0.0, 1.0])
    np.testing.assert_array_equal(g['robin'], [2.0, 3.0])
    vn.setFluxBCAmplitudes({'robin': [1.0, 2.0]})
    np.testing.assert_array_equal(vn.engine.amps, [0.5, -1.0, 1.0, 2.0])
    np.testing.assert_array_equal(vn.fluxBCAmplitudes()['robin'], [1.0, 2.0])
    # with learnFluxBC the engine gets b/a, g/a and the [J, nF] streams apart, "flux, then robin", each on its own indicator's rows
    rows = vn.fluxRows
    n0 = rows['edges'][0][2]
    coef0, label0 = _want(rows, [0, 0], [0, 0])
    np.testing.assert_allclose(vn.engine.flux['coef'], coef0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(vn.engine.flux['label'], label0, rtol=0, atol=1e-15)
    S, Jl = vn.engine.fbasis
    assert Jl == 2 and S.shape == (4, rows['X'].shape[0]) and S.dtype == np.float64
    assert np.all(S[:3, :n0] == 0) and np.all(S[3, n0:] == 0) and np.all(S[0, n0:] != 0) and np.all(S[2, n0:] == 1.0)
    x, t = rows['X'][:, :1], rows['X'][:, 1:2]
    np.testing.assert_allclose(S[1, n0:], np.sin(3.0 * t[n0:]).reshape(-1), rtol=0, atol=1e-15)
    np.testing.assert_allclose(S[3, :n0], (t[:n0] ** 2).reshape(-1), rtol=0, atol=1e-15)
    # a key left out: none of that basis is learnt; fluxBCLr defaults to the network's learning rate
    vn = make(learnFluxBC={'robin': True}, learning_rate=0.01)
    assert vn.engine.fbc_reg['mask'] == [0, 0, 1, 1] and vn.engine.fbc_reg['lr'] == 0.01
    vn = make(pde(robinBasis=ETA), learnFluxBC={'robin': [0, 1]})
    assert vn.engine.fbc_reg['mask'] == [0, 1] and vn.engine.fbasis[1] == 0


@pytest.mark.parametrize('name, amp', [('fluxBasis', 'fluxAmp'), ('robinBasis', 'robinAmp')])
def test_malformed_pde_arguments_name_the_field(name, amp):
    f = lambda x, t: t
    two = [(1, f), (1, f)]
    for kw, msg in [
        ({name: [(1, 3.0)]}, r'%s\[0\]: the function must be callable' % name),
        ({name: [np.sin]}, r'%s\[0\] must be a pair \(bInd, f\)' % name),
        ({name: []}, '%s must be a non-empty list' % name),
        ({name: [(2, f)]}, r'%s\[0\]: boundary indicator 2 outside \[0, 2\)' % name),
        ({name: [(-1, f)]}, r'%s\[0\]: boundary indicator -1 outside' % name),
        ({name: [(1, f), (0, f)], 'BCs': [[], [1.0, 0.0, 0.0]]}, r'%s\[1\]: boundary indicator 0 carries a Dirichlet condition' % name),
        ({name: [(0, f)], 'BCs': [[], []], 'periodic': [(0, 1)]}, r'%s\[0\]: boundary indicator 0 is paired by `periodic`' % name),
        ({name: two, amp: [1.0]}, '%s holds 1 values for the 2 functions of %s' % (amp, name)),
        ({name: two, amp: [1.0, np.inf]}, '%s must be finite' % amp),
        ({name: two, amp: 'abc'}, '%s must be a list of 2 numbers' % amp),
        ({amp: [1.0]}, '%s is an option of %s' % (amp, name)),
        ({name: two * 33}, '%s holds 66 functions, at most 64' % name),
    ]:
        with pytest.raises(ValueError, match=msg):
            pde(**kw)
    with pytest.raises(ValueError, match='fluxBasis and robinBasis hold 65 functions together, at most 64'):
        pde(fluxBasis=two * 16, robinBasis=[(0, f)] * 33)
    pde(fluxBasis=two * 16, robinBasis=[(0, f)] * 32)                        # 64 together: accepted


@pytest.mark.parametrize('kw, msg', [
    (dict(learnFluxBC=True), 'learnFluxBC must be a dict'),
    (dict(learnFluxBC={'flux': True, 'edge': True}), 'learnFluxBC must be a dict'),
    (dict(learnFluxBC={'flux': [True]}), r"learnFluxBC\['flux'\] must be True or a mask of 2 booleans"),
    (dict(learnFluxBC={'robin': [1, 2]}), r"learnFluxBC\['robin'\] must be True or a mask of 2 booleans"),
    (dict(learnFluxBC={'flux': [False] * 2}), 'learnFluxBC selects no amplitude'),
    (dict(fluxBCLr=0.1), 'fluxBCLr=0.1 is an option of learnFluxBC'),
    (dict(fluxBCBounds={'flux': (0, 1)}), 'fluxBCBounds is an option of learnFluxBC'),
    (dict(learnFluxBC={'flux': True}, fluxBCLr=0.0), 'fluxBCLr=0.0 must be a finite number > 0'),
    (dict(learnFluxBC={'flux': True}, fluxBCLr=float('nan')), 'fluxBCLr=nan must be a finite number > 0'),
    (dict(learnFluxBC={'flux': True}, fluxBCBounds=(0, 1)), 'fluxBCBounds must be a dict'),
    (dict(learnFluxBC={'flux': True}, fluxBCBounds={'flux': [(0, 1)]}), r"fluxBCBounds\['flux'\] must be \(lo, hi\) or a list of 2 entries"),
    (dict(learnFluxBC={'flux': True}, fluxBCBounds={'flux': [(5.0, 4.0), None]}), 'lower bound 5.0 above upper bound 4.0'),
    (dict(learnFluxBC={'flux': True}, fluxBCBounds={'flux': [(1.0, None), None]}), r'excludes the initial guess 0.5'),
    (dict(learnFluxBC={'flux': [1, 0]}, fluxBCBounds={'flux': [None, (-2, 1)]}), 'bounds an amplitude that learnFluxBC does not select'),
])
def test_malformed_options_name_the_field(kw, msg):
    with pytest.raises(ValueError, match=msg):
        make(**kw)


def test_refusals():
    with pytest.raises(ValueError, match=r"learnFluxBC\['flux'\]: the PDE has no flux basis"):
        make(pde(robinBasis=ETA), learnFluxBC={'flux': True})
    with pytest.raises(ValueError, match=r"learnFluxBC\['robin'\]: the PDE has no robin basis"):
        make(pde(fluxBasis=GAMMA), learnFluxBC={'robin': True})
    with pytest.raises(ValueError, match=r"fluxBCBounds\['robin'\]: the PDE has no robin basis"):
        make(pde(fluxBasis=GAMMA), learnFluxBC={'flux': True}, fluxBCBounds={'robin': (0, 1)})
    with pytest.raises(ValueError, match='fluxBasis / robinBasis.*needs fluxBC=True'):
        make(fluxBC=False)
    with pytest.raises(ValueError, match='fluxBasis / robinBasis.*needs fluxBC=True'):
        make(pde(robinBasis=ETA), fluxBC=False, learnFluxBC={'robin': True})
    with pytest.raises(ValueError, match='learnFluxBC needs observations=.*every amplitude admits a solution'):
        make(obs=None, learnFluxBC={'flux': True})
    for opt in ('lbfgs', 'rmsprop', 'rms'):
        with pytest.raises(NotImplementedError, match='learnFluxBC with optimizer='):
            make(learnFluxBC={'flux': True}, optimizer=opt)
    with pytest.raises(NotImplementedError, match='learnFluxBC with causal=1.0'):
        make(learnFluxBC={'flux': True}, causal=1.0)
    with pytest.raises(NotImplementedError, match='learnFluxBC with towers'):
        make(learnFluxBC={'flux': True}, processors=['GPU:0', 'GPU:1'])
    vn = make(learnFluxBC={'flux': True})
    for bad in ({'flux': [1.0]}, {'flux': [1.0, np.nan]}, {'robin': 'abc'}):
        with pytest.raises(ValueError, match=r'setFluxBCAmplitudes\[.*\] takes \d finite numbers'):
            vn.setFluxBCAmplitudes(bad)
    with pytest.raises(ValueError, match='setFluxBCAmplitudes takes a dict'):
        vn.setFluxBCAmplitudes([1.0, 2.0])


def test_mor_is_refused():
    def diffFun(x, t=0, D=0.01):
        return D * np.ones([len(x), 1])

    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    kw = dict(diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x), MORvar=mor,
              BCs=[[], [1.0, 0.0, 0.0]])
    with pytest.raises(NotImplementedError, match='fluxBasis with model-order reduction is not supported'):
        ADPDE(Domain1D(), fluxBasis=[(1, lambda x, t: t)], **kw)
    with pytest.raises(NotImplementedError, match='robinBasis with model-order reduction is not supported'):
        ADPDE(Domain1D(), robinBasis=[(1, lambda x, t: t)], **kw)
    with pytest.raises(NotImplementedError, match='learnFluxBC with model-order reduction'):
        VarNet(ADPDE(Domain1D(), **kw), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, MORdiscScheme=[3], observations=(X4, C4),
               learnFluxBC={'flux': True})


def test_learning_next_to_the_other_vectors():
    src = [lambda x, t: np.sin(pi * x)]
    ic = [lambda x: np.sin(2 * pi * x)]
    vn = make(pde(reaction=(1.0, [-1.0]), sourceBasis=src, diffBasis=[1.0], icBasis=ic, **FULL), learnFluxBC={'robin': True},
              learnSource=True, learnField={'diff': True}, learnCoef={'reaction': [1, 0, 0]}, learnBic={'ic': True})
    assert all(getattr(vn, a) is not None for a in ('fbcLearn', 'srcLearn', 'fldLearn', 'coefLearn', 'bicLearn'))
    assert vn.engine.fbc_reg['mask'] == [0, 0, 1, 1]
    assert [lv.option for lv in VarNet.LEARNT] == ['learnCoef', 'learnSource', 'learnField', 'learnBic', 'learnFluxBC']
    assert VarNet.LEARNT[4].key == 'fluxbc_amplitudes'


def test_checkpoint_round_trip_of_the_amplitudes():
    vn = make(learnFluxBC={'flux': [1, 0], 'robin': True})
    vn.engine.amps = np.array([-1.25, -1.0, 0.125, 3.0])
    arrays = vn.checkpoint_arrays()
    np.testing.assert_array_equal(arrays['fluxbc_amplitudes'], vn.engine.amps)
    other = make(learnFluxBC={'flux': [1, 0], 'robin': True})
    np.testing.assert_array_equal(other.fluxBCAmplitudes()['robin'], [1.5, -0.25])
    other.restore_arrays(arrays)
    np.testing.assert_array_equal(other.engine.amps, vn.engine.amps)
    assert 'fluxbc_amplitudes' not in make().checkpoint_arrays()            # without learnFluxBC the checkpoint is what it was


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entry_points():
    import ctypes as C
    from varnet_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    h = r'\s*vn_engine\s*\*\s*h\s*,\s*'
    assert re.search(r'int\s+vn_set_fluxbc_basis\s*\(' + h + r'const\s+float\s*\*\s*S_dev\s*,\s*int32_t\s+J_flux\s*,\s*int32_t\s+J_robin\s*\)\s*;', code)
    assert re.search(r'int\s+vn_set_fluxbc_learn\s*\(' + h + r'int32_t\s+J\s*,\s*const\s+int32_t\s*\*\s*mask\s*,\s*const\s+double\s*\*\s*init\s*,'
                     r'\s*const\s+double\s*\*\s*lo\s*,\s*const\s+double\s*\*\s*hi\s*,\s*double\s+lr\s*\)\s*;', code)
    assert re.search(r'int\s+vn_get_fluxbc_amps\s*\(' + h + r'double\s*\*\s*amp\s*,\s*double\s*\*\s*grad\s*,\s*int32_t\s+J\s*\)\s*;', code)
    assert re.search(r'int\s+vn_set_fluxbc_amps\s*\(' + h + r'const\s+double\s*\*\s*amp\s*,\s*int32_t\s+J\s*\)\s*;', code)
    assert re.search(r'#define\s+VN_FBC_MAX\s+64\b', hdr)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr)            # additive: the version stays
    for name in ('vn_set_fluxbc_basis', 'vn_set_fluxbc_learn', 'vn_get_fluxbc_amps', 'vn_set_fluxbc_amps'):
        assert name in engine.ABI_SYMBOLS
    pd = C.POINTER(C.c_double)
    assert engine._SIGS['vn_set_fluxbc_basis'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32])
    assert engine._SIGS['vn_set_fluxbc_learn'] == (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), pd, pd, pd, C.c_double])
    assert engine._SIGS['vn_get_fluxbc_amps'] == (C.c_int, [C.c_void_p, pd, pd, C.c_int32])
    assert engine._SIGS['vn_set_fluxbc_amps'] == (C.c_int, [C.c_void_p, pd, C.c_int32])
    assert engine.LEARNT['fluxbc'] == ('fluxbc_amps', None)
    for name in ('set_fluxbc_basis', 'set_fluxbc_learn', 'get_fluxbc_amps', 'set_fluxbc_amps'):
        assert callable(getattr(engine.VNEngine, name))
