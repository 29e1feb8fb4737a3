"""
CPU tier of field identification (vn_set_field_basis, vn_set_field_learn, `ADPDE(diffBasis=..., diffAmp=..., d_diffBasis=...,
velBasis=..., velAmp=...)`, `VarNet(..., learnField=..., fieldLr=..., fieldBounds=...)`): the reference tests/field_ref.py against
tests/inverse_ref.py and against central differences, the input condition of the GPU cases from the CPU numbers alone, the host
fold of the amplitudes without learnField, the streams the host hands the engine with it, the validation of every option, the
refusals, the C header, and the checkpoint round trip on a stub engine.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import field_cases as fc
from tests import inverse_ref
from tests.oracle_engine import OracleEngine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

pi = np.pi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _premixed(i, J, amp=None, gcoef=None):
    """inverse_ref's evaluation of case i with gcoef = g0 + sum_j b_j G_j summed beforehand (gcoef: another direction)."""
    nldiff, nlflux, reaction = fc.terms_of(i)
    kw = fc.ref_kw(i)
    kw['gcoef'] = fc.mixed(i, J, amp) if gcoef is None else gcoef
    return inverse_ref.evaluate(fc.theta(i), fc.case(i)[0], fc.case(i)[2], fc.coefs_of(i), nldiff, nlflux, reaction, torch.float64, **kw)


def _same(res, g, want, gw, tol=1e-13):
    for k in ('loss', 'BCloss', 'ICloss', 'varLoss'):
        assert abs(res[k] - want[k]) <= tol * abs(want[k]), (k, res[k], want[k])
    assert np.max(np.abs(res['lossVec'] - want['lossVec'])) <= tol * np.max(np.abs(want['lossVec']))
    assert np.max(np.abs(g - gw)) <= tol * np.max(np.abs(gw))


@pytest.mark.parametrize('i', range(fc.N_CASES), ids=fc.IDS)
def test_reference_restates_inverse_ref(i):
    """At b = 0 the reference equals tests/inverse_ref.evaluate on g0, and at the case's amplitudes on the pre-mixed gcoef, to
    1e-13 (loss pieces, lossVec, theta-gradient); the amplitude gradient agrees with central differences of that loss to 1e-6 of
    S_j.  D(u) multiplies A_r = grad u . gcoef and does not depend on b, so the loss is quadratic in the amplitudes for every D:
    the central difference is exact up to rounding at any step, and h = 1e-3 keeps the rounding of the difference (1e-16 loss / h)
    far below 1e-6 S_j."""
    J = 3
    res, g, gb, S = fc.reference64(i, J)
    _same(res, g, *_premixed(i, J)[:2])
    res0, g0, _, _ = fc.evaluate(i, J, amp=np.zeros(J))
    _same(res0, g0, *_premixed(i, J, gcoef=fc.inputs(i)['gcoef'].astype(np.float64))[:2])
    resn, gn, gbn, Sn = fc.evaluate(i, J, with_basis=False)
    _same(resn, gn, res0, g0, tol=0.0)
    assert gbn.size == 0 and Sn.size == 0
    b0 = fc.basis(i, J)[1]
    for j in range(J):
        h = 1e-3
        bp, bm = b0.copy(), b0.copy()
        bp[j] += h
        bm[j] -= h
        fd = (_premixed(i, J, bp)[0]['loss'] - _premixed(i, J, bm)[0]['loss']) / (2 * h)
        print('%s b%d: g %.6e fd %.6e S %.3e dev/S %.2e' % (fc.IDS[i], j, gb[j], fd, S[j], abs(gb[j] - fd) / S[j]))
        assert abs(gb[j] - fd) <= 1e-6 * S[j], (fc.IDS[i], j, gb[j], fd, S[j])


def test_gpu_cases_condition():
    """From the CPU numbers alone: every component is non-zero, the conditioning floor 0.01 S_j is the binding branch of the bar
    for at most 5 % of all components over all (case, J), and the reference evaluated in fp32 stays within the bar -- a change of
    the cases or of the basis cannot quietly widen it."""
    binding, total, worst = [], 0, 0.0
    for i, J in fc.PAIRS:
        _, _, g64, S = fc.reference64(i, J)
        assert np.all(g64 != 0.0) and np.all(S > 0.0), (fc.IDS[i], J)
        total += J
        for j in range(J):
            if abs(g64[j]) < fc.COND_FLOOR * S[j]:
                binding.append((fc.IDS[i], J, j, abs(g64[j]) / S[j]))
        g32 = fc.evaluate(i, J, dtype=torch.float32)[2]
        rel = np.abs(g32 - g64) / fc.bars(g64, S)
        worst = max(worst, rel.max())
        print('%s J=%d: fp32 restatement worst err/bar %.3f' % (fc.IDS[i], J, rel.max()))
        assert np.all(rel <= 1.0), (fc.IDS[i], J, rel)
    print('floor binding: %d of %d; fp32 restatement worst err/bar %.3f' % (len(binding), total, worst), binding)
    assert len(binding) <= fc.BINDING_FRAC * total, binding


@pytest.mark.parametrize('i', range(fc.N_CASES), ids=fc.IDS)
def test_leaving_the_basis_out_moves_everything(i):
    """(A condition on the inputs.)  Loss, lossVec and every block of the theta-gradient move by >= 100 x the bar each is compared
    at when the basis is left out: an engine that ignored the registered streams could not pass the GPU tier."""
    from tests.gradcheck import block_errors
    from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL
    J = 3
    res, g, _, _ = fc.reference64(i, J)
    res0, g0, _, _ = fc.evaluate(i, J, with_basis=False)
    assert abs(res0['loss'] - res['loss']) >= 100 * LOSS_RTOL * abs(res['loss'])
    assert abs(res0['varLoss'] - res['varLoss']) >= 100 * LOSS_RTOL * abs(res['varLoss'])
    assert np.max(np.abs(res0['lossVec'] - res['lossVec'])) >= 100 * LVEC_RTOL * np.max(np.abs(res['lossVec']))
    errs = block_errors(g0, g, fc.case(i)[0], fc.case(i)[2], fc.case(i)[1], fc.case(i)[10])
    print('%s: without the basis the gradient blocks move by %s' % (fc.IDS[i], errs))
    assert min(errs.values()) >= 100 * GRAD_RTOL, errs


def test_cases_reach_the_row_paths_and_both_kinds_of_stream():
    """nT dim % 4 != 0 on case 6 (the one-entry mix kernel), a multiple of 4 elsewhere; dim 1 to 3; streams of the diffusivity kind
    are pointwise parallel to gcoef, those of the velocity kind are not."""
    assert (fc.inputs(6)['Input'].shape[0] * fc.case(6)[1]) % 4 == 2
    assert (fc.inputs(0)['Input'].shape[0] * fc.case(0)[1]) % 4 == 0
    assert sorted({fc.case(i)[1] for i in range(fc.N_CASES)}) == [1, 2, 3]
    for J in (1, 3, 5, fc.JMAX):
        G = fc.basis(0, J)[0]
        g0 = fc.inputs(0)['gcoef']
        assert G.shape == (J,) + g0.shape and G.dtype == np.float32
        cross = lambda a: a[:, 0] * g0[:, 1] - a[:, 1] * g0[:, 0]
        assert np.max(np.abs(cross(G[0]))) <= 1e-5 * np.max(np.abs(G[0])) * np.max(np.abs(g0))
        if J > 1:
            assert np.max(np.abs(cross(G[1]))) >= 0.1 * np.max(np.abs(g0)) ** 2
    for i, J in fc.PAIRS:
        assert 1 <= J <= 32


# ---- the Python surface on a stub engine -----------------------------------------------------------------------------------------
class FieldStubEngine(OracleEngine):
    """The oracle engine plus the registrations the constructor and the training set make: observations, the amplitudes and the
    basis streams are only stored."""
    fld_reg = None
    amps = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.fld_basis = {}

    def set_observations(self, *a, **kw):
        pass

    def set_coef_learn(self, *a, **kw):
        pass

    def set_source_learn(self, *a, **kw):
        pass

    def set_source_basis(self, *a, **kw):
        pass

    def set_field_basis(self, batch, G=None):
        self.fld_basis[batch] = None if G is None else G.numpy().copy()

    def set_field_learn(self, mask=None, init=None, lo=None, hi=None, lr=None):
        self.fld_reg = None if mask is None else dict(mask=list(mask), lo=np.array(lo), hi=np.array(hi), lr=lr)
        self.amps = None if mask is None else np.asarray(init, dtype=np.float32).astype(np.float64)

    def get_field_amps(self, grad=False, J=None):
        assert J is None or J == self.amps.size
        return (self.amps.copy(), np.arange(float(self.amps.size))) if grad else self.amps.copy()

    def set_field_amps(self, amp):
        self.amps = np.asarray(amp, dtype=np.float32).astype(np.float64)


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return FieldStubEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                               isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                               learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


X4 = np.array([[0.2, 0.1], [0.4, 0.2], [0.6, 0.3], [0.8, 0.4]])
C4 = np.array([0.1, 0.2, 0.3, 0.4])
X7 = np.column_stack([np.linspace(0.05, 0.95, 7), np.linspace(0.0, 0.5, 7)])
CHI = [lambda x, t: np.sin(pi * x) * (1.0 + t), 1.0]
DCHI = [lambda x, t: pi * np.cos(pi * x) * (1.0 + t), None]
OMEGA = [lambda x, t: np.cos(pi * x) + t, 2.0, lambda x, t: x * x]
KAPPA0 = lambda x, t: 0.1 + 0.05 * x
DKAPPA0 = lambda x, t: 0.05 + 0.0 * x
VEL0 = lambda x, t: 0.3 * x - t
BK, BV = [0.5, -0.02], [0.25, -1.0, 2.0]


def pde(**kw):
    kw.setdefault('diff', KAPPA0)
    kw.setdefault('vel', VEL0)
    return ADPDE(Domain1D(np.array([0.0, 1.0])), tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x), **kw)


FULL = dict(d_diff=DKAPPA0, diffBasis=CHI, diffAmp=BK, d_diffBasis=DCHI, velBasis=OMEGA, velAmp=BV)


def make(p=None, obs=(X4, C4), **kw):
    return VarNet(pde(**FULL) if p is None else p, layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, observations=obs, **kw)


def summed(bk=BK, bv=BV):
    """The fields of FULL at the amplitudes (bk, bv) as plain callables."""
    kappa = lambda x, t: KAPPA0(x, t) + bk[0] * CHI[0](x, t) + bk[1] * 1.0
    dkappa = lambda x, t: DKAPPA0(x, t) + bk[0] * DCHI[0](x, t)
    vel = lambda x, t: VEL0(x, t) + bv[0] * OMEGA[0](x, t) + bv[1] * 2.0 + bv[2] * OMEGA[2](x, t)
    return kappa, dkappa, vel


def test_amplitudes_fold_into_the_fields_without_learning():
    """Without learnField the engine sees a plain gcoef: that of a plain ADPDE with the summed callables."""
    kappa, dkappa, vel = summed()
    x, t = X7[:, :1], X7[:, 1:2]
    vn = make()
    assert vn.fldLearn is None and vn.engine.fld_reg is None
    d, v, _ = vn.PDEinpData(X7)
    np.testing.assert_allclose(d, kappa(x, t), rtol=0, atol=1e-15)
    np.testing.assert_allclose(v, vel(x, t), rtol=0, atol=1e-15)
    np.testing.assert_allclose(vn.diffGradData(X7), dkappa(x, t), rtol=0, atol=1e-15)
    np.testing.assert_allclose(vn.PDE.diffFun(x, t), kappa(x, t), rtol=0, atol=1e-15)
    np.testing.assert_allclose(vn.PDE.velFun(x, t), vel(x, t), rtol=0, atol=1e-15)
    np.testing.assert_allclose(vn.PDE.d_diffFun(x, t), dkappa(x, t), rtol=0, atol=1e-15)
    d0, v0, _ = vn.PDEinpData(X7, field=False)
    np.testing.assert_array_equal(d0, KAPPA0(x, t))
    np.testing.assert_array_equal(v0, VEL0(x, t))
    amps = vn.fieldAmplitudes()
    np.testing.assert_array_equal(amps['diff'], BK)
    np.testing.assert_array_equal(amps['vel'], BV)
    plain = make(pde(diff=kappa, vel=vel, d_diff=dkappa))
    a, b = vn._build_tdata(), plain._build_tdata()
    assert vn.engine.fld_basis == {} and a.mor[0]['fldG'] is None
    np.testing.assert_allclose(vn.engine.batches[0][1], plain.engine.batches[0][1], rtol=0, atol=1e-14)
    # the amplitudes default to zeros; without a basis nothing changes
    vn = make(pde(diffBasis=CHI, velBasis=OMEGA))
    np.testing.assert_array_equal(vn.fieldAmplitudes()['vel'], np.zeros(3))
    np.testing.assert_array_equal(vn.PDEinpData(X7)[0], KAPPA0(x, t))
    vn = make(pde())
    with pytest.raises(ValueError, match='the PDE has no field basis'):
        vn.fieldAmplitudes()
    for f in (vn.fieldGrad, lambda: vn.setFieldAmplitudes({'diff': [1.0]})):
        with pytest.raises(ValueError, match='learns no field amplitudes'):
            f()


def test_streams_handed_to_the_engine_with_learning():
    """With learnField the engine gets g0 of the plain fields and one [J, nT, dim] tensor, the diffusivity streams first:
    g0 + sum_j b_j G_j is the gcoef of the summed fields; every block of the training set gets its rows, also after a shuffle."""
    kappa, dkappa, vel = summed()
    vn = make(learnField={'diff': True, 'vel': [1, 0, 1]})
    plain, base = make(pde(diff=kappa, vel=vel, d_diff=dkappa)), make(pde(d_diff=DKAPPA0))
    td, tp, tb = vn._build_tdata(batchNum=2), plain._build_tdata(batchNum=2), base._build_tdata(batchNum=2)
    b = np.array(BK + BV)
    for k in (0, 1):
        G, g0 = vn.engine.fld_basis[k], vn.engine.batches[k][1]
        assert G.shape == (5,) + g0.shape
        np.testing.assert_array_equal(g0, base.engine.batches[k][1])
        np.testing.assert_allclose(g0 + np.tensordot(b, G, axes=1), plain.engine.batches[k][1], rtol=0, atol=1e-14)
    np.random.seed(3)
    td.shuffleTrainData()
    np.random.seed(3)
    tp.shuffleTrainData()
    for k in (0, 1):
        G, g0 = vn.engine.fld_basis[k], vn.engine.batches[k][1]
        np.testing.assert_allclose(g0 + np.tensordot(b, G, axes=1), plain.engine.batches[k][1], rtol=0, atol=1e-14)
    # a velocity stream is omega N, a diffusivity stream chi dN/dx: the constant chi_2 = 1 gives dN/dx itself
    fd = vn.fixData
    G = td.mor[0]['fldG'].numpy()
    np.testing.assert_allclose(G[1].reshape(fd.nt, fd.integNum, 1), np.broadcast_to(fd.dNx[None], (fd.nt, fd.integNum, 1)), atol=1e-15)
    np.testing.assert_allclose(G[3].reshape(fd.nt, fd.integNum), 2.0 * np.broadcast_to(np.reshape(fd.N, -1)[None], (fd.nt, fd.integNum)),
                               atol=1e-15)


def test_registration_and_accessors():
    vn = make(learnField={'diff': [True, False], 'vel': True}, fieldLr=0.05,
              fieldBounds={'diff': [(0.0, None), None], 'vel': (-3.0, 4.0)})
    reg = vn.engine.fld_reg
    assert reg['mask'] == [1, 0, 1, 1, 1] and reg['lr'] == 0.05
    assert list(reg['lo']) == [0.0, -np.inf, -3.0, -3.0, -3.0] and list(reg['hi']) == [np.inf, np.inf, 4.0, 4.0, 4.0]
    np.testing.assert_array_equal(vn.fieldAmplitudes()['diff'], np.float32(BK).astype(np.float64))
    g = vn.fieldGrad()
    np.testing.assert_array_equal(g['diff'], [0.0, 1.0])
    np.testing.assert_array_equal(g['vel'], [2.0, 3.0, 4.0])
    vn.setFieldAmplitudes({'vel': [1.0, 2.0, 3.0]})
    np.testing.assert_array_equal(vn.engine.amps, list(np.float32(BK).astype(np.float64)) + [1.0, 2.0, 3.0])
    vn.setFieldAmplitudes({'diff': [0.25, 0.5], 'vel': [1.0, 2.0, 4.0]})
    np.testing.assert_array_equal(vn.engine.amps, [0.25, 0.5, 1.0, 2.0, 4.0])
    # PDEinpData, and so Residual, simRes and residual(), see kappa, v and grad kappa at the current amplitudes
    kappa, dkappa, vel = summed([0.25, 0.5], [1.0, 2.0, 4.0])
    x, t = X7[:, :1], X7[:, 1:2]
    d, v, _ = vn.PDEinpData(X7)
    np.testing.assert_allclose(d, kappa(x, t), rtol=0, atol=1e-15)
    np.testing.assert_allclose(v, vel(x, t), rtol=0, atol=1e-14)
    np.testing.assert_allclose(vn.diffGradData(X7), dkappa(x, t), rtol=0, atol=1e-15)
    # only one basis, a key left out, fieldLr defaults to the network's learning rate
    vn = make(pde(velBasis=[1.0]), learnField={'vel': True}, learning_rate=0.01)
    assert vn.engine.fld_reg['mask'] == [1] and vn.engine.fld_reg['lr'] == 0.01
    vn = make(learnField={'diff': True})
    assert vn.engine.fld_reg['mask'] == [1, 1, 0, 0, 0]


def test_residual_reads_the_current_fields():
    """residual() hands the engine kappa, v and grad kappa at the current amplitudes, on the uniform set too."""
    seen = {}

    def residual(self, X, diff, vel, source=None, diff_dx=None, fp64=False, **kw):
        seen.update(diff=np.array(diff), vel=np.array(vel), ddx=np.array(diff_dx))
        z = torch.zeros(X.shape[0], dtype=torch.float64)
        return z, z
    vn = make(pde(cEx=None, **FULL), learnField={'diff': True, 'vel': True})
    type(vn.engine).residual = residual
    try:
        ui = vn.fixData.uniform_input
        x, t = ui[:, :1], ui[:, 1:2]
        for bk, bv in ((BK, BV), ([0.25, 0.5], [1.0, 2.0, 4.0])):
            vn.setFieldAmplitudes({'diff': bk, 'vel': bv})
            bk32, bv32 = [float(np.float32(v)) for v in bk], [float(np.float32(v)) for v in bv]
            kappa, dkappa, vel = summed(bk32, bv32)
            vn.residual()
            np.testing.assert_allclose(seen['diff'], kappa(x, t), rtol=0, atol=1e-14)
            np.testing.assert_allclose(seen['vel'], vel(x, t), rtol=0, atol=1e-14)
            np.testing.assert_allclose(seen['ddx'], dkappa(x, t), rtol=0, atol=1e-14)
    finally:
        del type(vn.engine).residual


@pytest.mark.parametrize('kw, msg', [
    (dict(diffBasis=[np.sin, 'a']), r'diffBasis\[1\] must be callable, a finite number!'),
    (dict(diffBasis=[np.sin, [1.0, 2.0]]), r'diffBasis\[1\] must be callable, a finite number!'),
    (dict(velBasis=[np.sin, np.inf]), r'velBasis\[1\] must be callable, a finite number'),
    (dict(diffBasis=[]), 'diffBasis must be a non-empty list'),
    (dict(velBasis=np.sin), 'velBasis must be a non-empty list'),
    (dict(diffBasis=CHI, diffAmp=[1.0]), 'diffAmp holds 1 values for the 2 functions of diffBasis'),
    (dict(velBasis=OMEGA, velAmp=[1.0, 2.0]), 'velAmp holds 2 values for the 3 functions of velBasis'),
    (dict(diffBasis=CHI * 17), 'diffBasis holds 34 functions, at most 32'),
    (dict(diffBasis=CHI * 10, velBasis=OMEGA * 5), 'diffBasis and velBasis hold 35 functions together, at most 32'),
    (dict(diffBasis=CHI, diffAmp=[1.0, np.inf]), 'diffAmp must be finite'),
    (dict(velBasis=OMEGA, velAmp=[1.0, np.nan, 0.0]), 'velAmp must be finite'),
    (dict(velBasis=OMEGA, velAmp='abc'), 'velAmp must be a list of 3 numbers'),
    (dict(diffAmp=[1.0]), 'diffAmp is an option of diffBasis'),
    (dict(velAmp=[1.0]), 'velAmp is an option of velBasis'),
    (dict(d_diffBasis=DCHI), 'd_diffBasis is an option of diffBasis'),
    (dict(diffBasis=CHI, d_diffBasis=DCHI[:1]), 'd_diffBasis must be a list of 2 entries'),
    (dict(diffBasis=CHI, d_diffBasis=[DCHI[0], 'x']), r'd_diffBasis\[1\] must be callable, a finite number'),
])
def test_malformed_pde_arguments_name_the_field(kw, msg):
    with pytest.raises(ValueError, match=msg):
        pde(**kw)


def test_basis_functions_of_the_wrong_shape_name_the_entry():
    with pytest.raises(ValueError, match=r'diffBasis\[0\] must return one value \(a column\) per point'):
        make(pde(diffBasis=[lambda x, t: np.ones(3)]))
    with pytest.raises(ValueError, match=r'velBasis\[1\] must return one value \(a column\) per point, got shape \(3,\)'):
        make(pde(velBasis=[1.0, lambda x, t: np.ones(3)]))


@pytest.mark.parametrize('kw, msg', [
    (dict(learnField=True), 'learnField must be a dict'),
    (dict(learnField={}), 'learnField must be a dict'),
    (dict(learnField={'kappa': True}), 'learnField must be a dict'),
    (dict(learnField={'diff': [True]}), r"learnField\['diff'\] must be True or a mask of 2 booleans"),
    (dict(learnField={'vel': [1, 0, 2]}), r"learnField\['vel'\] must be True or a mask of 3 booleans"),
    (dict(learnField={'vel': 'all'}), r"learnField\['vel'\] must be True or a mask of 3 booleans"),
    (dict(learnField={'diff': [False] * 2, 'vel': False}), 'learnField selects no amplitude'),
    (dict(fieldLr=0.1), 'fieldLr=0.1 is an option of learnField'),
    (dict(fieldBounds={'diff': (0, 1)}), 'fieldBounds is an option of learnField'),
    (dict(learnField={'diff': True}, fieldLr=0.0), 'fieldLr=0.0 must be a finite number > 0'),
    (dict(learnField={'diff': True}, fieldLr=float('nan')), 'fieldLr=nan must be a finite number > 0'),
    (dict(learnField={'diff': True}, fieldLr='x'), 'fieldLr=.* must be a finite number > 0'),
    (dict(learnField={'diff': True}, fieldBounds=(0, 1)), 'fieldBounds must be a dict'),
    (dict(learnField={'diff': True}, fieldBounds={'kappa': (0, 1)}), 'fieldBounds must be a dict'),
    (dict(learnField={'diff': True}, fieldBounds={'diff': [(0, 1)]}), r"fieldBounds\['diff'\] must be \(lo, hi\) or a list of 2 entries"),
    (dict(learnField={'vel': True}, fieldBounds={'vel': [1.0, None, None]}), r"fieldBounds\['vel'\]\[0\] must be None or \(lo, hi\)"),
    (dict(learnField={'diff': True}, fieldBounds={'diff': [('a', 1), None]}), r"fieldBounds\['diff'\]\[0\] must hold numbers or None"),
    (dict(learnField={'diff': True}, fieldBounds={'diff': [(5.0, 4.0), None]}), 'lower bound 5.0 above upper bound 4.0'),
    (dict(learnField={'diff': True}, fieldBounds={'diff': [(1.0, None), None]}), r"fieldBounds\['diff'\]\[0\] = .* excludes the initial guess 0.5"),
    (dict(learnField={'vel': True}, fieldBounds={'vel': (0.0, None)}), r"fieldBounds\['vel'\]\[1\] = .* excludes the initial guess -1.0"),
    (dict(learnField={'vel': [1, 0, 0]}, fieldBounds={'vel': [None, (-2, 1), None]}), 'bounds an amplitude that learnField does not select'),
])
def test_malformed_options_name_the_field(kw, msg):
    with pytest.raises(ValueError, match=msg):
        make(**kw)


def test_refusals():
    with pytest.raises(ValueError, match=r"learnField\['diff'\]: the PDE has no diff basis"):
        make(pde(velBasis=OMEGA), learnField={'diff': True})
    with pytest.raises(ValueError, match=r"fieldBounds\['vel'\]: the PDE has no vel basis"):
        make(pde(diffBasis=CHI), learnField={'diff': True}, fieldBounds={'vel': (0, 1)})
    with pytest.raises(ValueError, match='^learnField selects no amplitude$'):      # (a PDE without bases: nothing to select from)
        VarNet.fieldLearnData(pde(), {'diff': False})
    with pytest.raises(ValueError, match='learnField needs observations=.*every amplitude admits a solution'):
        make(obs=None, learnField={'diff': True})
    for opt in ('lbfgs', 'rmsprop', 'rms'):
        with pytest.raises(NotImplementedError, match='learnField with optimizer='):
            make(learnField={'diff': True}, optimizer=opt)
    with pytest.raises(NotImplementedError, match='learnField with causal=1.0'):
        make(learnField={'diff': True}, causal=1.0)
    with pytest.raises(NotImplementedError, match='learnField with towers'):
        make(learnField={'diff': True}, processors=['GPU:0', 'GPU:1'])
    with pytest.raises(NotImplementedError, match='velBasis with nldiff is not supported'):
        pde(velBasis=OMEGA, nldiff=[1.0, 0.5])
    make(pde(diffBasis=CHI, nldiff=[1.0, 0.5]), learnField={'diff': True})           # diffBasis with nldiff is allowed
    vn = make(learnField={'diff': True})
    for bad in ({'diff': [1.0]}, {'diff': [1.0, np.nan]}, {'vel': 'abc'}):
        with pytest.raises(ValueError, match=r'setFieldAmplitudes\[.*\] takes \d finite numbers'):
            vn.setFieldAmplitudes(bad)
    for bad in ([1.0, 2.0], {}, {'kappa': [1.0]}):
        with pytest.raises(ValueError, match='setFieldAmplitudes takes a dict'):
            vn.setFieldAmplitudes(bad)


def test_mor_is_refused():
    def diffFun(x, t=0, D=0.01):
        return D * np.ones([len(x), 1])

    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    kw = dict(diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x), MORvar=mor)
    with pytest.raises(NotImplementedError, match='diffBasis with model-order reduction is not supported'):
        ADPDE(Domain1D(), diffBasis=[1.0], **kw)
    with pytest.raises(NotImplementedError, match='velBasis with model-order reduction is not supported'):
        ADPDE(Domain1D(), velBasis=[1.0], **kw)
    with pytest.raises(NotImplementedError, match='learnField with model-order reduction'):
        VarNet(ADPDE(Domain1D(), **kw), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, MORdiscScheme=[3], observations=(X4, C4),
               learnField={'diff': True})


def test_learning_next_to_the_other_learnt_vectors():
    p = pde(reaction=(1.0, [-1.0]), sourceBasis=[lambda x, t: np.sin(pi * x)], **FULL)
    vn = make(p, learnField={'vel': True}, learnCoef={'reaction': [1, 0, 0]}, learnSource=True)
    assert vn.fldLearn is not None and vn.coefLearn is not None and vn.srcLearn is not None
    assert vn.engine.fld_reg['mask'] == [0, 0, 1, 1, 1]


def test_checkpoint_round_trip_of_the_amplitudes():
    vn = make(learnField={'diff': [1, 0], 'vel': True})
    vn.engine.amps = np.array([-1.25, -0.0625, 0.125, 3.0, -4.0])
    arrays = vn.checkpoint_arrays()
    np.testing.assert_array_equal(arrays['field_amplitudes'], vn.engine.amps)
    other = make(learnField={'diff': [1, 0], 'vel': True})
    np.testing.assert_array_equal(other.fieldAmplitudes()['vel'], BV)
    other.restore_arrays(arrays)
    np.testing.assert_array_equal(other.engine.amps, vn.engine.amps)
    assert 'field_amplitudes' not in make().checkpoint_arrays()           # without learnField the checkpoint is what it was


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entry_points():
    import ctypes as C
    from varnet_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    h = r'\s*vn_engine\s*\*\s*h\s*,\s*'
    assert re.search(r'int\s+vn_set_field_basis\s*\(' + h + r'int32_t\s+batch\s*,\s*const\s+float\s*\*\s*G_dev\s*,\s*int32_t\s+J\s*\)\s*;', code)
    assert re.search(r'int\s+vn_set_field_learn\s*\(' + h + r'int32_t\s+J\s*,\s*const\s+int32_t\s*\*\s*mask\s*,\s*const\s+double\s*\*\s*init\s*,'
                     r'\s*const\s+double\s*\*\s*lo\s*,\s*const\s+double\s*\*\s*hi\s*,\s*double\s+lr\s*\)\s*;', code)
    assert re.search(r'int\s+vn_get_field_amps\s*\(' + h + r'double\s*\*\s*amp\s*,\s*double\s*\*\s*grad\s*,\s*int32_t\s+J\s*\)\s*;', code)
    assert re.search(r'int\s+vn_set_field_amps\s*\(' + h + r'const\s+double\s*\*\s*amp\s*,\s*int32_t\s+J\s*\)\s*;', code)
    assert re.search(r'#define\s+VN_FLD_MAX\s+32\b', hdr)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr)            # additive: the version stays
    for name in ('vn_set_field_basis', 'vn_set_field_learn', 'vn_get_field_amps', 'vn_set_field_amps'):
        assert name in engine.ABI_SYMBOLS
    pd = C.POINTER(C.c_double)
    assert engine._SIGS['vn_set_field_basis'] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32])
    assert engine._SIGS['vn_set_field_learn'] == (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), pd, pd, pd, C.c_double])
    assert engine._SIGS['vn_get_field_amps'] == (C.c_int, [C.c_void_p, pd, pd, C.c_int32])
    assert engine._SIGS['vn_set_field_amps'] == (C.c_int, [C.c_void_p, pd, C.c_int32])
    for name in ('set_field_basis', 'set_field_learn', 'get_field_amps', 'set_field_amps'):
        assert callable(getattr(engine.VNEngine, name))
    assert ADPDE.FLD_MAX == 32
