"""
CPU tier of boundary data identification (vn_set_bic_basis, vn_set_bic_learn, `ADPDE(bcBasis=..., bcAmp=..., icBasis=...,
icAmp=...)`, `VarNet(..., learnBic=..., bicLr=..., bicBounds=...)`): the reference tests/bic_ref.py against tests/nldiff_ref.py and
against central differences, the input condition of the GPU cases from the CPU numbers alone, the host fold of the amplitudes
without learnBic, the validation of every option, the refusals, the C header, the checkpoint round trip on a stub engine, and
the basis columns on the shuffle path.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import bic_cases as bc
from tests import nldiff_ref
from tests.oracle_engine import OracleEngine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

pi = np.pi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _presummed_loss(i, J, amp=None):
    """nldiff_ref's loss of case i with the labels label0 + B^T a summed beforehand."""
    nldiff, nlflux, reaction = bc.terms_of(i)
    f64 = lambda t: (None if t[0] is None else t[0].astype(np.float64), t[1])
    kw = bc.ref_kw(i)
    kw['biLabel'] = bc.mixed(i, J, amp)[:bc.rows(i)]
    return nldiff_ref.loss_and_grad(bc.theta(i).astype(np.float64), bc.case(i)[0], bc.case(i)[2], f64(nldiff), f64(nlflux), f64(reaction),
                                    torch.float64, **kw)


@pytest.mark.parametrize('i', range(bc.N_CASES), ids=bc.IDS)
def test_reference_restates_nldiff_ref(i):
    """Loss pieces, lossVec and theta-gradient equal tests/nldiff_ref.loss_and_grad with the pre-summed labels to 1e-13; the
    amplitude gradient agrees with central differences of that loss to 1e-6 of S_j (the loss is quadratic in the amplitudes: the
    difference quotient carries rounding only)."""
    J = 3
    res, g, ga, S = bc.reference64(i, J)
    want, gw = _presummed_loss(i, J)
    for k in ('loss', 'BCloss', 'ICloss', 'varLoss'):
        assert abs(res[k] - want[k]) <= 1e-13 * abs(want[k]), (k, res[k], want[k])
    assert np.max(np.abs(res['lossVec'] - want['lossVec'])) <= 1e-13 * np.max(np.abs(want['lossVec']))
    assert np.max(np.abs(g - gw)) <= 1e-13 * np.max(np.abs(gw))
    a0 = bc.basis(i, J)[1]
    for j in range(J):
        h = 1e-3
        ap, am = a0.copy(), a0.copy()
        ap[j] += h
        am[j] -= h
        fd = (_presummed_loss(i, J, ap)[0]['loss'] - _presummed_loss(i, J, am)[0]['loss']) / (2 * h)
        print('%s a%d: g %.6e fd %.6e S %.3e dev/S %.2e' % (bc.IDS[i], j, ga[j], fd, S[j], abs(ga[j] - fd) / S[j]))
        assert abs(ga[j] - fd) <= 1e-6 * S[j], (bc.IDS[i], j, ga[j], fd, S[j])


def test_gpu_cases_condition():
    """From the CPU numbers alone: every component is non-zero, the conditioning floor 0.01 S_j is the binding branch of the bar
    for at most 5 % of all components over all (case, J), and the reference evaluated in fp32 stays within the bar -- a change of
    the cases or of the basis cannot quietly widen it."""
    binding, total, least = [], 0, np.inf
    for i, J in bc.PAIRS:
        _, _, g64, S = bc.reference64(i, J)
        assert np.all(g64 != 0.0) and np.all(S > 0.0), (bc.IDS[i], J)
        total += J
        least = min(least, float(np.min(np.abs(g64) / S)))
        for j in range(J):
            if abs(g64[j]) < bc.COND_FLOOR * S[j]:
                binding.append((bc.IDS[i], J, j, abs(g64[j]) / S[j]))
        g32 = bc.evaluate(i, J, dtype=torch.float32)[2]
        rel = np.abs(g32 - g64) / bc.bars(g64, S)
        print('%s J=%d: fp32 restatement worst err/bar %.3f' % (bc.IDS[i], J, rel.max()))
        assert np.all(rel <= 1.0), (bc.IDS[i], J, rel)
    print('floor binding: %d of %d (least |g64| / S %.4f)' % (len(binding), total, least), binding)
    assert total == 170
    assert len(binding) <= bc.BINDING_FRAC * total, binding


def test_cases_reach_the_row_counts():
    """(nB, bDof) from (2, 2) to (40, 22), steady and time-dependent, nB of 31 and 2 no multiples of 4, bDof = nB on case 5; the
    large-row cases wrap the capped grid, one of them with nB % 4 == 2."""
    nbs = [(bc.case(i)[6], bc.case(i)[7]) for i in range(bc.N_CASES)]
    assert min(nbs) == (2, 2) and max(nbs) == (40, 22)
    assert bc.case(1)[6] == 31 and bc.case(6)[6] == 2 and bc.case(5)[6] == bc.case(5)[7]
    assert {bc.case(i)[10] for i in range(bc.N_CASES)} == {True, False}
    assert [bc.case(bc.N_CASES + k)[6:8] for k in range(2)] == [(65538, 40001), (262152, 131076)]
    assert 65538 > 256 * 256 and 65538 % 4 == 2 and 262152 > 4 * 256 * 256 and 262152 % 4 == 0
    for J in (1, 3, 5, 64):
        B = bc.basis(0, J)[0]
        assert B.shape == (J, 40) and (B.min(axis=1) < 0).any()             # at least one sign-changing stream


# ---- the Python surface on a stub engine -----------------------------------------------------------------------------------------
class BicStubEngine(OracleEngine):
    """The oracle engine plus the registrations the constructor makes: observations, the amplitudes and the bases are only stored."""
    bic_reg = None
    amps = None

    def set_observations(self, *a, **kw):
        pass

    def set_coef_learn(self, *a, **kw):
        pass

    def set_source_learn(self, *a, **kw):
        pass

    def set_field_learn(self, *a, **kw):
        pass

    def set_source_basis(self, *a, **kw):
        pass

    def set_field_basis(self, *a, **kw):
        pass

    def set_bic_learn(self, mask=None, init=None, lo=None, hi=None, lr=None):
        self.bic_reg = None if mask is None else dict(mask=list(mask), lo=np.array(lo), hi=np.array(hi), lr=lr)
        self.amps = None if mask is None else np.asarray(init, dtype=np.float32).astype(np.float64)

    def get_bic_amps(self, grad=False, J=None):
        assert J is None or J == self.amps.size
        return (self.amps.copy(), np.arange(float(self.amps.size))) if grad else self.amps.copy()

    def set_bic_amps(self, amp):
        self.amps = np.asarray(amp, dtype=np.float32).astype(np.float64)

    def set_bic(self, biInput, biLabel, bDof, biDimVal):
        super().set_bic(biInput, biLabel, bDof, biDimVal)
        self.bases = {k: v for k, v in getattr(self, 'bases', {}).items() if k != -1}

    def set_batch_bic(self, batch, biInput=None, biLabel=None):
        super().set_batch_bic(batch, biInput, biLabel)
        getattr(self, 'bases', {}).pop(batch, None)

    def set_bic_basis(self, batch, B=None):
        if not hasattr(self, 'bases'):
            self.bases = {}
        if B is None:
            self.bases.pop(batch, None)
        else:
            self.bases[batch] = B.numpy().copy()


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return BicStubEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                             isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                             learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


X4 = np.array([[0.2, 0.1], [0.4, 0.2], [0.6, 0.3], [0.8, 0.4]])
C4 = np.array([0.1, 0.2, 0.3, 0.4])
GAMMA = [(0, lambda x, t: 1.0 + t), (1, lambda x, t: np.sin(3.0 * t)), (1, lambda x, t: t * t)]
IOTA = [lambda x, j=j: np.sin(j * pi * x) for j in (1, 2)]
G0 = lambda x, t: 0.25 * np.cos(t)
IC0 = lambda x: np.sin(pi * x)


def pde(**kw):
    kw.setdefault('BCs', [[0.0, 2.0, G0], []])
    return ADPDE(Domain1D(np.array([0.0, 1.0])), diff=0.1, vel=0.0, tInterval=[0, 0.5], IC=IC0, **kw)


FULL = dict(bcBasis=GAMMA, bcAmp=[0.5, -1.0, 2.0], icBasis=IOTA, icAmp=[1.5, -0.25])


def make(p=None, obs=(X4, C4), **kw):
    return VarNet(pde(**FULL) if p is None else p, layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, observations=obs, **kw)


def _bic_rows(vn):
    fd = vn.fixData
    _, _, biInput, biDof = vn.trainingPoints('uniform', 0.5, True, 1.0)
    return biInput, biDof


def _want_labels(biInput, biDof, bcAmp, icAmp):
    """label0 + B a restated from the callables: edge 0 has g / beta = G0 / 2, edge 1 the default g = 0."""
    n0, n1 = biDof[0], biDof[0] + biDof[1]
    x, t = biInput[:, :1], biInput[:, 1:2]
    out = np.zeros((biInput.shape[0], 1))
    out[:n0] = G0(x[:n0], t[:n0]) / 2.0 + bcAmp[0] * GAMMA[0][1](x[:n0], t[:n0])
    out[n0:n1] = bcAmp[1] * GAMMA[1][1](x[n0:n1], t[n0:n1]) + bcAmp[2] * GAMMA[2][1](x[n0:n1], t[n0:n1])
    out[n1:] = IC0(x[n1:]) + icAmp[0] * IOTA[0](x[n1:]) + icAmp[1] * IOTA[1](x[n1:])
    return out


def test_amplitudes_fold_into_the_labels_without_learning():
    """Without learnBic the engine sees plain labels: label0 + B a at the constructor's amplitudes; a Dirichlet stream is zero on
    the rows of other indicators and on the initial rows, an initial stream on the boundary rows."""
    vn = make()
    assert vn.bicLearn is None and vn.engine.bic_reg is None
    biInput, biDof = _bic_rows(vn)
    n0, n1 = biDof[0], biDof[0] + biDof[1]
    assert n0 > 0 and n1 > n0 and biInput.shape[0] > n1
    want = _want_labels(biInput, biDof, FULL['bcAmp'], FULL['icAmp'])
    np.testing.assert_allclose(vn.biTrainData(biInput, biDof), want, rtol=0, atol=1e-15)
    np.testing.assert_allclose(vn.biTrainData(biInput, biDof, basis=False), _want_labels(biInput, biDof, [0, 0, 0], [0, 0]), rtol=0, atol=1e-15)
    B = vn._bic_basis(biInput, biDof)
    assert B.shape == (5, biInput.shape[0])
    assert np.all(B[0, n0:] == 0) and np.all(B[1:3, :n0] == 0) and np.all(B[1:3, n1:] == 0) and np.all(B[3:, :n1] == 0)
    assert np.all(B[0, :n0] != 0) and np.any(B[3, n1:] != 0)
    # the labels a training set uploads are the folded ones, and no basis is registered
    tData = vn._build_tdata()
    tData.select_mor(0)
    np.testing.assert_allclose(vn.engine.bic[1].reshape(-1, 1), want, rtol=0, atol=1e-15)
    assert not getattr(vn.engine, 'bases', {})
    got = vn.bicAmplitudes()
    np.testing.assert_array_equal(got['bc'], [0.5, -1.0, 2.0])
    np.testing.assert_array_equal(got['ic'], [1.5, -0.25])
    # amplitudes default to zeros; without a basis nothing changes
    vn0 = make(pde(bcBasis=GAMMA, icBasis=IOTA))
    np.testing.assert_array_equal(vn0.bicAmplitudes()['bc'], np.zeros(3))
    plain = make(pde())
    np.testing.assert_array_equal(vn0.biTrainData(biInput, biDof), plain.biTrainData(biInput, biDof))
    with pytest.raises(ValueError, match='the PDE has no Dirichlet or initial basis'):
        plain.bicAmplitudes()
    for f in (plain.bicGrad, lambda: plain.setBicAmplitudes({'bc': [1.0]})):
        with pytest.raises(ValueError, match='learns no boundary or initial amplitudes'):
            f()


def test_registration_and_accessors():
    vn = make(learnBic={'bc': [True, False, True], 'ic': True}, bicLr=0.05,
              bicBounds={'bc': [(0.0, None), None, (None, 4.0)], 'ic': (-2.0, 2.0)})
    reg = vn.engine.bic_reg
    assert reg['mask'] == [1, 0, 1, 1, 1] and reg['lr'] == 0.05
    assert reg['lo'][0] == 0.0 and reg['hi'][0] == np.inf and reg['lo'][2] == -np.inf and reg['hi'][2] == 4.0
    assert reg['lo'][1] == -np.inf and list(reg['lo'][3:]) == [-2.0, -2.0] and list(reg['hi'][3:]) == [2.0, 2.0]
    np.testing.assert_array_equal(vn.engine.amps, [0.5, -1.0, 2.0, 1.5, -0.25])            # one vector: bc, then ic
    g = vn.bicGrad()
    np.testing.assert_array_equal(g['bc'], [0.0, 1.0, 2.0])
    np.testing.assert_array_equal(g['ic'], [3.0, 4.0])
    vn.setBicAmplitudes({'ic': [1.0, 2.0]})
    np.testing.assert_array_equal(vn.engine.amps, [0.5, -1.0, 2.0, 1.0, 2.0])
    # with learnBic the training set uploads label0 and the [J, nB] streams apart; the host labels follow the current amplitudes
    biInput, biDof = _bic_rows(vn)
    tData = vn._build_tdata()
    tData.select_mor(0)
    np.testing.assert_allclose(vn.engine.bic[1].reshape(-1, 1), _want_labels(biInput, biDof, [0, 0, 0], [0, 0]), rtol=0, atol=1e-15)
    np.testing.assert_allclose(vn.engine.bases[-1], vn._bic_basis(biInput, biDof), rtol=0, atol=1e-15)
    np.testing.assert_allclose(vn.biTrainData(biInput, biDof), _want_labels(biInput, biDof, [0.5, -1.0, 2.0], [1.0, 2.0]), rtol=0, atol=1e-15)
    # a key left out: none of that basis is learnt; bicLr defaults to the network's learning rate
    vn = make(learnBic={'ic': True}, learning_rate=0.01)
    assert vn.engine.bic_reg['mask'] == [0, 0, 0, 1, 1] and vn.engine.bic_reg['lr'] == 0.01
    vn = make(pde(icBasis=IOTA), learnBic={'ic': [0, 1]})
    assert vn.engine.bic_reg['mask'] == [0, 1]


def test_basis_columns_follow_the_shuffle():
    """On the shuffle path a batch gets its own permuted BC/IC copy (biPerm): its basis is the same permutation of the columns."""
    vn = make(learnBic={'bc': True, 'ic': True})
    biInput, biDof = _bic_rows(vn)
    B = vn._bic_basis(biInput, biDof)
    tData = vn._build_tdata(batchNum=2)
    np.random.seed(3)
    tData.shuffleTrainData()
    assert sorted(tData.biPerm) == [0, 1]
    for bi in (0, 1):
        perm = tData.biPerm[bi]
        assert not np.array_equal(perm, np.arange(perm.size))
        b = tData.engine_batch(0, bi)
        np.testing.assert_allclose(vn.engine.bases[b], B[:, perm], rtol=0, atol=1e-15)
        np.testing.assert_array_equal(vn.engine.bbic[b][0], biInput[perm])
        np.testing.assert_allclose(vn.engine.bbic[b][1].reshape(-1), _want_labels(biInput, biDof, [0, 0, 0], [0, 0]).reshape(-1)[perm],
                                   rtol=0, atol=1e-15)


@pytest.mark.parametrize('kw, msg', [
    (dict(bcBasis=[(0, 3.0)]), r'bcBasis\[0\]: gamma must be callable'),
    (dict(bcBasis=[np.sin]), r'bcBasis\[0\] must be a pair \(bInd, gamma\)'),
    (dict(bcBasis=[]), 'bcBasis must be a non-empty list'),
    (dict(bcBasis=[(2, np.sin)]), r'bcBasis\[0\]: boundary indicator 2 outside \[0, 2\)'),
    (dict(bcBasis=[(-1, np.sin)]), r'bcBasis\[0\]: boundary indicator -1 outside'),
    (dict(bcBasis=[(1, np.sin)], BCs=[[], [1.0, 0.0, 0.0]]), r'bcBasis\[0\]: boundary indicator 1 carries a Neumann condition'),
    (dict(bcBasis=[(0, np.sin)], BCs=[[], []], periodic=[(0, 1)]), r'bcBasis\[0\]: boundary indicator 0 is paired by `periodic`'),
    (dict(bcBasis=GAMMA, bcAmp=[1.0, 2.0]), 'bcAmp holds 2 values for the 3 functions of bcBasis'),
    (dict(bcBasis=GAMMA, bcAmp=[1.0, np.inf, 0.0]), 'bcAmp must be finite'),
    (dict(bcBasis=GAMMA, bcAmp='abc'), 'bcAmp must be a list of 3 numbers'),
    (dict(bcAmp=[1.0]), 'bcAmp is an option of bcBasis'),
    (dict(icBasis=[np.sin, 3.0]), r'icBasis\[1\] must be callable'),
    (dict(icBasis=np.sin), 'icBasis must be a non-empty list'),
    (dict(icBasis=IOTA, icAmp=[1.0]), 'icAmp holds 1 values for the 2 functions of icBasis'),
    (dict(icBasis=IOTA, icAmp=[np.nan, 0.0]), 'icAmp must be finite'),
    (dict(icAmp=[1.0]), 'icAmp is an option of icBasis'),
    (dict(bcBasis=GAMMA * 22), 'bcBasis holds 66 functions, at most 64'),
    (dict(bcBasis=GAMMA * 11, icBasis=IOTA * 16), 'bcBasis and icBasis hold 65 functions together, at most 64'),
])
def test_malformed_pde_arguments_name_the_field(kw, msg):
    with pytest.raises(ValueError, match=msg):
        pde(**kw)


def test_ic_basis_needs_a_time_dependent_problem():
    with pytest.raises(ValueError, match='icBasis needs a time-dependent problem'):
        ADPDE(Domain1D(np.array([0.0, 1.0])), diff=0.1, vel=0.0, icBasis=IOTA)


@pytest.mark.parametrize('kw, msg', [
    (dict(learnBic=True), 'learnBic must be a dict'),
    (dict(learnBic={'bc': True, 'edge': True}), 'learnBic must be a dict'),
    (dict(learnBic={'bc': [True, False]}), r"learnBic\['bc'\] must be True or a mask of 3 booleans"),
    (dict(learnBic={'ic': [1, 2]}), r"learnBic\['ic'\] must be True or a mask of 2 booleans"),
    (dict(learnBic={'bc': [False] * 3}), 'learnBic selects no amplitude'),
    (dict(bicLr=0.1), 'bicLr=0.1 is an option of learnBic'),
    (dict(bicBounds={'bc': (0, 1)}), 'bicBounds is an option of learnBic'),
    (dict(learnBic={'bc': True}, bicLr=0.0), 'bicLr=0.0 must be a finite number > 0'),
    (dict(learnBic={'bc': True}, bicLr=float('nan')), 'bicLr=nan must be a finite number > 0'),
    (dict(learnBic={'bc': True}, bicBounds=(0, 1)), 'bicBounds must be a dict'),
    (dict(learnBic={'bc': True}, bicBounds={'bc': [(0, 1)]}), r"bicBounds\['bc'\] must be \(lo, hi\) or a list of 3 entries"),
    (dict(learnBic={'bc': True}, bicBounds={'bc': [(5.0, 4.0), None, None]}), 'lower bound 5.0 above upper bound 4.0'),
    (dict(learnBic={'bc': True}, bicBounds={'bc': [(1.0, None), None, None]}), r'excludes the initial guess 0.5'),
    (dict(learnBic={'bc': [1, 0, 0]}, bicBounds={'bc': [None, (-2, 1), None]}), 'bounds an amplitude that learnBic does not select'),
])
def test_malformed_options_name_the_field(kw, msg):
    with pytest.raises(ValueError, match=msg):
        make(**kw)


def test_refusals():
    with pytest.raises(ValueError, match=r"learnBic\['bc'\]: the PDE has no bc basis"):
        make(pde(icBasis=IOTA), learnBic={'bc': True})
    with pytest.raises(ValueError, match=r"learnBic\['ic'\]: the PDE has no ic basis"):
        make(pde(bcBasis=GAMMA), learnBic={'ic': True})
    with pytest.raises(ValueError, match=r"bicBounds\['ic'\]: the PDE has no ic basis"):
        make(pde(bcBasis=GAMMA), learnBic={'bc': True}, bicBounds={'ic': (0, 1)})
    with pytest.raises(ValueError, match='learnBic needs observations=.*every amplitude admits a solution'):
        make(obs=None, learnBic={'bc': True})
    for opt in ('lbfgs', 'rmsprop', 'rms'):
        with pytest.raises(NotImplementedError, match='learnBic with optimizer='):
            make(learnBic={'bc': True}, optimizer=opt)
    with pytest.raises(NotImplementedError, match='learnBic with causal=1.0'):
        make(learnBic={'bc': True}, causal=1.0)
    with pytest.raises(NotImplementedError, match='learnBic with towers'):
        make(learnBic={'bc': True}, processors=['GPU:0', 'GPU:1'])
    vn = make(learnBic={'bc': True})
    for bad in ({'bc': [1.0, 2.0]}, {'bc': [1.0, np.nan, 0.0]}, {'ic': 'abc'}):
        with pytest.raises(ValueError, match=r'setBicAmplitudes\[.*\] takes \d finite numbers'):
            vn.setBicAmplitudes(bad)
    with pytest.raises(ValueError, match='setBicAmplitudes takes a dict'):
        vn.setBicAmplitudes([1.0, 2.0, 3.0])


def test_mor_is_refused():
    def diffFun(x, t=0, D=0.01):
        return D * np.ones([len(x), 1])

    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    kw = dict(diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x), MORvar=mor)
    with pytest.raises(NotImplementedError, match='bcBasis with model-order reduction is not supported'):
        ADPDE(Domain1D(), bcBasis=[(0, lambda x, t: t)], **kw)
    with pytest.raises(NotImplementedError, match='icBasis with model-order reduction is not supported'):
        ADPDE(Domain1D(), icBasis=IOTA, **kw)
    with pytest.raises(NotImplementedError, match='learnBic with model-order reduction'):
        VarNet(ADPDE(Domain1D(), **kw), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, MORdiscScheme=[3], observations=(X4, C4),
               learnBic={'bc': True})


def test_learning_next_to_the_other_vectors():
    src = [lambda x, t: np.sin(pi * x)]
    vn = make(pde(reaction=(1.0, [-1.0]), sourceBasis=src, diffBasis=[1.0], **FULL), learnBic={'ic': True}, learnSource=True,
              learnField={'diff': True}, learnCoef={'reaction': [1, 0, 0]})
    assert vn.bicLearn is not None and vn.srcLearn is not None and vn.fldLearn is not None and vn.coefLearn is not None
    assert vn.engine.bic_reg['mask'] == [0, 0, 0, 1, 1]
    assert [lv.option for lv in VarNet.LEARNT] == ['learnCoef', 'learnSource', 'learnField', 'learnBic', 'learnFluxBC']


def test_checkpoint_round_trip_of_the_amplitudes():
    vn = make(learnBic={'bc': [1, 0, 1], 'ic': True})
    vn.engine.amps = np.array([-1.25, -1.0, 0.125, 3.0, -0.5])
    arrays = vn.checkpoint_arrays()
    np.testing.assert_array_equal(arrays['bic_amplitudes'], vn.engine.amps)
    other = make(learnBic={'bc': [1, 0, 1], 'ic': True})
    np.testing.assert_array_equal(other.bicAmplitudes()['ic'], [1.5, -0.25])
    other.restore_arrays(arrays)
    np.testing.assert_array_equal(other.engine.amps, vn.engine.amps)
    assert 'bic_amplitudes' not in make().checkpoint_arrays()              # without learnBic the checkpoint is what it was


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entry_points():
    import ctypes as C
    from varnet_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    h = r'\s*vn_engine\s*\*\s*h\s*,\s*'
    assert re.search(r'int\s+vn_set_bic_basis\s*\(' + h + r'int32_t\s+batch\s*,\s*const\s+float\s*\*\s*B_dev\s*,\s*int32_t\s+J\s*\)\s*;', code)
    assert re.search(r'int\s+vn_set_bic_learn\s*\(' + h + r'int32_t\s+J\s*,\s*const\s+int32_t\s*\*\s*mask\s*,\s*const\s+double\s*\*\s*init\s*,'
                     r'\s*const\s+double\s*\*\s*lo\s*,\s*const\s+double\s*\*\s*hi\s*,\s*double\s+lr\s*\)\s*;', code)
    assert re.search(r'int\s+vn_get_bic_amps\s*\(' + h + r'double\s*\*\s*amp\s*,\s*double\s*\*\s*grad\s*,\s*int32_t\s+J\s*\)\s*;', code)
    assert re.search(r'int\s+vn_set_bic_amps\s*\(' + h + r'const\s+double\s*\*\s*amp\s*,\s*int32_t\s+J\s*\)\s*;', code)
    assert re.search(r'#define\s+VN_BIC_MAX\s+64\b', hdr)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr)            # additive: the version stays
    for name in ('vn_set_bic_basis', 'vn_set_bic_learn', 'vn_get_bic_amps', 'vn_set_bic_amps'):
        assert name in engine.ABI_SYMBOLS
    pd = C.POINTER(C.c_double)
    assert engine._SIGS['vn_set_bic_basis'] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32])
    assert engine._SIGS['vn_set_bic_learn'] == (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), pd, pd, pd, C.c_double])
    assert engine._SIGS['vn_get_bic_amps'] == (C.c_int, [C.c_void_p, pd, pd, C.c_int32])
    assert engine._SIGS['vn_set_bic_amps'] == (C.c_int, [C.c_void_p, pd, C.c_int32])
    assert engine.LEARNT['bic'] == ('bic_amps', None)
    for name in ('set_bic_basis', 'set_bic_learn', 'get_bic_amps', 'set_bic_amps'):
        assert callable(getattr(engine.VNEngine, name))
