"""
CPU tier of the per-test-function loss weights and the causal time-slab mode (vn_set_tf_weights, vn_set_causal,
vn_causal_weights, `VarNet(causal=eps)`): the fp64 restatement of tests/causal_ref.py against the underlying references
(weights 1 and eps = 0: bit for bit), the weights of the cases (between 1/4 and 1, a real part of what the GPU tier compares),
the declaration and binding of the three entry points, and the host layer of `VarNet` through a stand-in engine: slab ids on the
uniform, shuffled, mini-batched and MOR sets, the refusals, `setCausal`, and the caseData.txt line.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import causal_ref, nldiff_ref
from tests.causal_cases import (CASES, IDS, LN4, eps_of, n_slabs, ref_kw, reference, reference64, slabs, static_weights, terms_of,
                                theta, weights_are_real)
from tests.oracle_engine import OracleEngine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pi = np.pi
KEYS = ('loss', 'BCloss', 'ICloss', 'varLoss')


# ---- the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['plain', 'terms'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_unit_weights_and_zero_eps_are_the_underlying_reference_exactly(i, variant):
    flat = theta(i).astype(np.float64)
    nldiff, nlflux, reaction = terms_of(i, variant)
    ref, g = nldiff_ref.loss_and_grad(flat, CASES[i][0], CASES[i][2], nldiff, nlflux, reaction, torch.float64, **ref_kw(i))
    for got, gg in (reference64(i, 'none', variant), reference(i, 'static', variant, omega=np.ones(CASES[i][4])),
                    reference(i, 'causal', variant, eps=0.0)):
        for k in KEYS:
            assert got[k] == ref[k], (k, got[k], ref[k])
        assert np.array_equal(got['lossVec'], ref['lossVec'])
        assert np.array_equal(gg, g)
        assert np.array_equal(got['omega'], np.ones(CASES[i][4]))


def test_causal_weights_by_hand():
    lv = np.array([1.0, 3.0, 2.0, 4.0, 10.0])
    slab = np.array([0, 0, 1, 3, 3])                                  # slab 2 is empty: its mean is 0
    om_k, om_s = causal_ref.causal_weights(lv, slab, 5, 0.5)
    C = np.array([0.0, 2.0, 4.0, 4.0, 11.0])
    np.testing.assert_allclose(om_s, np.exp(-0.5 * C), rtol=1e-15)
    np.testing.assert_array_equal(om_k, om_s[slab])
    assert om_s[0] == 1.0
    np.testing.assert_array_equal(causal_ref.causal_weights(lv, slab, 5, 0.0)[1], np.ones(5))


@pytest.mark.parametrize('variant', ['plain', 'terms'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_weights_of_the_cases(i, variant):
    """Between 1/4 and 1 (1/4 exactly on the last slab, 1 on slab 0), unweighted lossVec, and both modes are a real part of the
    compared quantities; the fp32 reference's weights stay within 2e-6 of the fp64 ones."""
    S = n_slabs(i)
    assert S == min(CASES[i][4], 5) and set(slabs(i).tolist()) == set(range(S))
    assert not np.array_equal(slabs(i), np.arange(CASES[i][4]) % S) or CASES[i][4] <= 5     # interleaved
    sw = static_weights(i)
    assert sw.dtype == np.float32 and sw.min() >= 0.2 and sw.max() <= 1.5
    ref, _ = reference64(i, 'causal', variant)
    om = ref['omega_slab']
    assert om[0] == 1.0 and abs(om[-1] - 0.25) <= 1e-12 and np.all(np.diff(om) <= 0.0)
    assert eps_of(i, variant) > 0.0
    assert np.array_equal(ref['lossVec'], reference64(i, 'none', variant)[0]['lossVec'])
    for mode in ('static', 'causal'):
        weights_are_real(i, mode, variant)
    r32, _ = reference(i, 'causal', variant, dtype=torch.float32)
    assert np.max(np.abs(r32['omega_slab'] - om) / om) <= 2e-6


@pytest.mark.parametrize('i', [1, 2], ids=[IDS[1], IDS[2]])
def test_the_gradient_holds_the_weights_constant(i):
    """The causal gradient is the static gradient at the same weights, bit for bit -- not the gradient of the weighted loss as
    a function of theta, which central differences of the loss show to be another vector."""
    ref, g = reference64(i, 'causal')
    ref_s, g_s = reference(i, 'static', omega=ref['omega'])
    assert np.array_equal(g, g_s) and ref['loss'] == ref_s['loss']
    flat = theta(i).astype(np.float64)
    p = int(np.argmax(np.abs(g)))
    e = np.zeros_like(flat)
    e[p] = 1e-5
    fd_frozen = (reference(i, 'static', flat=flat + e, omega=ref['omega'])[0]['loss']
                 - reference(i, 'static', flat=flat - e, omega=ref['omega'])[0]['loss']) / 2e-5
    fd_moving = (reference(i, 'causal', flat=flat + e)[0]['loss'] - reference(i, 'causal', flat=flat - e)[0]['loss']) / 2e-5
    assert abs(fd_frozen - g[p]) <= 1e-4 * abs(g[p])
    assert abs(fd_moving - g[p]) > 1e-2 * abs(g[p])


# ---- ABI --------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound():
    from varnet_amd import engine as vengine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    assert re.search(r'int\s+vn_set_tf_weights\s*\(\s*vn_engine\s*\*\s*h,\s*int32_t\s+batch,\s*const\s+float\s*\*\s*omega_dev\s*\)\s*;', hdr)
    assert re.search(r'int\s+vn_set_causal\s*\(\s*vn_engine\s*\*\s*h,\s*int32_t\s+batch,\s*const\s+int32_t\s*\*\s*slab_dev,'
                     r'\s*int32_t\s+n_slabs,\s*double\s+eps\s*\)\s*;', hdr)
    assert re.search(r'int\s+vn_causal_weights\s*\(\s*vn_engine\s*\*\s*h,\s*int32_t\s+batch,\s*double\s*\*\s*omega_slab_host,'
                     r'\s*int32_t\s+n_slabs\s*\)\s*;', hdr)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr) and vengine.VN_ABI_VERSION == 7
    for name, method in (('vn_set_tf_weights', 'set_tf_weights'), ('vn_set_causal', 'set_causal'),
                         ('vn_causal_weights', 'causal_weights')):
        assert name in vengine.ABI_SYMBOLS
        assert callable(getattr(vengine.VNEngine, method))
        if os.path.exists(vengine.LIB_PATH):                   # (needs the built library)
            assert hasattr(vengine.load_library(), name)


# ---- VarNet host layer through a stand-in engine ----------------------------------------------------------------------
class CausalOracleEngine(OracleEngine):
    """The oracle engine with vn_set_causal / vn_causal_weights: batches with a registration are evaluated by
    tests/causal_ref.py."""

    def set_interior(self, batch, *a, **kw):
        super().set_interior(batch, *a, **kw)
        self.__dict__.setdefault('causal', {}).pop(batch, None)         # vn_set_interior clears the registration

    def set_causal(self, batch, slab=None, n_slabs=None, eps=0.0):
        self.__dict__.setdefault('causal', {})
        if slab is None:
            self.causal.pop(batch, None)
            return
        ids = np.array(slab.numpy() if isinstance(slab, torch.Tensor) else slab).astype(np.int64).reshape(-1)
        assert ids.size == self.batches[batch][3] and ids.min() >= 0 and ids.max() < n_slabs and eps >= 0
        self.causal[batch] = (ids, int(n_slabs), float(eps))

    def _eval(self, batch):
        reg = getattr(self, 'causal', {}).get(batch)
        if reg is None:
            return super()._eval(batch)
        Input, gcoef, src, n_k, detJ, Nr, dNtr = self.batches[batch]
        biInput, biLabel, bDof, biDimVal = self.bic
        if batch in getattr(self, 'bbic', {}):
            biInput, biLabel = self.bbic[batch]
        N, dNt, W = self.fe
        n = Input.shape[0]
        kw = dict(Input=Input, gcoef=gcoef, source=None if not self.isSource else src.reshape(n, 1),
                  N=(np.tile(N, n_k) if Nr is None else Nr).reshape(n, 1), dNt=(np.tile(dNt, n_k) if dNtr is None else dNtr).reshape(n, 1),
                  integW=None if not self.integWflag else W.reshape(1, -1), intShape=[n_k, self.integNum], detJ=detJ,
                  detJvec=np.size(detJ) > 1, biInput=biInput, biLabel=biLabel.reshape(-1, 1), bDof=bDof, biDimVal=biDimVal,
                  w=self.w, dim=self.dim, time_dependent=self.td, is_source=self.isSource, integWflag=self.integWflag)
        return causal_ref.loss_and_grad(self.theta.astype(np.float64), self.inpDim, self.layerWidth, causal=reg, **kw)

    def causal_weights(self, batch=0):
        return self._eval(batch)[0]['omega_slab']


@pytest.fixture
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return CausalOracleEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                                  isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                                  learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


def _pde(**kw):
    return ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, vel=0.5, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x), **kw)


def _slab_from_rows(vn, X, S):
    """Slab ids recomputed from the rows a batch was registered with: the centre of a test function's time nodes."""
    q = vn.fixData.integNum
    t0, T = vn.PDE.tInterval
    h = (T - t0) / S
    tk = X[:, vn.dim].reshape(-1, q).mean(axis=1)
    return np.clip(np.round((tk - t0) / h - 1.0), 0, S - 1).astype(np.int64)


def test_slab_ids_follow_the_test_functions_of_every_batch(cpu_engine):
    vn = VarNet(_pde(), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6, causal=0.5)
    eng = vn.engine
    td = vn._build_tdata()
    ids, S, eps = eng.causal[0]
    assert S == 6 and eps == 0.5
    np.testing.assert_array_equal(ids, np.arange(vn.fixData.nt) % 6)      # space-major, time-minor: k % tDiscNum
    td = vn._build_tdata(batchNum=3)
    for shuffled in (False, True):
        if shuffled:
            np.random.seed(3)
            td.shuffleTrainData()
        seen = []
        for bi in range(td.batchNum):
            ids, S, eps = eng.causal[bi]
            np.testing.assert_array_equal(ids, _slab_from_rows(vn, eng.batches[bi][0], S))
            seen.append(ids)
        seen = np.concatenate(seen)
        assert seen.size == vn.fixData.nt
        np.testing.assert_array_equal(np.bincount(seen, minlength=6), np.full(6, vn.fixData.nt // 6))
        if shuffled:
            assert not np.array_equal(seen, np.arange(vn.fixData.nt) % 6)
    # fewer slabs than time nodes: two nodes per slab
    vn = VarNet(_pde(), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6, causal=0.5, causalSlabs=3)
    vn._build_tdata()
    ids, S, _ = vn.engine.causal[0]
    assert S == 3
    np.testing.assert_array_equal(ids, (np.arange(vn.fixData.nt) % 6) // 2)


def test_slab_ids_are_the_same_for_every_mor_batch(cpu_engine):
    def diffFun(x, t=0, D=0.01):
        return D * np.ones([len(x), 1])

    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    pde = ADPDE(Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x), MORvar=mor)
    vn = VarNet(pde, layerWidth=[5], discNum=6, bDiscNum=None, tDiscNum=4, MORdiscScheme=[3], causal=1.0)
    td = vn._build_tdata()
    assert vn.fixData.MORbatchNum > 1
    for mb in range(vn.fixData.MORbatchNum):
        ids, S, eps = vn.engine.causal[td.engine_batch(mb, 0)]
        assert S == 4 and eps == 1.0
        np.testing.assert_array_equal(ids, np.arange(vn.fixData.nt) % 4)


def test_loss_sees_the_weights_and_set_causal_changes_them(cpu_engine):
    vn = VarNet(_pde(), layerWidth=[6, 4], discNum=8, bDiscNum=None, tDiscNum=6, causal=0.0)
    vn.engine.set_params(vn.engine.get_params() + 0.1)
    td = vn._build_tdata()
    vn.tData = td
    c0, _, lv0 = vn.splitLoss(td)
    np.testing.assert_array_equal(vn.causalWeights(td), np.ones(6))       # eps = 0
    lv = vn.engine.eval_loss(0, lossVec=True)[1].numpy().reshape(-1)
    C5 = np.sum([lv[np.arange(lv.size) % 6 == s].mean() for s in range(5)])
    vn.setCausal(LN4 / C5)                                                 # re-registers on vn.tData
    assert vn.engine.causal[0][2] == LN4 / C5
    om = vn.causalWeights()
    assert om[0] == 1.0 and abs(om[-1] - 0.25) <= 1e-12
    c1, _, _ = vn.splitLoss(td)
    np.testing.assert_array_equal(c0[:2], c1[:2])                          # BC / IC are not weighted
    want = float(np.sum(om[np.arange(lv.size) % 6] * lv))
    assert abs(c1[2, 0] - want) <= 1e-12 * want and c1[2, 0] < 0.9 * c0[2, 0]
    np.testing.assert_array_equal(vn.engine.eval_loss(0, lossVec=True)[1].numpy().reshape(-1), lv)    # lossVec stays unweighted
    vn.setCausal(None)
    assert 0 not in vn.engine.causal
    np.testing.assert_allclose(vn.splitLoss(td)[0], c0, rtol=1e-11)          # (the stand-in's own evaluation: another fp64 route)
    with pytest.raises(ValueError, match='causal mode is off'):
        vn.causalWeights()
    for bad in (-1.0, float('nan'), float('inf'), 'fast', True):
        with pytest.raises(ValueError, match='causal must be a finite float >= 0'):
            vn.setCausal(bad)


def test_refusals(cpu_engine):
    with pytest.raises(ValueError, match='needs a time-dependent PDE'):
        VarNet(ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=1.0, vel=0.0, source=1.0), layerWidth=[5], discNum=8, bDiscNum=None,
               causal=1.0)
    with pytest.raises(ValueError, match='the search direction is not the gradient of the reported loss'):
        VarNet(_pde(), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6, causal=1.0, optimizer='lbfgs')
    for bad in (-0.5, float('nan'), 'on', True):
        with pytest.raises(ValueError, match='causal must be a finite float >= 0'):
            VarNet(_pde(), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6, causal=bad)
    for bad in (0, 4097, 2.5):
        with pytest.raises(ValueError, match='causalSlabs must be an integer'):
            VarNet(_pde(), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6, causal=1.0, causalSlabs=bad)
    with pytest.raises(ValueError, match='causalSlabs is an option of causal'):
        VarNet(_pde(), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6, causalSlabs=3)
    with pytest.raises(NotImplementedError, match='only its shard'):
        VarNet(_pde(), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6, causal=1.0, processors=['GPU:0', 'GPU:1'])
    vn = VarNet(_pde(), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6, optimizer='lbfgs')
    with pytest.raises(ValueError, match='search direction'):
        vn.setCausal(1.0)


def test_towers_kwargs_carry_the_two_arguments():
    import inspect
    src = inspect.getsource(VarNet.__init__)
    assert re.search(r'kw = dict\(.*?causal=causal, causalSlabs=causalSlabs\)', src, re.S)


def _case_lines(path):
    return [ln for ln in open(path).read().splitlines(True) if not ln.startswith('Simulation date')]


def test_case_file_names_the_mode_only_when_on(cpu_engine, tmp_path):
    lines = {}
    for key, kw in (('default', {}), ('none', {'causal': None}), ('on', {'causal': 2.5, 'causalSlabs': 3})):
        np.random.seed(0)
        vn = VarNet(_pde(), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6, **kw)
        vn.train(str(tmp_path / key), epochNum=1, saveFreq=1, verbose=False)
        lines[key] = _case_lines(str(tmp_path / key / 'caseData.txt'))
    assert lines['default'] == lines['none'] and not any('ausal' in ln for ln in lines['default'])
    extra = [ln for ln in lines['on'] if 'ausal' in ln]
    assert extra == ['Causal time-slab loss weights: eps = 2.5, 3 slabs\n']
