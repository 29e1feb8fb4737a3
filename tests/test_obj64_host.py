"""
CPU tier of the fp64 objective (vn_objective_f64): the host logic around it -- VarNet.splitLoss(fp64=True),
VarNet.precisionReport, the refusal on a controller of forked towers -- on an oracle-backed engine, and the agreement of the
header prototype with the ctypes binding.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.oracle_engine import OracleEngine
from varnet_amd import engine as vengine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.varnet import VarNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pi = np.pi


class Oracle64(OracleEngine):
    """OracleEngine with the two calls the device engine gained.  Its plain calls (eval_loss, grad) stand for the fp32 side:
    their results pass through float32; objective64 / eval_loss(fp64=True) return the oracle's doubles.  Every call is
    recorded."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls = []

    def eval_loss(self, batch=0, lossVec=False, **kw):
        self.calls.append(('eval_loss', batch, lossVec, dict(kw)))
        if kw.get('fp64'):
            out, _, lv = self.objective64(batch, grad=False, lossVec=lossVec)
            return out, lv
        out, lv = super().eval_loss(batch, lossVec)
        return [float(np.float32(x)) for x in out], (None if lv is None else lv.to(torch.float32))

    def grad(self, batch=0):
        self.calls.append(('grad', batch))
        super().grad(batch)
        self.gradbuf.copy_(self.gradbuf.to(torch.float32).to(torch.float64))

    def objective64(self, batch=0, theta=None, grad=True, lossVec=False):
        self.calls.append(('objective64', batch, grad, lossVec))
        keep = self.theta
        if theta is not None:
            self.theta = np.asarray(theta, dtype=np.float64)
        try:
            res, g = self._eval(batch)
        finally:
            self.theta = keep
        out = [res['loss'], res['BCloss'], res['ICloss'], res['varLoss']]
        return out, (torch.as_tensor(g) if grad else None), (torch.as_tensor(res['lossVec']).reshape(-1) if lossVec else None)

    def kernel_path(self):
        return 3, False


def _engine(cls):
    def make(self, processors):
        fd = self.fixData
        return cls(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                   isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'], learning_rate=self.learning_rate)
    return make


def _vn(monkeypatch, cls=Oracle64):
    monkeypatch.setattr(VarNet, '_make_engine', _engine(cls))
    pde = ADPDE(Domain1D(), diff=0.1 / pi, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x))
    vn = VarNet(pde, layerWidth=[6, 5], discNum=6, bDiscNum=None, tDiscNum=8)
    vn.engine.init_params(seed=4)
    return vn


def test_splitloss_fp64_sums_the_mini_batches_and_applies_the_weights(monkeypatch):
    vn = _vn(monkeypatch)
    td = vn._build_tdata(batchNum=3)
    assert td.batchNum == 3
    W = np.diag([3.0, 2.0, 5.0])
    eng = vn.engine
    got, _, _ = vn.splitLoss(td, W, fp64=True)
    made = [c for c in eng.calls if c[0] == 'eval_loss']
    assert len(made) == 3 and all(c[3] == {'fp64': True} for c in made)
    td.select_mor(0)
    var, bc, ic = 0.0, None, None
    for bi in range(td.batchNum):
        out, _, _ = eng.objective64(td.engine_batch(0, bi), grad=False)
        bc, ic = out[1], out[2]
        var += out[3]
    np.testing.assert_array_equal(got, np.matmul(W, np.array([[bc, ic, var]]).T))
    # the plain call: the same contract on the fp32 side -- close to, and not the same numbers as, the fp64 one
    plain, _, _ = vn.splitLoss(td, W)
    np.testing.assert_allclose(plain, got, rtol=1e-6)
    assert not np.array_equal(plain, got)
    ident, _, _ = vn.splitLoss(td, fp64=True)
    np.testing.assert_array_equal(ident, np.array([[bc, ic, var]]).T)


def test_splitloss_without_the_flag_makes_the_calls_it_made_before(monkeypatch):
    """On an engine that never heard of fp64 (tests/oracle_engine.OracleEngine: eval_loss(batch, lossVec)), splitLoss() runs
    as before; on the recording engine it passes no fp64 argument and never reaches objective64."""
    vn = _vn(monkeypatch, OracleEngine)
    td = vn._build_tdata(batchNum=2)
    ref, _, _ = vn.splitLoss(td)
    with pytest.raises(TypeError):
        vn.splitLoss(td, fp64=True)                        # that engine has no fp64 form: an error, not an fp32 result
    vn2 = _vn(monkeypatch)
    td2 = vn2._build_tdata(batchNum=2)
    vn2.splitLoss(td2)
    flag = vn2.fixData.lossVecflag
    assert vn2.engine.calls == [('eval_loss', td2.engine_batch(0, bi), flag, {}) for bi in range(2)]
    assert np.all(np.isfinite(ref))


def test_precision_report_fields_and_route(monkeypatch):
    vn = _vn(monkeypatch)
    td = vn._build_tdata(batchNum=2)
    before = vn.engine.theta.copy()
    rep = vn.precisionReport(td)
    assert set(rep) >= {'loss', 'grad_global', 'grad_blocks', 'route', 'kernel', 'two_pass', 'dedup', 'fp32', 'fp64', 'batches'}
    assert rep['route'] == 'fused16 (8-wave)' and rep['kernel'] == 3 and rep['two_pass'] is False and rep['dedup'] is False
    assert rep['batches'] == 2
    assert list(rep['grad_blocks']) == ['W1', 'b1', 'W2', 'b2', 'Wo', 'bo']
    assert set(rep['loss']) == {'loss', 'BCloss', 'ICloss', 'varLoss'}
    # the stand-in's fp32 side is the oracle rounded to float32: deviations of that size, none of them zero across the board
    assert 0.0 < rep['grad_global'] < 1e-6
    assert all(0.0 <= v < 1e-5 for v in rep['grad_blocks'].values())
    assert all(0.0 <= v < 1e-6 for v in rep['loss'].values()) and any(v > 0.0 for v in rep['loss'].values())
    assert np.array_equal(vn.engine.theta, before)
    kinds = [c[0] for c in vn.engine.calls]
    assert kinds.count('grad') == 2 and kinds.count('objective64') == 2 and 'eval_loss' not in kinds
    # without a training set: the set of the last train() call, else a freshly built full-batch one
    assert vn.precisionReport()['batches'] == 1
    # nothing in train() calls it
    import inspect
    assert 'precisionReport' not in inspect.getsource(VarNet.train)


def test_towers_refuse_fp64_and_say_why(monkeypatch):
    vn = _vn(monkeypatch)
    td = vn._build_tdata()
    vn._towers = object()                                  # the controller of forked towers
    try:
        with pytest.raises(NotImplementedError, match='controller of forked towers'):
            vn.splitLoss(td, fp64=True)
        with pytest.raises(NotImplementedError, match='fp32 result is never returned'):
            vn.precisionReport(td)
    finally:
        vn._towers = None


def test_header_prototype_binding_and_symbol_list_agree():
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'int\s+vn_objective_f64\s*\(([^)]*)\)\s*;', code)
    assert m, 'prototype missing'
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 6
    assert args[0].startswith('vn_engine*') and args[1].startswith('int32_t') and args[2].startswith('const double*')
    assert args[3].startswith('double*') and args[4].startswith('double*') and args[5].startswith('double out[4]')
    assert 'vn_objective_f64' in vengine.ABI_SYMBOLS
    res, argt = vengine._SIGS['vn_objective_f64']
    assert res is C.c_int and len(argt) == 6
    assert argt[:5] == [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p] and argt[5] == C.POINTER(C.c_double)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr) and vengine.VN_ABI_VERSION == 7
    if os.path.exists(vengine.LIB_PATH):
        assert hasattr(vengine.load_library(), 'vn_objective_f64')


def test_lbfgs_loss64_is_an_option_of_the_lbfgs_optimizer_only(monkeypatch):
    monkeypatch.setattr(VarNet, '_make_engine', _engine(Oracle64))
    pde = ADPDE(Domain1D(), diff=0.1 / pi, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x))
    with pytest.raises(ValueError, match='lbfgsLoss64'):
        VarNet(pde, layerWidth=[6], discNum=6, bDiscNum=None, tDiscNum=8, lbfgsLoss64=True)          # optimizer='adam'
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'int\s+vn_lbfgs_loss64\s*\(\s*vn_engine\*\s*h\s*,\s*int\s+on\s*\)\s*;', code)
    assert vengine._SIGS['vn_lbfgs_loss64'] == (C.c_int, [C.c_void_p, C.c_int]) and 'vn_lbfgs_loss64' in vengine.ABI_SYMBOLS
