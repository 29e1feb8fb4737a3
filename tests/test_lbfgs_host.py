"""
CPU tier of `VarNet(..., optimizer='lbfgs')`: the host logic (one L-BFGS iteration per epoch, the refusals, the two line-search
outcomes, re-draws, checkpoints across optimizers) on the oracle-backed test engine with the fp64 restatement of the algorithm
(tests/lbfgs_ref.py), and the ABI additions (one enumerator, one macro, one function; the ABI number stays).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.lbfgs_ref import LbfgsOracleEngine
from tests.test_varnet_host import cExact
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

pi = np.pi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return LbfgsOracleEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                                 isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                                 learning_rate=self.learning_rate, optimizer_name=self.optimizer)
    monkeypatch.setattr(VarNet, '_make_engine', make)


def problem(optimizer, layerWidth=[20], discNum=20, tDiscNum=20):
    pde = ADPDE(Domain1D(), diff=0.1 / pi, vel=1.0, timeDependent=True, tInterval=[0, 2.0],
                IC=lambda x: -np.sin(pi * x), cEx=cExact)
    return VarNet(pde, layerWidth=layerWidth, discNum=discNum, bDiscNum=None, tDiscNum=tDiscNum, optimizer=optimizer)


def small(optimizer='lbfgs'):
    return problem(optimizer, layerWidth=[6, 6], discNum=6, tDiscNum=8)


def case_text(tmp_path):
    return open(os.path.join(str(tmp_path), 'caseData.txt')).read()


def test_lbfgs_beats_adam_at_equal_gradient_evaluations(tmp_path):
    """The 1D+t problem of tests/test_varnet_host.py::op1dt at tDiscNum = 20 (6 400 rows), 300 gradient evaluations each from
    the same theta_0 and the same weights: the recorded L-BFGS losses never increase, and the loss L-BFGS has reached is below
    the loss Adam has reached."""
    vn = problem('lbfgs')
    eng = vn.engine
    theta0 = eng.get_params().copy()
    trace = []
    step = eng.lbfgs_step

    def counted(*a, **kw):
        info = step(*a, **kw)
        trace.append((eng.lb.evals, info['f_next']))
        return info
    eng.lbfgs_step = counted
    res = vn.train(str(tmp_path / 'lbfgs'), weight=[10., 10., 1.], epochNum=300, tol=0.0, saveFreq=100, verbose=False)
    losses = np.asarray(res.lossAll, dtype=float)
    assert len(losses) == 300 and np.all(np.diff(losses) <= 0.0)
    np.testing.assert_allclose(losses[0], 1e6, rtol=1e-6)
    assert trace[-1][0] >= 300
    f_lbfgs = [f for n, f in trace if n <= 300][-1]

    va = problem('adam')
    np.testing.assert_array_equal(va.engine.get_params(), theta0)
    va.train(str(tmp_path / 'adam'), weight=[10., 10., 1.], epochNum=300, tol=0.0, saveFreq=100, verbose=False)
    assert va.engine.step == 300
    f_adam = va.engine.eval_loss(0)[0][0]            # at the parameters after 300 steps, under the run's weights
    print('after 300 gradient evaluations: L-BFGS %.4e, Adam %.4e' % (f_lbfgs, f_adam))
    assert f_lbfgs < f_adam
    assert 'L-BFGS quasi-Newton' in case_text(tmp_path / 'lbfgs')


def test_refusals(tmp_path):
    vn = small()
    with pytest.raises(ValueError, match='needs the full batch'):
        vn.train(str(tmp_path), epochNum=2, batchNum=2, verbose=False)
    with pytest.raises(ValueError, match='needs the full batch'):
        vn.train(str(tmp_path), epochNum=2, batchLen=vn.fixData.nt // 2, verbose=False)
    with pytest.raises(ValueError, match='shuffleData=True'):
        vn.train(str(tmp_path), epochNum=2, shuffleData=True, verbose=False)
    vn.world = 2
    with pytest.raises(ValueError, match='runs on one rank'):
        vn.train(str(tmp_path), epochNum=2, verbose=False)
    vn.world = 1
    # the full batch spelled out is no mini-batching
    res = vn.train(str(tmp_path), epochNum=2, batchNum=1, verbose=False)
    assert len(res.lossAll) == 2
    with pytest.raises(ValueError, match='unknown optimizer requested!'):
        small('bfgs')

    def diffFun(x, t=0, D=0.01):
        return D * np.ones([np.shape(x)[0], 1])

    def disc(discNum=3):
        return np.array([0.003 * (11 ** (n / (discNum - 1))) for n in range(discNum)])[np.newaxis].T
    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    pde = ADPDE(Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x),
                MORvar=mor)
    vm = VarNet(pde, layerWidth=[5, 5], discNum=5, bDiscNum=None, tDiscNum=6, MORdiscScheme=disc, optimizer='lbfgs')
    assert vm.fixData.MORbatchNum == 3
    with pytest.raises(ValueError, match='3 MOR batches'):
        vm.train(str(tmp_path), epochNum=2, verbose=False)


def test_status_outcomes_in_the_training_loop(tmp_path):
    """Status 1 (history dropped) is noted in caseData.txt and training goes on; status 2 (stalled) ends train() with its
    sentence, as reaching `tol` does."""
    vn = small()
    eng = vn.engine
    step, n = eng.lbfgs_step, [0]

    def scripted(*a, **kw):
        n[0] += 1
        if n[0] == 4:
            eng.force_status = 1
        if n[0] == 9:
            eng.force_status = 2
        return step(*a, **kw)
    eng.lbfgs_step = scripted
    res = vn.train(str(tmp_path), weight=[10., 10., 1.], epochNum=30, tol=0.0, saveFreq=5, verbose=False)
    assert len(res.lossAll) == 9
    losses = np.asarray(res.lossAll)
    assert np.all(np.diff(losses) <= 0.0)
    txt = case_text(tmp_path)
    assert 'epoch 4: L-BFGS line search found no acceptable step, history dropped' in txt
    assert 'epoch 9: L-BFGS stalled' in txt and 'training ended' in txt
    assert 'Training completed!' not in txt


def test_redraw_restarts_the_optimizer(tmp_path):
    """smpScheme='optimal': the re-draw registers a new batch (and re-initialises the variables), so the iteration after it
    forms its direction from an empty ring at the new objective."""
    np.random.seed(1)
    vn = small()
    eng = vn.engine
    infos = []
    step = eng.lbfgs_step

    def logged(*a, **kw):
        infos.append(step(*a, **kw))
        return infos[-1]
    eng.lbfgs_step = logged
    res = vn.train(str(tmp_path), weight=[10., 10., 1.], smpScheme='optimal', epochNum=12, saveFreq=5, verbose=False,
                   trainUpdelay=5, tolUpd=10.0, frac=0.5, adjustWeight=True)
    assert res.inpIter == [5] and len(infos) == 12
    assert [i['pairs'] for i in infos[:5]] == [0, 1, 2, 3, 4]
    assert infos[5]['pairs'] == 0                                   # the first iteration on the re-drawn set
    assert infos[6]['pairs'] == 1
    assert infos[5]['f_k'] != infos[4]['f_next']                    # another objective, evaluated anew


def test_adam_checkpoint_continues_under_lbfgs_and_back(tmp_path):
    va = small('adam')
    va.train(str(tmp_path / 'adam'), weight=[10., 10., 1.], epochNum=20, tol=0.0, saveFreq=20, verbose=False)
    theta_a = va.engine.get_params().copy()
    vl = small('lbfgs')
    assert vl.loadModel(folderpath=str(tmp_path / 'adam')) == 20
    np.testing.assert_array_equal(vl.engine.get_params(), theta_a)
    assert vl.engine.step == 20
    # the same weights as the Adam run's (train() would re-derive them from the restored loss): continue from its loss
    vl._build_tdata().select_mor(0)
    vl.engine.set_weights(va.trainRes.trainWeight)
    va.engine.set_weights(va.trainRes.trainWeight)
    f_adam = va.engine.eval_loss(0)[0][0]
    info = vl.engine.lbfgs_step(0)
    np.testing.assert_allclose(info['f_k'], f_adam, rtol=1e-6)
    assert info['status'] == 0 and info['f_next'] < f_adam and info['pairs'] == 0
    # ... and an L-BFGS checkpoint (slots written as zeros) restores into an Adam run
    res = vl.train(str(tmp_path / 'lbfgs'), weight=[10., 10., 1.], epochNum=10, tol=0.0, saveFreq=10, verbose=False)
    assert len(res.lossAll) == 10
    z = np.load(os.path.join(str(tmp_path / 'lbfgs'), 'best_model-10.npz'))
    assert not np.any(z['dense_0/kernel/Adam']) and not np.any(z['output/bias/Adam_1'])
    theta_l = vl.engine.get_params().copy()
    vb = small('adam')
    assert vb.loadModel(folderpath=str(tmp_path / 'lbfgs')) == 10
    np.testing.assert_array_equal(vb.engine.get_params(), theta_l)


# ---- ABI: one enumerator, one macro, one function; the number stays ----------------------------------------------------------
def test_header_and_binding_agree_on_the_new_entry_point():
    from varnet_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    names = set(re.findall(r'\b(vn_[a-z0-9_]+)\s*\(', hdr))
    assert 'vn_lbfgs_step' in names and 'vn_lbfgs_step' in engine.ABI_SYMBOLS
    assert names == set(engine.ABI_SYMBOLS)
    assert re.search(r'VN_OPT_LBFGS\s*=\s*2\b', hdr) and re.search(r'#define\s+VN_LBFGS_HISTORY\s+10\b', hdr)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr) and engine.VN_ABI_VERSION == 7
    assert engine.VN_OPT_LBFGS == 2 and engine.VN_LBFGS_HISTORY == 10
    assert engine._SIGS['vn_lbfgs_step'] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double)])


def test_vn_create_accepts_the_new_optimizer_on_a_zeroed_adam_block():
    """optimizer = 2 passes validation with lr, beta1, beta2, eps all zero (L-BFGS ignores them): 0, or 2 (no HIP device)
    where the suite runs without a GPU -- never 1 (VN_EINVAL, 'unknown optimizer requested!')."""
    from varnet_amd import engine
    lib = engine.load_library()
    cfg = engine.VnConfig()
    cfg.dim, cfg.d_in, cfg.n_layers = 1, 2, 1
    cfg.widths[0] = 20
    cfg.integ_num, cfg.time_dependent = 16, 1
    cfg.optimizer = 2
    h = C.c_void_p()
    rc = lib.vn_create(C.byref(cfg), C.byref(h))
    assert rc in (0, 2), (rc, lib.vn_last_error().decode())
    if rc == 0:
        lib.vn_destroy(h)
    else:
        assert 'no HIP device' in lib.vn_last_error().decode()
    cfg.optimizer = 3
    assert lib.vn_create(C.byref(cfg), C.byref(h)) == 1 and 'unknown optimizer' in lib.vn_last_error().decode()
    cfg.optimizer = 0                                 # the zeroed block is still refused for Adam
    assert lib.vn_create(C.byref(cfg), C.byref(h)) == 1
