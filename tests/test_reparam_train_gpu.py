"""
A trained problem with learnt weight scales (`VarNet(..., reparam=...)`), judged by the twin rule of DESIGN.md sections 14-15.

The problem of tests/test_ansatz_train_gpu.py without the ansatz: 1D+t on [-1, 1] x [0, 1], u* = exp(-t) sin(pi x), diff = 0.1, the
source manufactured from u*, net [20] tanh, the same seed and 10 000 Adam epochs for the three runs:

    twin     the plain network;
    rwf      reparam='rwf' (random weight factorization, s ~ N(1, 0.1));
    slope    reparam={'kind': 'slope', 'n': 10, 'per': 'layer'} (one adaptive slope per hidden layer).

Condition on each reparametrised run: err <= 2 err_twin + 0.01 -- the run must solve the problem, not beat the twin.  The three
errors and the final scales are written to reparam_train.json in the directory VN_RECORD_DIR names (default: profile_out/ beside
tests/; the committed copy: profiles/reparam_train.json).
"""
import json
import os

import numpy as np
import pytest

from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.varnet import VarNet

pytestmark = pytest.mark.gpu

pi = np.pi
E2E = dict(layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=10, activationFun='tanh', learning_rate=0.01)
EPOCHS = 10000
KAPPA = 0.1
RECORD = {}
RUNS = {'rwf': 'rwf', 'slope': {'kind': 'slope', 'n': 10, 'per': 'layer'}}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'reparam_train.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def cEx(x, t=0):
    return np.exp(-t) * np.sin(pi * x)


def source(x, t=0):
    return -cEx(x, t) + KAPPA * pi ** 2 * cEx(x, t)                   # u*_t - kappa u*_xx


def pde():
    return ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=KAPPA, vel=0.0, source=source, tInterval=[0, 1.0], IC=lambda x: cEx(x, 0.0),
                 cEx=cEx, BCs=[[0.0, 1.0, cEx], [0.0, 1.0, cEx]])


def _train(path, **kw):
    """(l2 error, final scales per layer or None)"""
    np.random.seed(0)
    vn = VarNet(pde(), **dict(E2E, **kw))
    try:
        vn.train(str(path), weight=[1.0, 1.0, 1.0], epochNum=EPOCHS, tol=0.0, saveFreq=EPOCHS, verbose=False)
        sc = vn.scales()
        return float(vn.residual()[2]), None if sc is None else [[float(x) for x in a] for a in sc]
    finally:
        vn.engine.close()


@pytest.fixture(scope='module')
def twin(tmp_path_factory):
    return _train(tmp_path_factory.mktemp('twin'))[0]


@pytest.mark.parametrize('name', list(RUNS))
def test_reparametrised_run_solves_the_problem(name, twin, tmp_path):
    """
    Figures of this file's runs are kept in profiles/reparam_train.json and DESIGN.md section 32.
    """
    err, scales = _train(tmp_path / name, reparam=RUNS[name])
    RECORD[name] = {'error': err, 'twin': twin, 'bar': 2.0 * twin + 0.01, 'epochs': EPOCHS, 'scales': scales}
    print('reparam %s: l2 error %.4f, twin %.4f (bar %.4f), %d epochs, final scales %s' % (name, err, twin, 2.0 * twin + 0.01, EPOCHS, scales))
    assert np.isfinite(err) and err <= 2.0 * twin + 0.01, (name, err, twin)
    assert scales is not None and len(scales) == (2 if name == 'rwf' else 1)
    moved = np.concatenate([np.asarray(a) for a in scales])
    assert np.all(np.isfinite(moved)) and np.any(np.abs(moved - 1.0) > 1e-3)          # the scales were trained


def test_checkpoint_round_trip(tmp_path):
    """checkpoint_arrays() carries the joint state when the scales are on, restore_arrays() continues bit for bit, the TF-named
    arrays hold theta_eff, and loading across (on -> off, off -> on, another mode) raises."""
    np.random.seed(0)
    a = VarNet(pde(), reparam='rwf', reparamLr=0.02, **E2E)
    b = VarNet(pde(), reparam='rwf', reparamLr=0.02, **E2E)
    c = VarNet(pde(), **E2E)
    d = VarNet(pde(), reparam={'kind': 'slope', 'n': 2.0}, **E2E)
    try:
        a.train(str(tmp_path / 'a'), epochNum=20, tol=0.0, saveFreq=10 ** 6, verbose=False)
        arr = a.checkpoint_arrays()
        assert {'reparam_mode', 'reparam_V', 'reparam_s', 'reparam_slots'} <= set(arr) and 'reparam_mode' not in c.checkpoint_arrays()
        flat = np.concatenate([np.concatenate([arr['%s/kernel' % n].ravel(), arr['%s/bias' % n].ravel()]) for n in a._var_names()])
        assert np.array_equal(flat, a.engine.get_params()) and not np.array_equal(flat, arr['reparam_V'])
        b.restore_arrays(arr)
        keep = []
        for vn in (a, b):
            np.random.seed(1)
            keep.append(vn._build_tdata())                              # the same training set on both engines
            keep[-1].select_mor(0)
            vn.engine.set_weights([1.0, 1.0, 1.0])
            vn.engine.train_step(0)
            vn.engine.train_step(0)
        assert np.array_equal(np.asarray(a.engine.export_state()), np.asarray(b.engine.export_state()))
        ra, rb = a.engine.get_reparam(), b.engine.get_reparam()
        assert all(np.array_equal(ra[k], rb[k]) for k in ra)
        for other, ck in ((c, arr), (d, arr), (a, c.checkpoint_arrays())):
            with pytest.raises(ValueError, match='reparam'):
                other.restore_arrays(ck)
        case = open(os.path.join(str(tmp_path / 'a'), 'caseData.txt')).read()
        assert 'learnt weight scales' in case
    finally:
        for vn in (a, b, c, d):
            vn.engine.close()
