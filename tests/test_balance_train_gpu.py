"""
A trained problem with adaptive loss balancing (`VarNet.train(balance=...)`), judged by the twin rule of DESIGN.md sections 14-15.

The problem of tests/test_reparam_train_gpu.py: 1D+t on [-1, 1] x [0, 1], u* = exp(-t) sin(pi x), diff = 0.1, the source manufactured
from u*, net [20] tanh, lr 0.01, weight [1, 1, 1], the same seed and 10 000 Adam epochs for the three runs:

    twin       fixed weights;
    gradnorm   balance={'rule': 'gradnorm', 'freq': 500};
    maxmean    balance={'rule': 'maxmean', 'freq': 500}.

Condition on each balanced run: err <= min(2 err_twin + 0.01, 0.2), and the twin itself <= 0.05 -- the run must solve the problem;
whether it lands above or below the twin on this one seed is a record, not a claim.  The three errors and the weight histories are
written to balance_train.json in the directory VN_RECORD_DIR names (default: profile_out/ beside tests/; the committed copy:
profiles/balance_train.json).  With balancing on, lossLag = 8 and lossLag = 0 must end in the same parameters.
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
FREQ = 500
KAPPA = 0.1
RECORD = {}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'balance_train.json'), 'w') as f:
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


def _train(path, epochs=EPOCHS, **kw):
    """(l2 error, balanceHist, final parameters, step count)"""
    np.random.seed(0)
    vn = VarNet(pde(), **E2E)
    try:
        res = vn.train(str(path), weight=[1.0, 1.0, 1.0], epochNum=epochs, tol=0.0, saveFreq=epochs, verbose=False, **kw)
        return float(vn.residual()[2]), res.balanceHist, vn.engine.get_params().copy(), vn.engine.step
    finally:
        vn.engine.close()


@pytest.fixture(scope='module')
def twin(tmp_path_factory):
    return _train(tmp_path_factory.mktemp('twin'))[0]


@pytest.mark.parametrize('rule', ['gradnorm', 'maxmean'])
def test_balanced_run_solves_the_problem(rule, twin, tmp_path):
    """
    Figures of this file's runs are kept in profiles/balance_train.json and DESIGN.md section 33.
    """
    err, hist, _, steps = _train(tmp_path / rule, balance={'rule': rule, 'freq': FREQ})
    bar = min(2.0 * twin + 0.01, 0.2)
    RECORD[rule] = {'error': err, 'twin': twin, 'bar': bar, 'epochs': EPOCHS, 'freq': FREQ,
                    'weights': [[e] + [float(x) for x in w] for e, w, _, _, _ in hist],
                    'norms': [[e] + [float(x) for x in n] for e, _, n, _, _ in hist],
                    'cos_bc_var': [float(c[0, 2]) for _, _, _, c, _ in hist], 'skipped': [bool(s) for _, _, _, _, s in hist]}
    print('balance %s: l2 error %.4f, twin %.4f (bar %.4f), %d epochs, final weights %s' % (rule, err, twin, bar, EPOCHS, hist[-1][1]))
    assert twin <= 0.05, twin
    assert np.isfinite(err) and err <= bar, (rule, err, twin)
    assert steps == EPOCHS
    assert [h[0] for h in hist] == list(range(1, EPOCHS + 1, FREQ)) and not any(h[4] for h in hist)
    w = np.array([h[1] for h in hist])
    assert np.all(np.isfinite(w)) and np.all(w[:, :3] > 0.0) and np.all(w[:, 3] == 0.0)
    assert not np.array_equal(w[0], w[-1])                                 # the weights moved


@pytest.mark.parametrize('rule', ['gradnorm', 'maxmean'])
def test_loss_lag_is_only_a_readback_schedule_with_balance(rule, tmp_path):
    runs = [_train(tmp_path / ('lag%d' % lag), epochs=700, lossLag=lag, balance={'rule': rule, 'freq': 250}) for lag in (0, 8)]
    (e0, h0, p0, s0), (e8, h8, p8, s8) = runs
    assert s0 == s8 == 700 and [h[0] for h in h0] == [h[0] for h in h8] == [1, 251, 501]
    assert np.array_equal(p0.view(np.uint32), p8.view(np.uint32))
    for a, b in zip(h0, h8):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
