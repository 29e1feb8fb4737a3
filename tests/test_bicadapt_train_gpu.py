"""
One training pair per rule of the self-adaptive weights on the initial rows (`VarNet(bicAdapt='rba' | 'sa')`, the 'ic' part)
under the project's twin rule: the 1D+t travelling wave of
tests/test_causal_gpu.py::test_causal_run_against_the_plain_run (same network, seed and epochs, restated here) on
[-1, 1] x [0, 1], u = exp(-kappa pi^2 t) sin(pi (x - vel t)) with its Dirichlet data, whose initial profile is the hard part.  The
twin is the same run with no row weights, in the same process.  Required: l2 error against the exact solution
<= 2 twin + 0.01.  Whether the weights IMPROVE on the twin is recorded, not required.

Written to bicadapt_train.json in the directory VN_RECORD_DIR names (default: profile_out/ beside tests/; the committed copy:
profiles/bicadapt_train.json): both errors, their ratio, the final statistics and the correlation of omega_i with l_i at the end.
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
E2E = dict(layerWidth=[20], discNum=20, bDiscNum=None, activationFun='tanh', learning_rate=0.01)     # tests/test_causal_gpu.py
EPOCHS = 10000
KAPPA, T_END, VEL = 0.1, 1.0, 0.5
RECORD = {}
TWIN = {}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'bicadapt_train.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _pde():
    cEx = lambda x, t=0: np.exp(-KAPPA * pi ** 2 * t) * np.sin(pi * (x - VEL * t))
    return ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=KAPPA, vel=VEL, tInterval=[0, T_END], IC=lambda x: cEx(x, 0.0), cEx=cEx,
                 BCs=[[0.0, 1.0, cEx], [0.0, 1.0, cEx]])


def _twin(tmp_path_factory):
    """The plain run, trained once for both rules."""
    if 'err' not in TWIN:
        np.random.seed(0)
        vn = VarNet(_pde(), tDiscNum=10, **E2E)
        vn.train(str(tmp_path_factory.mktemp('twin')), epochNum=EPOCHS, tol=0.0, saveFreq=EPOCHS, verbose=False)
        TWIN['err'] = float(vn.residual()[2])
        vn.engine.close()
    return TWIN['err']


@pytest.mark.parametrize('rule', ['rba', 'sa'])
def test_adaptive_initial_rows_against_the_plain_run(tmp_path, tmp_path_factory, rule):
    twin = _twin(tmp_path_factory)
    np.random.seed(0)
    vn = VarNet(_pde(), tDiscNum=10, bicAdapt={'ic': rule}, **E2E)
    res = vn.train(str(tmp_path / rule), epochNum=EPOCHS, tol=0.0, saveFreq=EPOCHS, verbose=False)
    err = float(vn.residual()[2])
    w = vn.bicRowWeights()['ic']
    vn.engine.close()
    om, l = w['omega'].astype(np.float64), w['l'].astype(np.float64)
    rec = {'adaptive': err, 'twin': twin, 'ratio': err / twin, 'improves': bool(err < twin), 'bar': 2.0 * twin + 0.01, 'stats': w['stats'],
           'rows_ic': int(om.size), 'corr_omega_l': float(np.corrcoef(om, l)[0, 1]) if om.size > 1 and l.std() > 0 and om.std() > 0 else None,
           'epochs': EPOCHS}
    RECORD['twin/travelling_wave/ic/' + rule] = rec
    print('bicadapt travelling wave %s: %s' % (rule, json.dumps(rec, sort_keys=True)))
    assert w['stats']['tau'] == float(EPOCHS) and res.bicAdaptHist[-1][0] == EPOCHS
    assert np.all(np.isfinite(om)) and abs(w['stats']['mean'] - 1.0) <= 1e-12
    assert err <= 2.0 * twin + 0.01, (err, twin)
