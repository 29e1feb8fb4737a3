"""Cost of an L-BFGS iteration (vn_lbfgs_step, VarNet(optimizer='lbfgs')) against the Adam step on the same problem: both
optimizers in ONE process, alternating in blocks after a warm-up, a host clock around work that ends in a device synchronise.
    python tools/lbfgs_perf.py [cfg3|cfg1|converge|all] [iterations]
cfg3: the full-size Operator_2Dt problem (BASELINE config 3: 5x50 MLP, 1e5 test functions, 6.4 M rows, row-wise).
cfg1: the Operator_1Dt size ([20] MLP, 6e3 test functions, 96 000 rows).
converge: cfg1, wall time and gradient evaluations until l2Err(cExact) <= 0.05 for both optimizers (weights [10, 10, 1] scaled
to an initial loss of 1e6 as train() scales them; the error is looked at every 100 L-BFGS iterations / 1 000 Adam steps, its
evaluation is not timed).
An L-BFGS iteration is timed on its own (it ends in a read-back); the figure reported is that of iterations whose first trial
was accepted (one gradient evaluation, like the Adam step).  Prints one JSON line per problem."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D, PolygonDomain2D
from varnet_amd.utility import UF
from varnet_amd.varnet import VarNet

WHAT = sys.argv[1] if len(sys.argv) > 1 else 'all'
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 240
pi = np.pi


def cExact(x, t, trunc=800, u=1.0, D=0.1 / pi):
    """Fourier-series solution of the 1D+t problem (examples/operator_1dt.py)."""
    p = np.arange(0, trunc + 1.0).reshape(1, trunc + 1)
    c0 = 16 * pi ** 2 * D ** 3 * u * np.exp(u / D / 2 * (x - u * t / 2))
    e1 = np.exp(-D * p ** 2 * pi ** 2 * t)
    e2 = np.exp(-D * (2 * p + 1) ** 2 * pi ** 2 * t / 4)
    c1d = u ** 4 + 8 * (u * pi * D) ** 2 * (p ** 2 + 1) + 16 * (pi * D) ** 4 * (p ** 2 - 1) ** 2
    c2d = u ** 4 + (u * pi * D) ** 2 * (8 * p ** 2 + 8 * p + 10) + (pi * D) ** 4 * (4 * p ** 2 + 4 * p - 3) ** 2
    S = np.sinh(u / D / 2) * np.sum((-1) ** p * 2 * p * np.sin(p * pi * x) * e1 / c1d, axis=-1, keepdims=True) + \
        np.cosh(u / D / 2) * np.sum((-1) ** p * (2 * p + 1) * np.cos((p + 0.5) * pi * x) * e2 / c2d, axis=-1, keepdims=True)
    c = c0 * S
    c[t == 0] = -np.sin(pi * x[t == 0])
    return c


def op1dt(optimizer):
    pde = ADPDE(Domain1D(), diff=0.1 / pi, vel=1.0, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x), cEx=cExact)
    return VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=300, optimizer=optimizer)


def op2dt(optimizer):
    verts = np.array([[0.0, -0.5], [0.0, -0.2], [0.0, 0.2], [0.0, 0.5], [2.0, 0.5], [2.0, -0.5]])
    BC = [[], [0.0, 1.0, 1.0], [], [], [], []]
    pde = ADPDE(PolygonDomain2D(verts), diff=1e-3, vel=[1., 0.], tInterval=[0, 1.5], BCs=BC, IC=0.0)
    return VarNet(pde, layerWidth=[50] * 5, discNum=[50, 40], bDiscNum=40, tDiscNum=50, optimizer=optimizer)


def register(vn):
    td = vn._build_tdata()
    td.select_mor(0)
    vn.engine.set_weights([3.0, 2.0, 5.0])
    return td


def step_cost(name, make, block):
    adam, lb = make('adam'), make('lbfgs')
    keep = (register(adam), register(lb))
    ea, el = adam.engine, lb.engine
    ids = (0,) * block
    ea.train_epoch(ids, None)                        # warm-up of both
    for _ in range(block):
        el.lbfgs_step(0)
    torch.cuda.synchronize()
    adam_ms, first, other, trials = [], [], [], 0
    done = 0
    while done < ITERS:
        t0 = time.perf_counter()
        ea.train_epoch(ids, None)
        torch.cuda.synchronize()
        adam_ms.append((time.perf_counter() - t0) * 1e3 / block)
        for _ in range(block):
            t0 = time.perf_counter()
            info = el.lbfgs_step(0)                  # ends in its own read-back and synchronise
            dt = (time.perf_counter() - t0) * 1e3
            if info['status'] == 0:
                trials += info['trials']
                (first if info['trials'] == 1 else other).append(dt)
        done += block
    a = np.array(adam_ms)
    f = np.array(first)
    out = {'problem': name, 'parameters': int(ea.P), 'block': block,
           'adam_ms_per_step': {'median': round(float(np.median(a)), 5), 'min': round(float(a.min()), 5),
                                'max': round(float(a.max()), 5), 'blocks': len(a),
                                'spread_max_over_min': round(float(a.max() / a.min()), 4)},
           'lbfgs_ms_first_trial_accepted': {'median': round(float(np.median(f)), 5), 'mean': round(float(f.mean()), 5),
                                             'min': round(float(f.min()), 5), 'iterations': len(f)},
           'lbfgs_iterations_with_more_trials': len(other),
           'trials_per_accepted_iteration': round(trials / max(1, len(first) + len(other)), 4),
           'lbfgs_over_adam_median': round(float(np.median(f) / np.median(a)), 4)}
    print(json.dumps(out), flush=True)
    ea.close()
    el.close()
    del keep


def converge():
    uf = UF()
    out = {'problem': '1D+t Operator_1Dt [20], 96 000 rows: to l2Err(cExact) <= 0.05', 'bar': 0.05}
    for opt, chunk, cap in (('lbfgs', 100, 20000), ('adam', 1000, 300000)):
        vn = op1dt(opt)
        eng = vn.engine
        vn.train(tempfile.mkdtemp(), weight=[10., 10., 1.], epochNum=1, tol=0.0, saveFreq=10 ** 7, verbose=False)
        wall, evals, its, err, stalled = 0.0, 1, 1, 1.0, False
        while its < cap and err > 0.05 and not stalled:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if opt == 'adam':
                eng.train_epoch((0,) * chunk, None)
                evals += chunk
            else:
                for _ in range(chunk):
                    info = eng.lbfgs_step(0)
                    evals += info['trials']
                    if info['status'] == 2:
                        stalled = True
                        break
            torch.cuda.synchronize()
            wall += time.perf_counter() - t0
            its += chunk
            err = float(uf.l2Err(vn.fixData.cEx, vn.evaluate()))
        out[opt] = {'iterations': its, 'gradient_evaluations': evals, 'wall_s': round(wall, 4), 'l2Err': round(err, 5),
                    'reached': bool(err <= 0.05), 'stalled': stalled}
        eng.close()
    print(json.dumps(out), flush=True)


if WHAT in ('cfg3', 'all'):
    step_cost('2D+t Operator_2Dt 5x50, 1e5 test functions, 6.4 M rows, row-wise', op2dt, 10)
if WHAT in ('cfg1', 'all'):
    step_cost('1D+t Operator_1Dt [20], 6e3 test functions, 96 000 rows', op1dt, 50)
if WHAT in ('converge', 'all'):
    converge()
