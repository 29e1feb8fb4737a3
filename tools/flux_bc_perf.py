"""Per-step cost of the boundary-flux pass (vn_set_flux_bc, VarNet(fluxBC=True)): the same problem with its flux edges enforced and
without them, vn_train_epoch over the row-wise formulation, HIP-synchronised wall time per step.
    python tools/flux_bc_perf.py [steps]
Problems: a config-1-sized 1D+t run (Operator_1Dt, [20] MLP, 20 x 300 test functions, zero-flux outflow at x = 1) and the full-size
Operator_2Dt problem (BASELINE cfg 3, 5x50 MLP) with its top and bottom walls made zero-flux.  Prints one JSON line per problem."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D, PolygonDomain2D
from varnet_amd.varnet import VarNet

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 400
zero = lambda x, t=0: np.zeros([len(x), 1])     # a callable: constant g values would share one closure


def op1dt(flux):
    pde = ADPDE(Domain1D(), diff=0.1 / np.pi, vel=1.0, tInterval=[0, 2.0], IC=lambda x: -np.sin(np.pi * x),
                BCs=[[], [1.0, 0.0, zero]])
    return VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=300, fluxBC=flux)


def op2dt(flux):
    verts = np.array([[0.0, -0.5], [0.0, -0.2], [0.0, 0.2], [0.0, 0.5], [2.0, 0.5], [2.0, -0.5]])
    BC = [[], [0.0, 1.0, 1.0], [], [1.0, 0.0, zero], [], [1.0, 0.0, zero]]     # edges 3 (top) and 5 (bottom): zero flux
    pde = ADPDE(PolygonDomain2D(verts), diff=1e-3, vel=[1., 0.], tInterval=[0, 1.5], BCs=BC, IC=0.0)
    return VarNet(pde, layerWidth=[50] * 5, discNum=[50, 40], bDiscNum=40, tDiscNum=50, fluxBC=flux)


def step_ms(vn, steps):
    td = vn._build_tdata()
    td.select_mor(0)
    eng = vn.engine
    eng.set_weights([3.0, 2.0, 5.0])
    ids = (0,) * 50
    eng.train_epoch(ids, None)                      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps // len(ids)):
        eng.train_epoch(ids, None)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / (steps // len(ids) * len(ids))


for name, make in (('1D+t Operator_1Dt [20], 6e3 test functions, zero-flux outflow', op1dt),
                   ('2D+t Operator_2Dt 5x50, 1e5 test functions, zero-flux top and bottom walls', op2dt)):
    out = {'problem': name}
    for flux in (False, True, False, True):          # interleaved: a drift of the clock shows as a spread between repeats
        vn = make(flux)
        key = 'flux' if flux else 'plain'
        out.setdefault(key + '_ms', []).append(round(step_ms(vn, STEPS), 4))
        if flux:
            out['flux_rows'] = int(vn.fluxRows['X'].shape[0])
        vn.engine.close()
    out['extra_us_per_step'] = round((min(out['flux_ms']) - min(out['plain_ms'])) * 1e3, 1)
    print(json.dumps(out), flush=True)
