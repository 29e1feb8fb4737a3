"""Per-step cost of the periodic pass (vn_set_periodic, ADPDE(..., periodic=[(A, B)])): the same problem with an edge pair tied
periodically and with the pair left as (homogeneous Dirichlet) edges, vn_train_epoch over the row-wise formulation, HIP-synchronised
wall time per step.
    python tools/periodic_perf.py [steps]
Problems: a config-1-sized 1D+t run (Operator_1Dt, [20] MLP, 20 x 300 test functions, the two ends paired: 600 periodic rows) and the
full-size 2D+t problem of BASELINE cfg 3 (5x50 MLP) on its bounding rectangle with the left and right walls paired, at the boundary
density of that config (4 000 periodic rows) and at twice that (8 000).  The plain run
keeps the paired edges as Dirichlet rows of the fused kernel's BC/IC tiles, so the difference is the periodic pass minus those rows.
Prints one JSON line per problem."""
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


def op1dt(periodic):
    pde = ADPDE(Domain1D(), diff=0.1 / np.pi, vel=1.0, tInterval=[0, 2.0], IC=lambda x: -np.sin(np.pi * x),
                periodic=[(0, 1)] if periodic else None)
    return VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=300)


def op2dt(periodic, bDiscNum=40):
    verts = np.array([[0.0, -0.5], [0.0, 0.5], [2.0, 0.5], [2.0, -0.5]])      # edges: left, top, right, bottom
    pde = ADPDE(PolygonDomain2D(verts), diff=1e-3, vel=[1., 0.], tInterval=[0, 1.5], IC=0.0,
                periodic=[(0, 2)] if periodic else None)
    return VarNet(pde, layerWidth=[50] * 5, discNum=[50, 40], bDiscNum=bDiscNum, tDiscNum=50)


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


for name, make in (('1D+t Operator_1Dt [20], 6e3 test functions, the two ends paired', op1dt),
                   ('2D+t Operator_2Dt rectangle 5x50, 1e5 test functions, left and right walls paired', op2dt),
                   # the row count of the flux rows' measurement (tools/flux_bc_perf.py): 250 row tiles instead of 125
                   ('the same, boundary density doubled', lambda periodic: op2dt(periodic, 80))):
    out = {'problem': name}
    for periodic in (False, True, False, True):      # interleaved: a drift of the clock shows as a spread between repeats
        vn = make(periodic)
        key = 'periodic' if periodic else 'plain'
        out.setdefault(key + '_ms', []).append(round(step_ms(vn, STEPS), 4))
        if periodic:
            out['periodic_rows'] = int(vn.periodicRows['X'].shape[0])
        else:
            out['dirichlet_rows_plain'] = int(vn.fixData.bDofsum)
        vn.engine.close()
    out['extra_us_per_step'] = round((min(out['periodic_ms']) - min(out['plain_ms'])) * 1e3, 1)
    print(json.dumps(out), flush=True)
