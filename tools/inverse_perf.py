"""Per-step cost of learning the PDE coefficients (vn_set_coef_learn, VarNet(..., learnCoef=...)): one engine per problem, the
same vn_train_epoch steps with learning off and on, interleaved, timed with device events.
    python tools/inverse_perf.py [steps] [--out DIR]
Problems: a config-1-sized 1D+t run (Operator_1Dt, [20] MLP, 20 x 300 test functions) with a reaction, and the full-size 2D+t
problem of BASELINE cfg 3 (5x50 MLP) with all three terms, row-wise and on the de-duplicated step.  Prints one JSON line per
variant and writes them to DIR/inverse_perf.txt (default profiles/).  `reduction_TBps_at_least`: the bytes the reduction kernel
reads (4 B x rows x streams row-wise: u, s and one stream per term; 4 B x points x (1 + terms) de-duplicated) over the WHOLE extra
time, which also holds the apply kernel and two launch boundaries -- a lower bound of the kernel's rate; `fraction_of_hbm`: that over
the 6.29 TB/s a float4 copy reaches on this GPU."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D, PolygonDomain2D
from varnet_amd.varnet import VarNet

args = [a for a in sys.argv[1:] if not a.startswith('--')]
STEPS = int(args[0]) if args else 400
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles')
ROUNDS = 3
HBM_TBPS = 6.29


def op1dt():
    pde = ADPDE(Domain1D(), diff=0.1 / np.pi, vel=1.0, tInterval=[0, 2.0], IC=lambda x: -np.sin(np.pi * x), reaction=(1.0, [-0.5, 0.1, 0.0]))
    return VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=300), 1


def op2dt():
    verts = np.array([[0.0, -0.5], [0.0, 0.5], [2.0, 0.5], [2.0, -0.5]])
    pde = ADPDE(PolygonDomain2D(verts), diff=1e-3, vel=[1., 0.], tInterval=[0, 1.5], IC=0.0, reaction=(1.0, [-0.5, 0.1, 0.0]),
                nlflux=([1.0, 0.0], [0.0, 0.5]), nldiff=[1.0, 0.2, 0.0])
    return VarNet(pde, layerWidth=[50] * 5, discNum=[50, 40], bDiscNum=40, tDiscNum=50), 3


def step_ms(eng, ids, steps):
    reps = max(1, steps // len(ids))
    eng.train_epoch(ids, None)                      # warm-up
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        eng.train_epoch(ids, None)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / (reps * len(ids))


lines = []
for name, make, forms in (('1D+t Operator_1Dt [20], 6e3 test functions, reaction', op1dt, ['row-wise']),
                          ('2D+t Operator_2Dt rectangle 5x50, 1e5 test functions, reaction + flux + D(u)', op2dt, ['row-wise', 'de-duplicated'])):
    vn, nterms = make()
    td = vn._build_tdata()
    td.select_mor(0)
    eng = vn.engine
    eng.set_weights([3.0, 2.0, 5.0])
    init = VarNet._pde_coefs(vn.PDE)
    init = init[0] * init[1]
    ids = (0,) * 50
    rows = int(td.mor[0]['Input'].shape[0])
    for form in forms:
        points = 0
        if form == 'de-duplicated':
            points = int(td.enable_dedup())
            if not points:
                print('de-duplication does not apply: %s' % td.dedup_reason)
                continue
        out = {'problem': name, 'formulation': form, 'rows': rows, 'unique_points': points, 'off_ms': [], 'learn_ms': []}
        for _ in range(ROUNDS):                     # interleaved: a drift of the clock shows as a spread between repeats
            eng.set_coef_learn(None)
            out['off_ms'].append(round(step_ms(eng, ids, STEPS), 4))
            eng.set_coef_learn([1] * 9, init, lr=1e-6)
            out['learn_ms'].append(round(step_ms(eng, ids, STEPS), 4))
        eng.set_coef_learn(None)
        extra = min(out['learn_ms']) - min(out['off_ms'])
        nbytes = 4.0 * (points * (1 + nterms) if points else rows * (2 + nterms))
        out['extra_us_per_step'] = round(extra * 1e3, 1)
        out['reduction_bytes'] = int(nbytes)
        if extra > 0:
            out['reduction_TBps_at_least'] = round(nbytes / (extra * 1e-3) / 1e12, 3)
            out['fraction_of_hbm'] = round(out['reduction_TBps_at_least'] / HBM_TBPS, 3)
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))
    eng.close()

os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'inverse_perf.txt'), 'w') as f:
    f.write('tools/inverse_perf.py %d, one MI355X: vn_train_epoch steps, ms per step (device events), with the coefficients fixed and\n'
            'learnt (all nine masked) on the same engine, interleaved (%d rounds each).\n' % (STEPS, ROUNDS))
    f.write('\n'.join(lines) + '\n')
