"""Per-step cost of the observations' pass (vn_set_observations, VarNet(..., observations=...)): one engine per problem, the same
row-wise vn_train_epoch steps without and with a registration, interleaved, timed with device events.
    python tools/obs_perf.py [steps] [--out DIR]
Problems: a config-1-sized 1D+t run (Operator_1Dt, [20] MLP, 20 x 300 test functions) with 600 point sensors, and the full-size
2D+t problem of BASELINE cfg 3 (5x50 MLP) with 4 000 point sensors, with 10^5 point sensors, and with the same 10^5 points as
12 500 averaged sensors of 8 points each.  Prints one JSON line per variant and writes them to DIR/obs_perf.txt (default
profiles/)."""
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


def op1dt():
    pde = ADPDE(Domain1D(), diff=0.1 / np.pi, vel=1.0, tInterval=[0, 2.0], IC=lambda x: -np.sin(np.pi * x))
    return VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=300), ([-1.0], [1.0]), 2.0


def op2dt():
    verts = np.array([[0.0, -0.5], [0.0, 0.5], [2.0, 0.5], [2.0, -0.5]])
    pde = ADPDE(PolygonDomain2D(verts), diff=1e-3, vel=[1., 0.], tInterval=[0, 1.5], IC=0.0)
    return VarNet(pde, layerWidth=[50] * 5, discNum=[50, 40], bDiscNum=40, tDiscNum=50), ([0.0, -0.5], [2.0, 0.5]), 1.5


def observations(rng, box, t_end, n, seg):
    lo, hi = box
    X = np.column_stack([rng.uniform(lo, hi, (n, len(lo))), rng.uniform(0, t_end, n)])
    nO = n // seg
    kw = dict(value=rng.standard_normal(nO))
    if seg > 1:
        kw.update(q=np.full(n, 1.0 / seg), rowptr=seg * np.arange(nO + 1))
    return X, kw


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
for name, make, variants in (('1D+t Operator_1Dt [20], 6e3 test functions', op1dt, [(600, 1)]),
                             ('2D+t Operator_2Dt rectangle 5x50, 1e5 test functions', op2dt, [(4000, 1), (100000, 1), (100000, 8)])):
    vn, box, t_end = make()
    td = vn._build_tdata()
    td.select_mor(0)
    eng = vn.engine
    eng.set_weights([3.0, 2.0, 5.0])
    ids = (0,) * 50
    rng = np.random.default_rng(0)
    for n, seg in variants:
        X, kw = observations(rng, box, t_end, n, seg)
        out = {'problem': name, 'points': n, 'observations': n // seg, 'points_per_observation': seg, 'plain_ms': [], 'obs_ms': []}
        for _ in range(ROUNDS):                     # interleaved: a drift of the clock shows as a spread between repeats
            eng.set_observations(None)
            out['plain_ms'].append(round(step_ms(eng, ids, STEPS), 4))
            eng.set_observations(X, weight=1.0, **kw)
            out['obs_ms'].append(round(step_ms(eng, ids, STEPS), 4))
        out['extra_us_per_step'] = round((min(out['obs_ms']) - min(out['plain_ms'])) * 1e3, 1)
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))
    eng.set_observations(None)
    eng.close()

os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'obs_perf.txt'), 'w') as f:
    f.write('tools/obs_perf.py %d, one MI355X: row-wise vn_train_epoch steps, ms per step (device events), without and with the\n'
            'observations registered on the same engine, interleaved (%d rounds each).\n' % (STEPS, ROUNDS))
    f.write('\n'.join(lines) + '\n')
