"""Per-step cost of learning the amplitudes of a source basis (vn_set_source_learn, VarNet(..., learnSource=...)): one engine per
problem and J, the same vn_train_epoch steps with learning off and on, interleaved, timed with device events.
    python tools/source_perf.py [steps] [--out DIR] [--small]
Problems: a config-1-sized 1D+t run (Operator_1Dt, [20] MLP, 20 x 300 test functions) and the full-size 2D+t problem of BASELINE
cfg 3 (5x50 MLP), row-wise and on the de-duplicated step, each with a basis of J = 8 and J = 64 Gaussian bumps.  Both carry a
reaction term, so the step runs the two-pass sequence with learning off too and the difference is the two new passes alone (plus
the apply kernel and three launch boundaries).  --small: a tenth of the 2D+t test functions (a quick check of the tool).
Prints one JSON line per variant and writes them to DIR/source_perf.txt (default profiles/).
  `bytes_moved`        what the two passes read and write: the mix (J + 2) nT floats, the reduction (J + ceil(J / 8)) nT floats (the
                       seed stream once per group of eight streams; N_p comes from the integ_num-entry table)
  `bytes_lower_bound`  (J + 2) nT + (J + 1) nT floats
  `TBps_at_least`      bytes_moved over the WHOLE extra time -- a lower bound of the kernels' rate; `fraction_of_hbm`: that over the
                       6.29 TB/s a float4 copy reaches on this GPU; `bound_us`: the time bytes_lower_bound takes at that rate."""
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
SMALL = '--small' in sys.argv
ROUNDS = 3
HBM_TBPS = 6.29


def bumps(J, lo, hi):
    """J Gaussian bumps with seeded centres in the box [lo, hi] (space) and a width of a fifth of its diagonal."""
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    c = np.random.default_rng(7).uniform(lo, hi, (J, lo.size))
    s = 0.2 * np.linalg.norm(hi - lo)
    return [lambda x, t, cj=cj: np.exp(-np.sum((x - cj) ** 2, axis=1, keepdims=True) / (2 * s * s)) for cj in c]


def op1dt(J):
    pde = ADPDE(Domain1D(), diff=0.1 / np.pi, vel=1.0, tInterval=[0, 2.0], IC=lambda x: -np.sin(np.pi * x), reaction=(1.0, [-0.5, 0.1, 0.0]),
                sourceBasis=bumps(J, [-1.0], [1.0]))
    obs = (np.array([[0.0, 0.5], [0.5, 1.0]]), np.zeros(2))
    return VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=300, observations=obs, learnSource=True)


def op2dt(J):
    verts = np.array([[0.0, -0.5], [0.0, 0.5], [2.0, 0.5], [2.0, -0.5]])
    pde = ADPDE(PolygonDomain2D(verts), diff=1e-3, vel=[1., 0.], tInterval=[0, 1.5], IC=0.0, reaction=(1.0, [-0.5, 0.1, 0.0]),
                sourceBasis=bumps(J, [0.0, -0.5], [2.0, 0.5]))
    obs = (np.array([[0.5, 0.0, 0.5], [1.5, 0.2, 1.0]]), np.zeros(2))
    return VarNet(pde, layerWidth=[50] * 5, discNum=[50, 40], bDiscNum=40, tDiscNum=5 if SMALL else 50, observations=obs, learnSource=True)


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
                          ('2D+t Operator_2Dt rectangle 5x50, %s test functions, reaction' % ('1e4' if SMALL else '1e5'), op2dt,
                           ['row-wise', 'de-duplicated'])):
    for J in (8, 64):
        vn = make(J)
        td = vn._build_tdata()
        td.select_mor(0)
        eng = vn.engine
        eng.set_weights([3.0, 2.0, 5.0])
        ids = (0,) * 50
        rows = int(td.mor[0]['Input'].shape[0])
        for form in forms:
            points = 0
            if form == 'de-duplicated':
                points = int(td.enable_dedup())
                if not points:
                    print('de-duplication does not apply: %s' % td.dedup_reason)
                    continue
            out = {'problem': name, 'formulation': form, 'J': J, 'rows': rows, 'unique_points': points, 'off_ms': [], 'learn_ms': []}
            for _ in range(ROUNDS):                     # interleaved: a drift of the clock shows as a spread between repeats
                eng.set_source_learn(None)
                out['off_ms'].append(round(step_ms(eng, ids, STEPS), 4))
                eng.set_source_learn([1] * J, np.zeros(J), lr=1e-6)
                out['learn_ms'].append(round(step_ms(eng, ids, STEPS), 4))
            eng.set_source_learn(None)
            extra = min(out['learn_ms']) - min(out['off_ms'])
            moved = 4.0 * rows * ((J + 2) + (J + (J + 7) // 8))
            bound = 4.0 * rows * ((J + 2) + (J + 1))
            out['extra_us_per_step'] = round(extra * 1e3, 1)
            out['bytes_moved'] = int(moved)
            out['bytes_lower_bound'] = int(bound)
            out['bound_us'] = round(bound / (HBM_TBPS * 1e12) * 1e6, 1)
            if extra > 0:
                out['TBps_at_least'] = round(moved / (extra * 1e-3) / 1e12, 3)
                out['fraction_of_hbm'] = round(out['TBps_at_least'] / HBM_TBPS, 3)
            print(json.dumps(out), flush=True)
            lines.append(json.dumps(out))
        eng.close()
        del vn, td, eng
        torch.cuda.empty_cache()

os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'source_perf.txt'), 'w') as f:
    f.write('tools/source_perf.py %d%s, one MI355X: vn_train_epoch steps, ms per step (device events), with the amplitudes of a J-stream\n'
            'source basis fixed (learning off: the basis is registered and not read) and learnt (all J masked) on the same engine,\n'
            'interleaved (%d rounds each).\n' % (STEPS, ' --small' if SMALL else '', ROUNDS))
    f.write('\n'.join(lines) + '\n')
