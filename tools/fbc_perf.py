"""Per-step cost of learning the amplitudes of a flux-datum and a Robin-coefficient basis (vn_set_fluxbc_learn, VarNet(...,
learnFluxBC=...)): one engine per problem and J, the same vn_train_epoch steps with learning off and on, interleaved, timed with
device events.
    python tools/fbc_perf.py [steps] [--out DIR] [--small]
Problems: a config-1-sized 1D+t run (Operator_1Dt, [20] MLP, 20 x 300 test functions, a Neumann end: 300 flux rows) and the
full-size 2D+t problem of BASELINE cfg 3 (5x50 MLP) with its two long edges Neumann (8 000 flux rows), each at J = 8 and J = 64 (half the
streams on the flux datum, half on the Robin coefficient; Gaussian bumps in time), row-wise and on the de-duplicated step.
--small: a tenth of the 2D+t time nodes (a quick check of the tool).  Prints one JSON line per variant and writes them to
DIR/fbc_perf.txt (default profiles/).
  `launches`       what learning adds to a step: two mixes (label, coefficient), the reduction, the apply kernel
  `bytes_moved`    what the mixes and the reduction read and write: (J + 4) nF floats and (J + 2 ceil(J / 8)) nF floats (value and seed
                   once per group of eight streams)
  `bound_us`       the time bytes_moved takes at the 6.29 TB/s a float4 copy reaches on this GPU: nF is small against nT, so the extra
                   time is launches, not bytes"""
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


def bumps(J, edges, t_end):
    """J Gaussian bumps in time with seeded centres in [0, t_end], dealt round the indicators `edges`."""
    c = np.random.default_rng(7).uniform(0.0, t_end, J)
    s = 0.2 * t_end
    return [(edges[j % len(edges)], lambda x, t, cj=cj: np.exp(-(t - cj) ** 2 / (2 * s * s))) for j, cj in enumerate(c)]


def op1dt(J):
    zero = lambda x, t: 0.0 * t
    pde = ADPDE(Domain1D(), diff=0.1 / np.pi, vel=1.0, tInterval=[0, 2.0], IC=lambda x: -np.sin(np.pi * x), BCs=[[], [1.0, 0.0, zero]],
                fluxBasis=bumps(J // 2, [1], 2.0), robinBasis=bumps(J - J // 2, [1], 2.0))
    obs = (np.array([[0.0, 0.5], [0.5, 1.0]]), np.zeros(2))
    return VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=300, observations=obs, fluxBC=True,
                  learnFluxBC={'flux': True, 'robin': True})


def op2dt(J):
    verts = np.array([[0.0, -0.5], [0.0, 0.5], [2.0, 0.5], [2.0, -0.5]])
    zero = lambda x, t: 0.0 * t
    pde = ADPDE(PolygonDomain2D(verts), diff=1e-3, vel=[1., 0.], tInterval=[0, 1.5], IC=0.0, BCs=[[], [1.0, 0.0, zero], [], [1.0, 0.0, zero]],
                fluxBasis=bumps(J // 2, [1, 3], 1.5), robinBasis=bumps(J - J // 2, [1, 3], 1.5))
    obs = (np.array([[0.5, 0.0, 0.5], [1.5, 0.2, 1.0]]), np.zeros(2))
    return VarNet(pde, layerWidth=[50] * 5, discNum=[50, 40], bDiscNum=40, tDiscNum=5 if SMALL else 50, observations=obs, fluxBC=True,
                  learnFluxBC={'flux': True, 'robin': True})


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
for name, make in (('1D+t Operator_1Dt [20], 6e3 test functions', op1dt),
                   ('2D+t Operator_2Dt rectangle 5x50, %s test functions' % ('1e4' if SMALL else '1e5'), op2dt)):
    for J in (8, 64):
        vn = make(J)
        td = vn._build_tdata()
        td.select_mor(0)
        eng = vn.engine
        eng.set_weights([3.0, 2.0, 5.0])
        ids = (0,) * 50
        rows = int(td.mor[0]['Input'].shape[0])
        nF = int(vn.fluxRows['X'].shape[0])
        for form in ('row-wise', 'de-duplicated'):
            points = 0
            if form == 'de-duplicated':
                points = int(td.enable_dedup())
                if not points:
                    print('de-duplication does not apply: %s' % td.dedup_reason)
                    continue
            out = {'problem': name, 'formulation': form, 'J': J, 'rows': rows, 'flux_rows': nF, 'unique_points': points,
                   'kernel_path': list(eng.kernel_path()), 'off_ms': [], 'learn_ms': []}
            for _ in range(ROUNDS):                     # interleaved: a drift of the clock shows as a spread between repeats
                eng.set_fluxbc_learn(None)
                out['off_ms'].append(round(step_ms(eng, ids, STEPS), 4))
                eng.set_fluxbc_learn([1] * J, np.zeros(J), lr=1e-6)
                out['learn_ms'].append(round(step_ms(eng, ids, STEPS), 4))
            eng.set_fluxbc_learn(None)
            extra = min(out['learn_ms']) - min(out['off_ms'])
            moved = 4.0 * nF * ((J + 4) + (J + 2 * ((J + 7) // 8)))
            out['extra_us_per_step'] = round(extra * 1e3, 1)
            out['launches'] = 4
            out['bytes_moved'] = int(moved)
            out['bound_us'] = round(moved / (HBM_TBPS * 1e12) * 1e6, 3)
            print(json.dumps(out), flush=True)
            lines.append(json.dumps(out))
        eng.close()
        del vn, td, eng
        torch.cuda.empty_cache()

os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'fbc_perf.txt'), 'w') as f:
    f.write('tools/fbc_perf.py %d%s, one MI355X: vn_train_epoch steps, ms per step (device events), with the amplitudes of a J-stream\n'
            'flux-datum / Robin-coefficient basis fixed (learning off: the basis is registered and not read) and learnt (all J masked) on\n'
            'the same engine, interleaved (%d rounds each).\n' % (STEPS, ' --small' if SMALL else '', ROUNDS))
    f.write('\n'.join(lines) + '\n')
