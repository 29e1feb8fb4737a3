"""Per-step cost of learning the amplitudes of a diffusivity and a velocity basis (vn_set_field_learn, VarNet(..., learnField=...)):
one engine per problem and J, the same vn_train_epoch steps with learning off and on, interleaved, timed with device events.
    python tools/field_perf.py [steps] [--out DIR] [--small]
Problems: a config-1-sized 1D+t run (Operator_1Dt, [20] MLP, 20 x 300 test functions) and the full-size 2D+t problem of BASELINE
cfg 3 (5x50 MLP), row-wise and on the de-duplicated step, each with J = 2 (one bump per basis) and J = 32 (sixteen per basis).
Both carry a reaction term, so the step runs the two-pass sequence with learning off too and the difference is the new work
alone: the mix, on the de-duplicated step the permutation of the mixed gcoef, the reduction, the apply kernel, and on the row-wise
step the extra point pass over the batch's rows.  --small: a tenth of the 2D+t test functions (a quick check of the tool).
Prints one JSON line per variant and writes them to DIR/field_perf.txt (default profiles/).
  `point_pass_us`      (row-wise) vn_forward_grad over the batch's own rows, timed on its own: the pass the step adds for grad u_r
                       (it writes u and grad u apart where the step writes one 16-byte record per row: the same network work)
  `mix_reduce_us`      extra_us_per_step - point_pass_us: the mix, the reduction and the apply kernel (de-duplicated: the whole
                       extra, permutation included)
  `bytes_moved`        what the mix and the reduction read and write, in floats: the mix (J + 2) nT dim, the reduction
                       J nT dim + ceil(J / 8) 5 nT (seed and (u, grad u) record once per group of eight streams); de-duplicated: also
                       the permutation, 2 nT dim + nT, and the row -> point map in the reduction, ceil(J / 8) nT
  `TBps_at_least`      bytes_moved over mix_reduce_us -- a lower bound of those kernels' rate; `fraction_of_hbm`: that over the
                       6.29 TB/s a float4 copy reaches on this GPU."""
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


def bumps(J, lo, hi, ncol):
    """J Gaussian bumps with seeded centres in the box [lo, hi] (space) and a width of a fifth of its diagonal, [n, ncol] each."""
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    c = np.random.default_rng(7 + ncol).uniform(lo, hi, (J, lo.size))
    s = 0.2 * np.linalg.norm(hi - lo)
    return [lambda x, t, cj=cj: np.exp(-np.sum((x - cj) ** 2, axis=1, keepdims=True) / (2 * s * s)) * np.ones((1, ncol)) for cj in c]


def op1dt(J):
    pde = ADPDE(Domain1D(), diff=0.1 / np.pi, vel=1.0, tInterval=[0, 2.0], IC=lambda x: -np.sin(np.pi * x), reaction=(1.0, [-0.5, 0.1, 0.0]),
                diffBasis=bumps(J // 2, [-1.0], [1.0], 1), velBasis=bumps(J // 2, [-1.0], [1.0], 1))
    obs = (np.array([[0.0, 0.5], [0.5, 1.0]]), np.zeros(2))
    return VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=300, observations=obs, learnField={'diff': True, 'vel': True})


def op2dt(J):
    verts = np.array([[0.0, -0.5], [0.0, 0.5], [2.0, 0.5], [2.0, -0.5]])
    pde = ADPDE(PolygonDomain2D(verts), diff=1e-3, vel=[1., 0.], tInterval=[0, 1.5], IC=0.0, reaction=(1.0, [-0.5, 0.1, 0.0]),
                diffBasis=bumps(J // 2, [0.0, -0.5], [2.0, 0.5], 1), velBasis=bumps(J // 2, [0.0, -0.5], [2.0, 0.5], 2))
    obs = (np.array([[0.5, 0.0, 0.5], [1.5, 0.2, 1.0]]), np.zeros(2))
    return VarNet(pde, layerWidth=[50] * 5, discNum=[50, 40], bDiscNum=40, tDiscNum=5 if SMALL else 50, observations=obs,
                  learnField={'diff': True, 'vel': True})


def timed_ms(fn, reps):
    fn()                                            # warm-up
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def step_ms(eng, ids, steps):
    return timed_ms(lambda: eng.train_epoch(ids, None), max(1, steps // len(ids))) / len(ids)


lines = []
for name, make, forms in (('1D+t Operator_1Dt [20], 6e3 test functions, reaction', op1dt, ['row-wise']),
                          ('2D+t Operator_2Dt rectangle 5x50, %s test functions, reaction' % ('1e4' if SMALL else '1e5'), op2dt,
                           ['row-wise', 'de-duplicated'])):
    for J in (2, 32):
        vn = make(J)
        td = vn._build_tdata()
        td.select_mor(0)
        eng = vn.engine
        eng.set_weights([3.0, 2.0, 5.0])
        ids = (0,) * 50
        X = td.mor[0]['Input']
        rows, dim = int(X.shape[0]), vn.dim
        for form in forms:
            points = 0
            if form == 'de-duplicated':
                points = int(td.enable_dedup())
                if not points:
                    print('de-duplication does not apply: %s' % td.dedup_reason)
                    continue
            out = {'problem': name, 'formulation': form, 'J': J, 'rows': rows, 'dim': dim, 'unique_points': points, 'off_ms': [],
                   'learn_ms': []}
            for _ in range(ROUNDS):                     # interleaved: a drift of the clock shows as a spread between repeats
                eng.set_field_learn(None)
                out['off_ms'].append(round(step_ms(eng, ids, STEPS), 4))
                eng.set_field_learn([1] * J, np.zeros(J), lr=1e-6)
                out['learn_ms'].append(round(step_ms(eng, ids, STEPS), 4))
            eng.set_field_learn(None)
            extra = min(out['learn_ms']) - min(out['off_ms'])
            groups = (J + 7) // 8
            moved = 4.0 * rows * ((J + 2) * dim + J * dim + groups * 5)
            pp = 0.0
            if form == 'row-wise':
                pp = min(timed_ms(lambda: eng.forward_grad(X), 20) for _ in range(ROUNDS))
                out['point_pass_us'] = round(pp * 1e3, 1)
            else:
                moved += 4.0 * rows * (2 * dim + 1 + groups)
            out['extra_us_per_step'] = round(extra * 1e3, 1)
            out['mix_reduce_us'] = round((extra - pp) * 1e3, 1)
            out['bytes_moved'] = int(moved)
            if extra - pp > 0:
                out['TBps_at_least'] = round(moved / ((extra - pp) * 1e-3) / 1e12, 3)
                out['fraction_of_hbm'] = round(out['TBps_at_least'] / HBM_TBPS, 3)
            print(json.dumps(out), flush=True)
            lines.append(json.dumps(out))
        eng.close()
        del vn, td, eng, X
        torch.cuda.empty_cache()

os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'field_perf.txt'), 'w') as f:
    f.write('tools/field_perf.py %d%s, one MI355X: vn_train_epoch steps, ms per step (device events), with the amplitudes of a J-stream\n'
            'field basis fixed (learning off: the basis is registered and not read) and learnt (all J masked) on the same engine,\n'
            'interleaved (%d rounds each); point_pass_us: vn_forward_grad over the same rows, timed on its own.\n'
            % (STEPS, ' --small' if SMALL else '', ROUNDS))
    f.write('\n'.join(lines) + '\n')
