"""Per-step cost of regularising a learnt vector (vn_set_learnt_prior, VarNet(..., learntPrior=...)): the same vn_train_epoch steps
on one engine without a prior, with a dense quadratic prior, and with the quadratic prior plus L1 weights, interleaved, timed with
device events; and the time of one vn_get_learnt_prior call (launch, synchronise, copy) on the host clock.
    python tools/prior_perf.py [steps] [--out DIR]
Problem: the config-1-sized 1D+t run of tools/fbc_perf.py (Operator_1Dt, [20] MLP, 20 x 300 test functions, a Neumann end: 300 flux
rows) with the flux-row amplitudes learnt at J = 9 and J = 64, the cap.  The prior adds no launch: what a step pays is the apply
kernel's one block reading J^2 doubles of R (648 B at J = 9, 32 KiB at J = 64) and J fused multiply-adds per thread.  Prints one JSON
line per J and writes them to DIR/prior_perf.txt (default profiles/)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.varnet import VarNet

args = [a for a in sys.argv[1:] if not a.startswith('--')]
STEPS = int(args[0]) if args else 400
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles')
ROUNDS = 3


def bumps(J, t_end):
    c = np.random.default_rng(7).uniform(0.0, t_end, J)
    s = 0.2 * t_end
    return [(1, lambda x, t, cj=cj: np.exp(-(t - cj) ** 2 / (2 * s * s))) for cj in c]


def op1dt(J):
    zero = lambda x, t: 0.0 * t
    pde = ADPDE(Domain1D(), diff=0.1 / np.pi, vel=1.0, tInterval=[0, 2.0], IC=lambda x: -np.sin(np.pi * x), BCs=[[], [1.0, 0.0, zero]],
                fluxBasis=bumps(J // 2, 2.0), robinBasis=bumps(J - J // 2, 2.0))
    obs = (np.array([[0.0, 0.5], [0.5, 1.0]]), np.zeros(2))
    return VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=300, observations=obs, fluxBC=True,
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
for J in (9, 64):
    vn = op1dt(J)
    td = vn._build_tdata()
    td.select_mor(0)
    eng = vn.engine
    eng.set_weights([3.0, 2.0, 5.0])
    ids = (0,) * 50
    rng = np.random.default_rng(J)
    A = rng.standard_normal((J, J))
    R = A @ A.T / J
    R = 0.5 * (R + R.T)
    mean = rng.standard_normal(J)
    variants = {'off_ms': lambda: eng.set_learnt_prior('fluxbc', 0.0),
                'quadratic_ms': lambda: eng.set_learnt_prior('fluxbc', 1e-3, R, mean),
                'quadratic_l1_ms': lambda: eng.set_learnt_prior('fluxbc', 1e-3, R, mean, np.full(J, 1e-3))}
    out = {'problem': '1D+t Operator_1Dt [20], 6e3 test functions', 'J': J, 'rows': int(td.mor[0]['Input'].shape[0]),
           'flux_rows': int(vn.fluxRows['X'].shape[0]), 'matrix_bytes': 8 * J * J}
    out.update({k: [] for k in variants})
    eng.set_fluxbc_learn([1] * J, np.zeros(J), lr=1e-6)
    for _ in range(ROUNDS):                         # interleaved: a drift of the clock shows as a spread between repeats
        for k, register in variants.items():
            register()
            out[k].append(round(step_ms(eng, ids, STEPS), 4))
    base = min(out['off_ms'])
    out['quadratic_extra_us_per_step'] = round((min(out['quadratic_ms']) - base) * 1e3, 2)
    out['quadratic_l1_extra_us_per_step'] = round((min(out['quadratic_l1_ms']) - base) * 1e3, 2)
    out['spread_us'] = round((max(out['off_ms']) - base) * 1e3, 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        eng.learnt_prior('fluxbc')
    out['get_prior_us_per_call'] = round((time.perf_counter() - t0) / 200 * 1e6, 1)
    counts = []
    for k in ('off_ms', 'quadratic_l1_ms'):             # the launches vn_profile_begin / _end count in one step, without and with
        variants[k]()
        eng.profile_begin()
        eng.train_step(0)
        counts.append(int(eng.profile_end()[1]))
    out['profiled_launches_per_step'] = {'off': counts[0], 'prior': counts[1]}
    print(json.dumps(out), flush=True)
    lines.append(json.dumps(out))
    eng.close()
    del vn, td, eng
    torch.cuda.empty_cache()

os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'prior_perf.txt'), 'w') as f:
    f.write('tools/prior_perf.py %d, one MI355X: vn_train_epoch steps, ms per step (device events), with J learnt flux-row amplitudes on one\n'
            'engine: no prior, a dense quadratic prior, the quadratic prior plus L1 weights, interleaved (%d rounds each); and one\n'
            'vn_get_learnt_prior call on the host clock.\n' % (STEPS, ROUNDS))
    f.write('\n'.join(lines) + '\n')
