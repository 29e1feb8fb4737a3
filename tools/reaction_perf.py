"""Cost of the polynomial reaction term (vn_set_reaction) on the training step.
    python tools/reaction_perf.py [--out DIR] [--steps N] [--rounds R]
On the headline workload (BASELINE config 3: Operator_2Dt, 5x50 MLP, 6.4 M rows) and on config 1 (3x20 MLP, 96 000 rows, where
extra launches show), ms per gradient step (vn_grad: every kernel of the step and its reduction, no optimizer update, so all
variants see the same parameters) of four variants of the SAME engine and batch:
    row-wise             the single-launch 8-wave step
    row-wise + reaction  the two-pass sequence (forward-only launch, seed kernel, seeded reverse launch: 8 F_pt per row for 6)
    dedup                the de-duplicated step
    dedup + reaction     ... plus vn_react_source_kernel and vn_react_gather_kernel
The variants are interleaved round by round in one process (R rounds of N steps each after a warm-up round), timed with device
events around the N steps; the median over the rounds is reported with the spread.  The reaction is rate * (u - u^2 + 0.5 u^3)
with a per-row rate stream in [0.5, 2].  Written to DIR/reaction_perf.txt.  A record, not a test: no bar."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench

COEF = (1.0, -1.0, 0.5)


def timed(eng, b, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        eng.grad(b)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def perf(cfg, steps, rounds):
    vn, name = bench.build_problem(cfg)
    eng = vn.engine
    td = vn._build_tdata()
    td.select_mor(0)
    b = td.engine_batch(0, 0)
    n_int = int(eng._keep[('int', b)][0].shape[0])
    rate = torch.as_tensor(np.random.default_rng(12).uniform(0.5, 2.0, n_int).astype(np.float32), device=eng.device)
    variants = [('row-wise', False, False), ('row-wise + reaction', False, True), ('dedup', True, False),
                ('dedup + reaction', True, True)]
    can_dedup = td.dedup_applies() is None
    times = {v[0]: [] for v in variants}
    for r in range(rounds + 1):                       # round 0: warm-up (allocations, first launches)
        for label, dd, rx in variants:
            if dd and not can_dedup:
                continue
            if dd:
                td.enable_dedup()
            else:
                td.disable_dedup()
            eng.set_reaction(b, rate if rx else None, COEF if rx else None)
            t = timed(eng, b, steps)
            if r:
                times[label].append(t)
    td.disable_dedup()
    eng.set_reaction(b)
    kp = eng.kernel_path()
    out = {'problem': name, 'rows_interior': n_int, 'parameters': int(eng.P), 'steps_per_round': steps, 'rounds': rounds,
           'kernel_path': list(kp), 'unique_points': int(sum(v[0].shape[0] for v in getattr(td, '_dd_cache', {}).values()))}
    for label, ts in times.items():
        if ts:
            a = np.array(ts)
            out[label] = {'ms_median': round(float(np.median(a)), 4), 'ms_min': round(float(a.min()), 4),
                          'ms_max': round(float(a.max()), 4)}
    if 'row-wise + reaction' in out and 'row-wise' in out:
        out['row-wise ratio'] = round(out['row-wise + reaction']['ms_median'] / out['row-wise']['ms_median'], 4)
    if 'dedup + reaction' in out and 'dedup' in out:
        out['dedup ratio'] = round(out['dedup + reaction']['ms_median'] / out['dedup']['ms_median'], 4)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/reaction_perf.py measures on the GPU: none found')
    os.makedirs(args.out, exist_ok=True)
    lines = ['vn_set_reaction: ms per gradient step (vn_grad; device events around %d steps, %d interleaved rounds after a warm-up '
             'round, median [min, max]) -- python tools/reaction_perf.py' % (args.steps, args.rounds),
             'expectation: row-wise + reaction ~ 8/6 of the plain step plus one seed launch; dedup + reaction = the plain dedup step '
             'plus two small kernels', '']
    for cfg in (3, 1):
        res = perf(cfg, args.steps, args.rounds)
        lines.append('config %d: %s' % (cfg, json.dumps(res)))
        print(lines[-1], flush=True)
        with open(os.path.join(args.out, 'reaction_perf.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
