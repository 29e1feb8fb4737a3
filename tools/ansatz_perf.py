"""Cost of the hard-constraint ansatz u = A + B n (vn_set_ansatz) on the training step.
    python tools/ansatz_perf.py [--out DIR] [--steps N] [--rounds R]
On the headline workload (BASELINE config 3: Operator_2Dt, 5x50 MLP, 6.4 M rows) and on config 1 (3x20 MLP, 96 000 rows, where
extra launches show), ms per gradient step (vn_grad: every kernel of the step and its reduction, no optimizer update, so all
variants see the same parameters) of five variants of the SAME engine and batch:
    row-wise              the single-launch 8-wave step
    two-pass              the two-pass sequence (forward-only launch, seed kernel, seeded reverse launch) as the engine ran it
                          before: forced by a reaction term of no numerical weight, which lives inside the seed kernel and adds
                          no kernel -- an ansatz batch runs this sequence whatever else it has, so this is its baseline
    row-wise + ansatz     ... with the two elementwise kernels of vn_ansatz.hip around the seed kernel, and the BC/IC rows out
                          of the reverse launch, on the generic kernels (forward, fold, seed, adjoint, reverse)
    dedup                 the de-duplicated step
    dedup + ansatz        ... plus the two point kernels and the same BC/IC passes
The variants are interleaved round by round in one process (R rounds of N steps each after a warm-up round), timed with device
events around the N steps; the median over the rounds is reported with the spread.  Streams: A ~ 0.5 N(0,1), B ~ U(0.3, 1.7),
a, b ~ N(0,1) (the cost does not depend on their values).  Written to DIR/ansatz_perf.txt.  A record, not a test: no bar."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench

NO_WEIGHT = (0.0, 0.0, 1e-30)                         # a registered reaction that changes no bit that matters


def timed(eng, b, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        eng.grad(b)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def streams(rng, n, dim=None, device=None):
    f = lambda a: torch.as_tensor(a.astype(np.float32), device=device)
    shape = (n,) if dim is None else (n, dim)
    return f(0.5 * rng.standard_normal(n)), f(rng.uniform(0.3, 1.7, n)), f(rng.standard_normal(shape)), f(rng.standard_normal(shape))


def perf(cfg, steps, rounds):
    vn, name = bench.build_problem(cfg)
    eng = vn.engine
    td = vn._build_tdata()
    td.select_mor(0)
    b = td.engine_batch(0, 0)
    n_int = int(eng._keep[('int', b)][0].shape[0])
    nB = int(eng._keep['bic'][0].shape[0])
    rng = np.random.default_rng(16)
    rows = streams(rng, n_int, device=eng.device)
    bic = streams(rng, nB, device=eng.device)[:2]
    pts = None
    #           label                 dedup  two-pass ansatz
    variants = [('row-wise', False, False, False), ('two-pass', False, True, False), ('row-wise + ansatz', False, False, True),
                ('dedup', True, False, False), ('dedup + ansatz', True, False, True)]
    can_dedup = td.dedup_applies() is None
    times = {v[0]: [] for v in variants}
    for r in range(rounds + 1):                       # round 0: warm-up (allocations, first launches)
        for label, dd, tp, az in variants:
            if dd and not can_dedup:
                continue
            if dd:
                td.enable_dedup()
            else:
                td.disable_dedup()
            eng.set_reaction(b, None, NO_WEIGHT if tp else None)
            eng.set_ansatz(b, *(rows if az else ()))
            eng.set_ansatz_rows('bic', *(bic if az else ()))
            if dd and az:
                if pts is None:
                    U = int(td._dd_cache[(0, 0)][0].shape[0])
                    pts = streams(rng, U, vn.dim, device=eng.device)
                eng.set_ansatz_points(b, *pts)
            t = timed(eng, b, steps)
            if r:
                times[label].append(t)
    td.disable_dedup()
    eng.set_reaction(b)
    eng.set_ansatz(b)
    eng.set_ansatz_rows('bic')
    kp = eng.kernel_path()
    out = {'problem': name, 'rows_interior': n_int, 'rows_bcic': nB, 'parameters': int(eng.P), 'steps_per_round': steps, 'rounds': rounds,
           'kernel_path': list(kp), 'unique_points': int(sum(v[0].shape[0] for v in getattr(td, '_dd_cache', {}).values()))}
    for label, ts in times.items():
        if ts:
            a = np.array(ts)
            out[label] = {'ms_median': round(float(np.median(a)), 4), 'ms_min': round(float(a.min()), 4),
                          'ms_max': round(float(a.max()), 4)}
    if 'row-wise + ansatz' in out and 'two-pass' in out:
        out['ansatz over two-pass, ms'] = round(out['row-wise + ansatz']['ms_median'] - out['two-pass']['ms_median'], 4)
    if 'dedup + ansatz' in out and 'dedup' in out:
        out['ansatz over dedup, ms'] = round(out['dedup + ansatz']['ms_median'] - out['dedup']['ms_median'], 4)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/ansatz_perf.py measures on the GPU: none found')
    os.makedirs(args.out, exist_ok=True)
    lines = ['vn_set_ansatz: ms per gradient step (vn_grad; device events around %d steps, %d interleaved rounds after a warm-up '
             'round, median [min, max]) -- python tools/ansatz_perf.py' % (args.steps, args.rounds),
             'expectation (unmeasured when written): row-wise + ansatz = two-pass + on the order of 0.1 ms at 6.4 M rows for the two '
             'row kernels (about 56 B per interior row, 360 MB moved) + the BC/IC rows\' generic passes', '']
    for cfg in (3, 1):
        res = perf(cfg, args.steps, args.rounds)
        lines.append('config %d: %s' % (cfg, json.dumps(res)))
        print(lines[-1], flush=True)
        with open(os.path.join(args.out, 'ansatz_perf.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
