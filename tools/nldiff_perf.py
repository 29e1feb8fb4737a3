"""Cost of the solution-dependent diffusivity D(u) (vn_set_nldiff) on the training step.
    python tools/nldiff_perf.py [--out DIR] [--steps N] [--rounds R]
On the headline workload (BASELINE config 3: Operator_2Dt, 5x50 MLP, 6.4 M rows) and on config 1 (3x20 MLP, 96 000 rows, where
extra launches show), ms per gradient step (vn_grad: every kernel of the step and its reduction, no optimizer update, so all
variants see the same parameters) of five variants of the SAME engine and batch:
    row-wise                         the single-launch 8-wave step
    row-wise + D                     the two-pass sequence (forward-only launch, seed kernel, seeded reverse launch) with the two
                                     elementwise kernels of vn_terms.hip around the seed kernel
    row-wise + reaction + flux + D   ... the flux term's pair inside those and the reaction inside the seed kernel
    dedup                            the de-duplicated step
    dedup + D                        ... plus vn_nldiff_source_kernel and vn_nldiff_point_kernel
The variants are interleaved round by round in one process (R rounds of N steps each after a warm-up round), timed with device
events around the N steps; the median over the rounds is reported with the spread.  D = 0.7 + 0.4 u + 0.3 u^2 with a per-row psi
stream ~ N(0, 1) (the batch's gcoef is left as it is: the cost does not depend on its values); the flux and the reaction are those
of tools/nlflux_perf.py.  Written to DIR/nldiff_perf.txt.  A record, not a test: no bar.  Read the figures against
profiles/nlflux_perf.txt."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench

FLUX = (0.6, 0.5, -0.3)
COEF = (1.0, -1.0, 0.5)
DIFF = (0.7, 0.4, 0.3)


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
    phi = torch.as_tensor(np.random.default_rng(14).standard_normal(n_int).astype(np.float32), device=eng.device)
    psi = torch.as_tensor(np.random.default_rng(15).standard_normal(n_int).astype(np.float32), device=eng.device)
    rate = torch.as_tensor(np.random.default_rng(12).uniform(0.5, 2.0, n_int).astype(np.float32), device=eng.device)
    #           label                              dedup  reaction+flux D
    variants = [('row-wise', False, False, False), ('row-wise + D', False, False, True),
                ('row-wise + reaction + flux + D', False, True, True), ('dedup', True, False, False), ('dedup + D', True, False, True)]
    can_dedup = td.dedup_applies() is None
    times = {v[0]: [] for v in variants}
    for r in range(rounds + 1):                       # round 0: warm-up (allocations, first launches)
        for label, dd, rf, nd in variants:
            if dd and not can_dedup:
                continue
            if dd:
                td.enable_dedup()
            else:
                td.disable_dedup()
            eng.set_reaction(b, rate if rf else None, COEF if rf else None)
            eng.set_nlflux(b, phi if rf else None, FLUX if rf else None)
            eng.set_nldiff(b, psi if nd else None, DIFF if nd else None)
            t = timed(eng, b, steps)
            if r:
                times[label].append(t)
    td.disable_dedup()
    eng.set_reaction(b)
    eng.set_nlflux(b)
    eng.set_nldiff(b)
    kp = eng.kernel_path()
    out = {'problem': name, 'rows_interior': n_int, 'parameters': int(eng.P), 'steps_per_round': steps, 'rounds': rounds,
           'kernel_path': list(kp), 'unique_points': int(sum(v[0].shape[0] for v in getattr(td, '_dd_cache', {}).values()))}
    for label, ts in times.items():
        if ts:
            a = np.array(ts)
            out[label] = {'ms_median': round(float(np.median(a)), 4), 'ms_min': round(float(a.min()), 4),
                          'ms_max': round(float(a.max()), 4)}
    if 'row-wise + D' in out and 'row-wise' in out:
        out['row-wise ratio'] = round(out['row-wise + D']['ms_median'] / out['row-wise']['ms_median'], 4)
    if 'dedup + D' in out and 'dedup' in out:
        out['dedup ratio'] = round(out['dedup + D']['ms_median'] / out['dedup']['ms_median'], 4)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/nldiff_perf.py measures on the GPU: none found')
    os.makedirs(args.out, exist_ok=True)
    lines = ['vn_set_nldiff: ms per gradient step (vn_grad; device events around %d steps, %d interleaved rounds after a warm-up '
             'round, median [min, max]) -- python tools/nldiff_perf.py' % (args.steps, args.rounds),
             'expectation: row-wise + D = the two-pass sequence (profiles/nlflux_perf.txt: row-wise + flux) with two elementwise '
             'kernels that also write a row array each; dedup + D = the plain dedup step plus two small kernels', '']
    for cfg in (3, 1):
        res = perf(cfg, args.steps, args.rounds)
        lines.append('config %d: %s' % (cfg, json.dumps(res)))
        print(lines[-1], flush=True)
        with open(os.path.join(args.out, 'nldiff_perf.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
