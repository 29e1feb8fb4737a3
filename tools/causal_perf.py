"""Cost of per-test-function loss weights (vn_set_tf_weights) and of the causal time-slab mode (vn_set_causal) on the training step.
    python tools/causal_perf.py [--out DIR] [--steps N] [--rounds R]
On the headline workload (BASELINE config 3: Operator_2Dt, 5x50 MLP, 6.4 M rows) and on config 1 (3x20 MLP, 96 000 rows, where
extra launches show), ms per gradient step (vn_grad: every kernel of the step and its reduction, no optimizer update, so all
variants see the same parameters) of five variants of the SAME engine and batch:
    row-wise           the single-launch 8-wave step
    row-wise + causal  the two-pass sequence (forward-only launch, seed kernel, seeded reverse launch) with the slab-sum and apply
                       kernels of vn_weights.hip and one elementwise pass over the rows' seeds after the seed kernel
    dedup              the de-duplicated step
    dedup + causal     ... plus the slab-sum kernel and the n_k-sized apply kernel between the seed and the gather kernel
    dedup + static     ... plus the apply kernel alone
The variants are interleaved round by round in one process (R rounds of N steps each after a warm-up round), timed with device
events around the N steps; the median over the rounds is reported with the spread.  Slab ids: VarNet.causalSlabIds of the rows
(S = tDiscNum), eps = 1; static weights ~ U(0.2, 1.5).
Written to DIR/causal_perf.txt.  A record, not a test: no bar.  Read the row-wise figure against the reaction's two-pass figure in
profiles/reaction_perf.txt and the dedup ratio against "dedup + flux" in profiles/nlflux_perf.txt."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench


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
    n_k = n_int // eng.integNum
    S = int(vn.tDiscNum)
    slab = torch.as_tensor(vn.causalSlabIds(td.mor[0]['Input_host']), dtype=torch.int32, device=eng.device)
    omega = torch.as_tensor(np.random.default_rng(22).uniform(0.2, 1.5, n_k).astype(np.float32), device=eng.device)
    #           label                dedup  weights
    variants = [('row-wise', False, None), ('row-wise + causal', False, 'causal'), ('dedup', True, None),
                ('dedup + causal', True, 'causal'), ('dedup + static', True, 'static')]
    can_dedup = td.dedup_applies() is None
    times = {v[0]: [] for v in variants}
    for r in range(rounds + 1):                       # round 0: warm-up (allocations, first launches)
        for label, dd, wt in variants:
            if dd and not can_dedup:
                continue
            if dd:
                td.enable_dedup()
            else:
                td.disable_dedup()
            if wt == 'causal':
                eng.set_causal(b, slab, S, 1.0)
            elif wt == 'static':
                eng.set_tf_weights(b, omega)
            else:
                eng.set_causal(b)
                eng.set_tf_weights(b)
            t = timed(eng, b, steps)
            if r:
                times[label].append(t)
    td.disable_dedup()
    eng.set_causal(b)
    eng.set_tf_weights(b)
    kp = eng.kernel_path()
    out = {'problem': name, 'rows_interior': n_int, 'test_functions': n_k, 'slabs': S, 'parameters': int(eng.P),
           'steps_per_round': steps, 'rounds': rounds, 'kernel_path': list(kp),
           'unique_points': int(sum(v[0].shape[0] for v in getattr(td, '_dd_cache', {}).values()))}
    for label, ts in times.items():
        if ts:
            a = np.array(ts)
            out[label] = {'ms_median': round(float(np.median(a)), 4), 'ms_min': round(float(a.min()), 4),
                          'ms_max': round(float(a.max()), 4)}
    if 'row-wise + causal' in out and 'row-wise' in out:
        out['row-wise ratio'] = round(out['row-wise + causal']['ms_median'] / out['row-wise']['ms_median'], 4)
    for label in ('dedup + causal', 'dedup + static'):
        if label in out and 'dedup' in out:
            out[label + ' ratio'] = round(out[label]['ms_median'] / out['dedup']['ms_median'], 4)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/causal_perf.py measures on the GPU: none found')
    os.makedirs(args.out, exist_ok=True)
    lines = ['vn_set_causal / vn_set_tf_weights: ms per gradient step (vn_grad; device events around %d steps, %d interleaved rounds '
             'after a warm-up round, median [min, max]) -- python tools/causal_perf.py' % (args.steps, args.rounds),
             'expectation: row-wise + causal = the two-pass sequence (profiles/reaction_perf.txt: row-wise + reaction) plus one '
             'elementwise pass and two n_k-sized launches; dedup + causal = the plain dedup step plus two small launches, dedup + '
             'static plus one', '']
    for cfg in (3, 1):
        res = perf(cfg, args.steps, args.rounds)
        lines.append('config %d: %s' % (cfg, json.dumps(res)))
        print(lines[-1], flush=True)
        with open(os.path.join(args.out, 'causal_perf.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
