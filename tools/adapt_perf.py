"""Cost of the self-adaptive test-function weights (vn_set_tf_adapt, VarNet(tfAdapt=...)) on the training step.
    python tools/adapt_perf.py [--out DIR] [--steps N] [--rounds R] [--commit HASH]
On BASELINE configs 1, 2 and 3, row-wise and de-duplicated, ms per step of vn_train_epoch (N steps enqueued by one host call,
device events around them) for four registrations of the SAME engine and batch:
    static      vn_set_tf_weights with a fixed [n_k] array: the parent's own path, the baseline -- the difference to it is the
                feature's (a plain unweighted step takes another route on the single-launch kernels and is no baseline here)
    rba         tfAdapt='rba': three more n_k-sized launches per step (reduce, update, normalise; vn_adapt.hip)
    sa          tfAdapt='sa': the same three, with the two Adam slots
    every=10    rba updating on every tenth step: nine of ten steps are static-weights steps
The variants are interleaved round by round in one process (R rounds after a warm-up round); the median over the rounds is
reported with the spread, and the overhead per step against static in microseconds.  In the same run: the time of three
back-to-back launches of an n_k-sized elementwise torch kernel, the yardstick the overhead is read against.
Written to DIR/adapt_perf.txt.  A record, not a test: no bar."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench

VARIANTS = [('static', None), ('rba', 'rba'), ('sa', 'sa'), ('every=10', {'rule': 'rba', 'every': 10})]


def timed(eng, b, steps):
    ids = (b,) * steps
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    eng.train_epoch(ids)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def three_launches(n_k, steps, device):
    x = torch.zeros(n_k, dtype=torch.float32, device=device)
    for _ in range(30):
        x.add_(1.0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3 * steps):
        x.add_(1.0)
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
    omega = torch.as_tensor(np.random.default_rng(22).uniform(0.2, 1.5, n_k).astype(np.float32), device=eng.device)
    state0 = eng.export_state()                       # every variant and round starts from the same parameters
    can_dedup = td.dedup_applies() is None
    out = {'problem': name, 'rows_interior': n_int, 'test_functions': n_k, 'parameters': int(eng.P), 'steps_per_round': steps,
           'rounds': rounds, 'kernel_path': list(eng.kernel_path())}
    for form in ('row-wise', 'dedup'):
        if form == 'dedup' and not can_dedup:
            continue
        times = {v[0]: [] for v in VARIANTS}
        n = steps
        for r in range(rounds + 1):                   # round 0: warm-up (allocations, first launches), and the window's size
            for label, spec in VARIANTS:
                if form == 'dedup':
                    td.enable_dedup()
                else:
                    td.disable_dedup()
                if spec is None:
                    eng.set_tf_weights(b, omega)
                else:
                    eng.set_tf_adapt(b, spec)
                if spec is None:
                    eng.import_state(state0)
                else:                                 # (the adaptive state follows the optimizer state in the exported layout)
                    eng.import_state(np.concatenate([state0, eng.export_state()[state0.size:]]))
                t = timed(eng, b, n)
                if r:
                    times[label].append(t)
                elif label == 'static':               # a timed window of a quarter of a second at least (config 1: 40 us steps)
                    n = int(min(8000, max(steps, 250.0 / t)))
        res = {}
        for label, ts in times.items():
            a = np.array(ts)
            if not ts:
                continue
            res[label] = {'ms_median': round(float(np.median(a)), 5), 'ms_min': round(float(a.min()), 5), 'ms_max': round(float(a.max()), 5)}
        for label in ('rba', 'sa', 'every=10'):
            res[label]['us_over_static'] = round(1e3 * (res[label]['ms_median'] - res['static']['ms_median']), 2)
        res['steps_per_window'] = n
        out[form] = res
    eng.set_tf_adapt(b)
    td.disable_dedup()
    out['three_torch_launches_us'] = round(1e3 * three_launches(n_k, 2000, eng.device), 2)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--commit', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/adapt_perf.py measures on the GPU: none found')
    os.makedirs(args.out, exist_ok=True)
    lines = ['vn_set_tf_adapt: ms per step of vn_train_epoch (device events around one host call of at least %d steps and a quarter of a second, %d interleaved rounds '
             'after a warm-up round, median [min, max]; us_over_static: median minus the static registration\'s) -- python '
             'tools/adapt_perf.py' % (args.steps, args.rounds),
             'taken at: %s' % (args.commit or 'unrecorded'),
             'expectation: three n_k-sized launches per updating step; every=10 a tenth of that', '']
    for cfg in (1, 2, 3):
        res = perf(cfg, args.steps, args.rounds)
        lines.append('config %d: %s' % (cfg, json.dumps(res)))
        print(lines[-1], flush=True)
        with open(os.path.join(args.out, 'adapt_perf.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
