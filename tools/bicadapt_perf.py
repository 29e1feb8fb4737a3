"""Cost of the weights on the boundary and initial rows (vn_set_bic_weights, vn_set_bic_adapt, VarNet(bicWeights=..., bicAdapt=...))
on the training step.
    python tools/bicadapt_perf.py [--out DIR] [--steps N] [--rounds R] [--commit HASH]
On BASELINE configs 1, 2 and 3, row-wise and de-duplicated, ms per step of vn_train_epoch (N steps enqueued by one host call,
device events around them) for four states of the SAME engine and batch:
    plain       no registration: the parent's own step, the BC/IC rows inside the step's main launch
    static      vn_set_bic_weights with a fixed [nB] array: the rows leave the main launch and run their own pass -- the 8-wave
                kernel's forward-only mode, the rows' seed kernel, generic reverse pass (vn_bicadapt.hip); this difference is the
                price of the feature
    rba         static's pass plus, per adaptive part, the three launches of vn_adapt.hip on the part's own loss field; both parts
                of a time-dependent problem are registered
    sa          the same with the two Adam slots
The variants are interleaved round by round in one process (R rounds after a warm-up round); the median over the rounds is
reported with the spread, and the overhead per step in microseconds: static over plain, rba and sa over static.  Also recorded:
what vn_profile_begin / vn_profile_end count over ten unregistered steps (the regions of the step's own kernel sequence).
Written to DIR/bicadapt_perf.txt.  A record, not a test: no bar is fixed for the registered step."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench

VARIANTS = ['plain', 'static', 'rba', 'sa']


def timed(eng, b, steps):
    ids = (b,) * steps
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    eng.train_epoch(ids)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def register(eng, label, omega):
    eng.set_bic_weights(None)
    if label.startswith('static'):
        eng.set_bic_weights(omega)
    elif label != 'plain':
        for part in ('bc', 'ic'):
            if eng.bic_rows(part) > 0:
                eng.set_bic_adapt(part, label)


def perf(cfg, steps, rounds):
    vn, name = bench.build_problem(cfg)
    eng = vn.engine
    td = vn._build_tdata()
    td.select_mor(0)
    b = td.engine_batch(0, 0)
    n_int = int(eng._keep[('int', b)][0].shape[0])
    rows = (eng.bic_rows('bc'), eng.bic_rows('ic'))
    omega = torch.as_tensor(np.random.default_rng(22).uniform(0.2, 1.5, sum(rows)).astype(np.float32), device=eng.device)
    state0 = eng.export_state()                       # every variant and round starts from the same parameters
    can_dedup = td.dedup_applies() is None
    out = {'problem': name, 'rows_interior': n_int, 'rows_bc_ic': list(rows), 'parameters': int(eng.P), 'steps_per_round': steps,
           'rounds': rounds, 'kernel_path': list(eng.kernel_path())}
    for form in ('row-wise', 'dedup'):
        if form == 'dedup' and not can_dedup:
            continue
        times = {v: [] for v in VARIANTS}
        n = steps
        for r in range(rounds + 1):                   # round 0: warm-up (allocations, first launches), and the window's size
            for label in VARIANTS:
                if form == 'dedup':
                    td.enable_dedup()
                else:
                    td.disable_dedup()
                register(eng, label, omega)
                # (the rows' state follows the optimizer state in the exported layout)
                eng.import_state(np.concatenate([state0, eng.export_state()[state0.size:]]))
                t = timed(eng, b, n)
                if r:
                    times[label].append(t)
                elif label == 'plain':                # a timed window of a quarter of a second at least (config 1: 40 us steps)
                    n = int(min(8000, max(steps, 250.0 / t)))
        res = {}
        for label, ts in times.items():
            a = np.array(ts)
            res[label] = {'ms_median': round(float(np.median(a)), 5), 'ms_min': round(float(a.min()), 5), 'ms_max': round(float(a.max()), 5)}
        res['static']['us_over_plain'] = round(1e3 * (res['static']['ms_median'] - res['plain']['ms_median']), 2)
        for label in ('rba', 'sa'):
            res[label]['us_over_static'] = round(1e3 * (res[label]['ms_median'] - res['static']['ms_median']), 2)
        res['steps_per_window'] = n
        register(eng, 'plain', omega)                 # the unregistered step: regions vn_profile_* counts over ten steps
        eng.profile_begin()
        eng.train_epoch((b,) * 10)
        res['plain']['profile_regions_10_steps'] = int(eng.profile_end()[1])
        out[form] = res
    eng.set_bic_weights(None)
    td.disable_dedup()
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
        raise SystemExit('tools/bicadapt_perf.py measures on the GPU: none found')
    os.makedirs(args.out, exist_ok=True)
    lines = ['vn_set_bic_weights / vn_set_bic_adapt: ms per step of vn_train_epoch (device events around one host call of at least %d steps '
             'and a quarter of a second, %d interleaved rounds after a warm-up round, median [min, max]; us_over_plain: the static '
             'registration\'s median minus the unregistered step\'s; us_over_static: median minus the static registration\'s) -- python '
             'tools/bicadapt_perf.py' % (args.steps, args.rounds),
             'taken at: %s' % (args.commit or 'unrecorded'),
             'expectation: static = plain + the rows\' own pass (three launches); rba, sa = static + three n_s-sized launches per part', '']
    for cfg in (1, 2, 3):
        res = perf(cfg, args.steps, args.rounds)
        lines.append('config %d: %s' % (cfg, json.dumps(res)))
        print(lines[-1], flush=True)
        with open(os.path.join(args.out, 'bicadapt_perf.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
