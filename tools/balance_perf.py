"""Cost of a balancing probe (vn_term_grads, VarNet.train(balance=...)) next to a training step: on BASELINE configs 1, 2 and 3 the
time of one probe over the batch (the active terms' gradient evaluations, two small launches per term, the statistics pair and the
one read-back) and of one plain vn_train_step on the same engine, interleaved in one process, device events, three rounds, minima.
    python tools/balance_perf.py [steps] [--out DIR] [--parent-tree DIR]
--parent-tree: a built checkout of the parent commit; its plain train_step is timed by this script in a fresh child process that
imports that tree, before and after this tree's measurement (the same box, the same steps).  Prints one JSON line per config and
writes them to DIR/balance_perf.txt (default profiles/).  No pass / fail bar."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
opt = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
sys.path.insert(0, os.path.abspath(opt('--tree')) if opt('--tree') else ROOT)       # (--tree: the child's side of --parent-tree)

PLAIN_ONLY = '--plain-only' in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith('--') and a not in (opt('--parent-tree'), opt('--out'), opt('--tree'))]
STEPS = int(args[0]) if args else 300
OUT = opt('--out') or os.path.join(ROOT, 'profiles')
ROUNDS = 3


def parent_ms(tree):
    """{config: [ms per plain step]} of a child process on the parent commit's tree."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(STEPS), '--plain-only', '--tree', tree], capture_output=True,
                       text=True, timeout=600)
    if r.returncode:
        raise SystemExit('the child on %s failed:\n%s' % (tree, r.stderr[-2000:]))
    return {str(j['config']): j['plain_ms'] for j in (json.loads(l) for l in r.stdout.splitlines() if l.startswith('{'))}


before = parent_ms(opt('--parent-tree')) if opt('--parent-tree') else None

import torch  # noqa: E402

import bench  # noqa: E402


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


lines = []
for cfg in (1, 2, 3):
    vn, name = bench.build_problem(cfg)
    td = vn._build_tdata()
    td.select_mor(0)
    eng = vn.engine
    eng.set_weights([3.0, 2.0, 5.0])
    steps = STEPS if cfg != 3 else max(20, STEPS // 10)
    probes = max(5, steps // 10)
    out = {'config': cfg, 'problem': name, 'P': int(eng.P), 'steps': steps, 'probes': probes, 'plain_ms': [], 'probe_ms': []}
    theta = eng.get_params()
    for _ in range(ROUNDS):                         # interleaved: a drift of the clock shows as a spread between repeats
        eng.set_params(theta)
        out['plain_ms'].append(round(timed(lambda: eng.train_step(0), steps, 10), 5))
        if PLAIN_ONLY:
            continue
        eng.set_params(theta)
        out['probe_ms'].append(round(timed(lambda: eng.term_grads((0,)), probes, 2), 5))
    if not PLAIN_ONLY:
        r = eng.term_grads((0,))
        out['terms'] = int(sum(1 for s in r['sumsq'] if s > 0.0))
        out['probe_over_step'] = round(min(out['probe_ms']) / min(out['plain_ms']), 2)
        out['share_at_freq_1000'] = round(min(out['probe_ms']) / min(out['plain_ms']) / 1000.0, 5)
    print(json.dumps(out), flush=True)
    lines.append(out)
    eng.close()

if not PLAIN_ONLY:
    after = parent_ms(opt('--parent-tree')) if opt('--parent-tree') else None
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'balance_perf.txt'), 'w') as f:
        f.write('tools/balance_perf.py %d, one MI355X: ms per vn_train_step (plain) and per vn_term_grads probe over the batch (the host\n'
                'call, its one synchronisation included), device events, interleaved (%d rounds each).\n' % (STEPS, ROUNDS))
        for out in lines:
            if before is not None:
                out['parent_plain_ms_before'], out['parent_plain_ms_after'] = before[str(out['config'])], after[str(out['config'])]
            f.write(json.dumps(out) + '\n')
