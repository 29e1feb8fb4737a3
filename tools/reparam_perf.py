"""Per-step cost of the learnt weight scales (vn_set_reparam, VarNet(..., reparam=...)): vn_train_step on BASELINE configs 1, 2
and 3, plain and with each mode registered on the same engine, interleaved in one process and timed with device events.
    python tools/reparam_perf.py [steps] [--out DIR] [--parent-tree DIR]
A plain step folds the optimizer into the gradient reduction; a reparametrised step un-folds it and adds the stage's one launch
(vn_reparam.hip).  --parent-tree: a built checkout of the parent commit; its plain train_step is timed by this script in a fresh
child process that imports that tree, before and after this tree's measurement (the same box, the same steps).  Prints one JSON line per config and writes them
to DIR/reparam_perf.txt (default profiles/).  No pass / fail bar."""
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
MODES = [('rwf', dict(mode='rwf')), ('slope_neuron', dict(mode='slope', per='neuron', n=10.0)),
         ('slope_layer', dict(mode='slope', per='layer', n=10.0))]


def parent_ms(tree):
    """{config: [ms per plain step]} of a child process on the parent commit's tree."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(STEPS), '--plain-only', '--tree', tree], capture_output=True,
                       text=True, timeout=600)
    if r.returncode:
        raise SystemExit('the child on %s failed:\n%s' % (tree, r.stderr[-2000:]))
    out = r.stdout
    return {str(j['config']): j['plain_ms'] for j in (json.loads(l) for l in out.splitlines() if l.startswith('{'))}


before = parent_ms(opt('--parent-tree')) if opt('--parent-tree') else None

import torch  # noqa: E402

import bench  # noqa: E402


def step_ms(eng, batch, steps):
    for _ in range(10):
        eng.train_step(batch)                       # warm-up
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        eng.train_step(batch)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


lines = []
for cfg in (1, 2, 3):
    vn, name = bench.build_problem(cfg)
    td = vn._build_tdata()
    td.select_mor(0)
    eng = vn.engine
    eng.set_weights([3.0, 2.0, 5.0])
    batch = 0
    steps = STEPS if cfg != 3 else max(20, STEPS // 10)
    out = {'config': cfg, 'problem': name, 'steps': steps, 'plain_ms': []}
    out.update({k + '_ms': [] for k, _ in MODES})
    theta = eng.get_params()
    for _ in range(ROUNDS):                         # interleaved: a drift of the clock shows as a spread between repeats
        eng.set_params(theta)
        out['plain_ms'].append(round(step_ms(eng, batch, steps), 5))
        if PLAIN_ONLY:
            continue
        for k, kw in MODES:
            eng.set_params(theta)
            eng.set_reparam(**kw)
            out[k + '_ms'].append(round(step_ms(eng, batch, steps), 5))
            eng.set_reparam(None)
    if not PLAIN_ONLY:
        for k, _ in MODES:
            out[k + '_extra_us'] = round((min(out[k + '_ms']) - min(out['plain_ms'])) * 1e3, 2)
    print(json.dumps(out), flush=True)
    lines.append(out)
    eng.close()

if not PLAIN_ONLY:
    after = parent_ms(opt('--parent-tree')) if opt('--parent-tree') else None
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'reparam_perf.txt'), 'w') as f:
        f.write('tools/reparam_perf.py %d, one MI355X: vn_train_step, ms per step (device events), plain and with each mode of\n'
                'vn_set_reparam registered on the same engine, interleaved (%d rounds each); slope modes with n = 10.\n' % (STEPS, ROUNDS))
        for out in lines:
            if before is not None:
                out['parent_plain_ms_before'], out['parent_plain_ms_after'] = before[str(out['config'])], after[str(out['config'])]
            f.write(json.dumps(out) + '\n')
