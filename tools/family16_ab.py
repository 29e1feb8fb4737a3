"""Bit-level A/B of the 8-wave kernel family: every instantiation of the table in varnet_amd/csrc/vn_fused16_common.h (VN16_TABLE)
and both activations through every entry point that dispatches on it, one sha256 per (instantiation, entry point, point count).
Two builds whose device code is the same give equal files; the committed one is profiles/family16_ab.json.

    python tools/family16_ab.py OUT.json [TREE]

TREE is the checkout whose built library is exercised (default: this one); the table is always this checkout's.  One child process
per row of the table (one k-step count), each under its own time limit; the first failure ends the run and no file is written.
"""
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH = {5: 20, 8: 32, 13: 50, 16: 64}          # widest hidden layer an instantiation of KS k-steps serves
D_IN, DIM, INTEG_NUM, N_TF, N_BIC, BDOF = 3, 2, 4, 40, 30, 20
ROW_TIMEOUT_S = 240


def family_table():
    """[(L, KS), ...] in the order of VN16_TABLE."""
    src = open(os.path.join(ROOT, 'varnet_amd', 'csrc', 'vn_fused16_common.h')).read()
    body = re.search(r'#define VN16_TABLE\(F, S\)((?:.*\\\n)*.*)\n', src).group(1)
    return [(int(l), int(ks)) for l, ks in re.findall(r'[FS]\((\d+), *(\d+)\)', body)]


def key_of(L, KS, act):
    return 'L%d_KS%d_%s' % (L, KS, act)


def make_case(L, KS, act):
    """Parameters, points and a small weak-form batch for one instantiation, in numpy from a fixed seed."""
    import numpy as np
    rng = np.random.default_rng(1000 * KS + 10 * L + (act == 'tanh'))
    widths = [WIDTH[KS]] * L
    P = sum(a * b + b for a, b in zip([D_IN] + widths, widths + [1]))
    nT = N_TF * INTEG_NUM
    return dict(
        widths=widths, act=act, theta=rng.uniform(-0.5, 0.5, P).astype(np.float32),
        N1=rng.uniform(0, 1, INTEG_NUM).astype(np.float32), dNt1=rng.standard_normal(INTEG_NUM).astype(np.float32),
        Input=rng.uniform(-1, 1, (nT, D_IN)).astype(np.float32), gcoef=rng.standard_normal((nT, DIM)).astype(np.float32),
        biInput=rng.uniform(-1, 1, (N_BIC, D_IN)).astype(np.float32), biLabel=rng.standard_normal((N_BIC, 1)).astype(np.float32),
        rng=rng)


def make_engine(case):
    from varnet_amd.engine import VNEngine
    eng = VNEngine(DIM, D_IN, case['widths'], True, INTEG_NUM, activationFun=case['act'])
    assert eng.P == case['theta'].size
    eng.set_params(case['theta'])
    return eng


def point_outputs(eng, case, n):
    """{entry point: [tensors]} at n points drawn from the case's generator."""
    import numpy as np
    rng = case['rng']
    X = rng.uniform(-1, 1, (n, D_IN))
    diff, vel = rng.uniform(0.01, 0.1, n), rng.standard_normal((n, DIM))
    X32 = X.astype(np.float32)
    return {
        'forward': [eng.forward(X32)],
        'forward_grad': list(eng.forward_grad(X32)),
        'residual': list(eng.residual(X32, diff, vel)),
        'residual_f64': list(eng.residual(X, diff, vel, fp64=True)),
        'forward_f64': [eng.forward_f64(X)],
    }


def grad_output(eng, case):
    """{'grad': [gradient buffer]} of the case's weak-form batch."""
    import numpy as np
    import torch
    eng.set_fe_table(case['N1'], case['dNt1'])
    eng.set_interior(0, case['Input'], case['gcoef'], None, n_k=N_TF, detJ=0.01)
    eng.set_bic(case['biInput'], case['biLabel'], BDOF, 2.0)
    eng.set_weights(np.array([2.0, 3.0, 4.0]))
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    return {'grad': [gb]}


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def run_row(ks, out):
    import torch
    sys.path.insert(0, os.getcwd())
    big = 16 * 8 * 2 * torch.cuda.get_device_properties(0).multi_processor_count + 17      # past the grid cap: the grid-stride loop runs
    res = {}
    for L, KS in family_table():
        if KS != ks:
            continue
        for act in ('sigmoid', 'tanh'):
            case = make_case(L, KS, act)
            eng = make_engine(case)
            rec = {}
            for n, tag in ((17, '17'), (big, 'big')):
                for name, ts in point_outputs(eng, case, n).items():
                    rec['%s@%s' % (name, tag)] = digest(ts)
            rec['grad'] = digest(grad_output(eng, case)['grad'])
            eng.close()
            res[key_of(L, KS, act)] = rec
    json.dump(res, open(out, 'w'))


def main():
    if sys.argv[1] == '--row':
        return run_row(int(sys.argv[2]), sys.argv[3])
    out = os.path.abspath(sys.argv[1])
    tree = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ROOT
    res = {}
    for ks in sorted(WIDTH):
        part = out + '.ks%d' % ks
        # a fresh child per row, under its own time limit; a failure (or a child that ran out of time) ends the run
        subprocess.run([sys.executable, os.path.abspath(__file__), '--row', str(ks), part], cwd=tree, timeout=ROW_TIMEOUT_S, check=True)
        res.update(json.load(open(part)))
        os.remove(part)
        print('KS %d: %d instantiations' % (ks, sum(1 for k in res if '_KS%d_' % ks in k)), flush=True)
    assert len(res) == 2 * len(family_table())
    with open(out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
