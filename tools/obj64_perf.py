"""Cost and full-size use of the fp64 objective (vn_objective_f64, VNEngine.objective64).
    python tools/obj64_perf.py [--parity | --lbfgs] [--out DIR] [--calls N]
Without --parity: ms per call, loss-only and with the gradient, on the BASELINE config 3 problem (5x50 MLP, 1e5 test functions,
6.4 M rows) and on the config 1 problem (3x20 MLP, 6e3 test functions, 96 000 rows), written to DIR/obj64_perf.txt.  A call
synchronises, so a host clock around it times the whole evaluation (pack, forward, seed, reverse, reduce, read-back); two
warm-up calls of each form, then N timed calls of each, the two forms alternating.  The matrix work is counted from the shapes:
with W = sum of H[l-1] * H[l] over the hidden layers, a row's forward pass is 2 W multiply-adds per stream (interior and flux
rows carry two streams, BC/IC rows one), the reverse pass recomputes it and adds the adjoint sweep (W - H[0] H[1] per stream)
and the weight-gradient contraction (W per stream).  Useful FLOP/s over the fp64 MFMA rate that vn_debug_calibrate_f64 measures
in the same process is the fraction reported; padding of the 16-wide tiles is not counted as work.
With --parity: VarNet.precisionReport on all rows of the config 3 problem -- the deviation of the fp32 step's loss components
and per-tensor gradient from the device's fp64 evaluation -- for the row-wise fused route and for the de-duplicated formulation,
at the initial parameters and after 200 Adam steps, written to DIR/obj64_fullsize.json.
With --lbfgs: the end-to-end L-BFGS run of the Operator_1Dt problem ([20], 96 000 rows, weights [10, 10, 1], budget 8 000 epochs)
with the line search on the fp32 loss (default) and on the fp64 loss (lbfgsLoss64=True): epochs run (a run that ends before the
budget stalled there), l2Err(cExact), trials per accepted iteration, wall time; written to DIR/obj64_lbfgs.txt.  A record."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench


def matrix_flop(vn, n_int, n_bc, grad):
    H = [vn.inpDim] + list(vn.layerWidth)
    W = sum(a * b for a, b in zip(H[:-1], H[1:]))
    fwd = 2.0 * W
    rev = 2.0 * (W - H[0] * H[1]) + 2.0 * W
    per_stream = fwd + ((fwd + rev) if grad else 0.0)
    return per_stream * (2 * n_int + n_bc)


def perf(cfg, calls):
    vn, name = bench.build_problem(cfg)
    eng = vn.engine
    td = vn._build_tdata()
    td.select_mor(0)
    b = td.engine_batch(0, 0)
    n_int = int(eng._keep[('int', b)][0].shape[0])
    bic = eng._keep.get('bic')
    n_bc = int(bic[0].shape[0]) if bic is not None else 0
    for _ in range(2):
        eng.objective64(b, grad=False)
        eng.objective64(b, grad=True)
    t_loss, t_grad = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        eng.objective64(b, grad=False)
        t_loss.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        eng.objective64(b, grad=True)
        t_grad.append((time.perf_counter() - t0) * 1e3)
    cal = eng.calibrate_f64()
    peak = cal['mfma_f64_tflops']
    out = {'problem': name, 'rows_interior': n_int, 'rows_bc_ic': n_bc, 'parameters': int(eng.P), 'calls': calls,
           'fp64_mfma_tflops_calibrated': peak}
    for key, ts, grad in (('loss_only', t_loss, False), ('with_gradient', t_grad, True)):
        a = np.array(ts)
        flop = matrix_flop(vn, n_int, n_bc, grad)
        med = float(np.median(a))
        out[key] = {'ms_median': round(med, 4), 'ms_min': round(float(a.min()), 4), 'ms_max': round(float(a.max()), 4),
                    'matrix_flop': flop, 'tflops_at_median': round(flop / (med * 1e-3) / 1e12, 4),
                    'fraction_of_calibrated_fp64_mfma_rate': round(flop / (med * 1e-3) / 1e12 / peak, 4)}
    eng.close()
    return out


def parity():
    vn, name = bench.build_problem(3)
    eng = vn.engine
    td = vn._build_tdata()
    td.select_mor(0)
    b = td.engine_batch(0, 0)
    out = {'problem': name, 'rows': int(eng._keep[('int', b)][0].shape[0]), 'points': {}}
    for label, steps in (('initial parameters', 0), ('after 200 Adam steps', 200)):
        if steps:
            eng.train_epoch((b,) * steps, None)
            torch.cuda.synchronize()
        rec = {}
        rec['row-wise'] = vn.precisionReport(td)
        if td.enable_dedup():
            rec['de-duplicated'] = vn.precisionReport(td)
            td.disable_dedup()
        out['points'][label] = rec
    eng.close()
    return out


def cExact(x, t, trunc=800, u=1.0, D=0.1 / np.pi):
    """Fourier-series solution of the 1D+t problem (examples/operator_1dt.py)."""
    pi = np.pi
    p = np.arange(0, trunc + 1.0).reshape(1, trunc + 1)
    c0 = 16 * pi ** 2 * D ** 3 * u * np.exp(u / D / 2 * (x - u * t / 2))
    e1 = np.exp(-D * p ** 2 * pi ** 2 * t)
    e2 = np.exp(-D * (2 * p + 1) ** 2 * pi ** 2 * t / 4)
    c1d = u ** 4 + 8 * (u * pi * D) ** 2 * (p ** 2 + 1) + 16 * (pi * D) ** 4 * (p ** 2 - 1) ** 2
    c2d = u ** 4 + (u * pi * D) ** 2 * (8 * p ** 2 + 8 * p + 10) + (pi * D) ** 4 * (4 * p ** 2 + 4 * p - 3) ** 2
    S = np.sinh(u / D / 2) * np.sum((-1) ** p * 2 * p * np.sin(p * pi * x) * e1 / c1d, axis=-1, keepdims=True) + \
        np.cosh(u / D / 2) * np.sum((-1) ** p * (2 * p + 1) * np.cos((p + 0.5) * pi * x) * e2 / c2d, axis=-1, keepdims=True)
    c = c0 * S
    c[t == 0] = -np.sin(pi * x[t == 0])
    return c


def lbfgs_record(epochs=8000):
    import tempfile
    from varnet_amd.adpde import ADPDE
    from varnet_amd.domain import Domain1D
    from varnet_amd.utility import UF
    from varnet_amd.varnet import VarNet
    out = []
    for loss64 in (False, True):
        pde = ADPDE(Domain1D(), diff=0.1 / np.pi, vel=1.0, timeDependent=True, tInterval=[0, 2.0],
                    IC=lambda x: -np.sin(np.pi * x), cEx=cExact)
        vn = VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=300, optimizer='lbfgs', lbfgsLoss64=loss64)
        eng = vn.engine
        trials, status = [], []
        step = eng.lbfgs_step

        def counted(*a, **kw):
            info = step(*a, **kw)
            trials.append(info['trials'])
            status.append(info['status'])
            return info
        eng.lbfgs_step = counted
        t0 = time.perf_counter()
        res = vn.train(tempfile.mkdtemp(), weight=[10., 10., 1.], epochNum=epochs, tol=0.0, saveFreq=1000, verbose=False)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        losses = np.asarray(res.lossAll, dtype=float)
        err = float(UF().l2Err(vn.fixData.cEx, vn.evaluate()))
        out.append({'line_search_loss': 'fp64' if loss64 else 'fp32', 'budget_epochs': epochs, 'epochs_run': int(len(losses)),
                    'stalled': bool(status and status[-1] == 2), 'accepted_iterations': int(eng.step),
                    'status_1_calls': int(sum(1 for x in status if x == 1)),
                    'loss_first_last': [float(losses[0]), float(losses[-1])], 'l2Err_cExact': err,
                    'trials_per_accepted_iteration': float(np.sum(trials)) / max(1, int(eng.step)),
                    'wall_s_whole_train_call': round(wall, 3)})
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parity', action='store_true')
    ap.add_argument('--lbfgs', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/obj64_perf.py measures on the GPU: none found')
    os.makedirs(args.out, exist_ok=True)
    if args.lbfgs:
        with open(os.path.join(args.out, 'obj64_lbfgs.txt'), 'w') as f:
            f.write('Operator_1Dt [20], 96 000 rows, optimizer=lbfgs, weights [10, 10, 1]: line search on the fp32 loss (default) '
                    'and on the fp64 loss (lbfgsLoss64=True) -- python tools/obj64_perf.py --lbfgs\n\n')
            for rec in lbfgs_record():
                f.write(json.dumps(rec) + '\n')
                print(json.dumps(rec), flush=True)
        return
    if args.parity:
        res = parity()
        with open(os.path.join(args.out, 'obj64_fullsize.json'), 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(json.dumps(res))
        return
    lines = ['vn_objective_f64: ms per call (host clock around a call that ends in a device synchronise; %d calls of each form,'
             % args.calls, 'alternating, after two warm-up calls of each) -- python tools/obj64_perf.py', '']
    for cfg in (3, 1):
        res = perf(cfg, args.calls)
        lines.append('config %d: %s' % (cfg, json.dumps(res)))
        print(lines[-1], flush=True)
        with open(os.path.join(args.out, 'obj64_perf.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
