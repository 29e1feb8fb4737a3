"""
GPU tier of the device-resident L-BFGS optimizer (vn_lbfgs_step, `VNEngine(optimizer_name='lbfgs')`,
`VarNet(optimizer='lbfgs')`): teacher-forced step parity of the device's Gram-form recursion against the plain two-loop
restatement of tests/lbfgs_ref.py on every route, the line-search contract read from `info`, bitwise repeatability,
invalidation, the refusals and the restore after a failed search, and one converged run of the 1D+t problem.
Figures go to profile_out/lbfgs_parity.json (kept out of git; a copy of one run is committed as profiles/lbfgs_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import lbfgs_ref as ref
from tests.parity_cases import synth
from tests.test_flux_bc_gpu import flux_rows
from tests.test_varnet_host import cExact
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import VN_KERNEL_AUTO, VN_KERNEL_GENERIC, VN_KERNEL_LAYERED, VNEngine, VNError
from varnet_amd.utility import UF
from varnet_amd.varnet import VarNet

pytestmark = pytest.mark.gpu

uf = UF()
pi = np.pi
CFG1_BAR = 0.05             # tests/test_exact_tables.py: l2Err(fixData.cEx, evaluate()) of the Operator_1Dt problem
# Step parity.  Both sides see identical fp32 inputs and the device's inner products are fp64: what differs is the rounding to
# fp32 of d, of t d and of the sum (three roundings of 6e-8), times 5 for what the two-loop makes of the fp64 summation-order
# difference.
PARITY_BAR = 1e-6
ITERS = 30

#            d_in dim widths                integNum n_k nB  bDof kernel            extra
NETS = {
    'w20_din2':   (2, 1, [20],                 16,  40, 50, 30, VN_KERNEL_AUTO, None),
    '3x20':       (3, 2, [20, 20, 20],         64,  9,  33, 20, VN_KERNEL_AUTO, None),
    '5x50':       (3, 2, [50, 50, 50, 50, 50], 64,  9,  77, 40, VN_KERNEL_AUTO, None),
    '5x50_dedup': (3, 2, [50, 50, 50, 50, 50], 64,  9,  77, 40, VN_KERNEL_AUTO, 'dedup'),
    '5x50_flux':  (3, 2, [50, 50, 50, 50, 50], 64,  9,  77, 40, VN_KERNEL_AUTO, 'flux'),
    'generic':    (3, 2, [10, 20],             64,  5,  33, 20, VN_KERNEL_GENERIC, None),
    'layered':    (2, 1, [128, 128],           16,  40, 50, 30, VN_KERNEL_LAYERED, None),
}


def record(key, value):
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, 'lbfgs_parity.json')
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[key] = value
        json.dump(data, open(path, 'w'), indent=1, sort_keys=True)
    except OSError:
        pass


def make_engine(name, optimizer='lbfgs', seed=11):
    d_in, dim, widths, q, n_k, nB, bDof, kernel, extra = NETS[name]
    d = synth(seed, d_in, dim, widths, q, n_k, nB, bDof)
    eng = VNEngine(dim, d_in, widths, True, q, kernel=kernel, optimizer_name=optimizer)
    eng.init_params(seed=0)
    eng.set_fe_table(d['N1'], d['dNt1'], None)
    eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=n_k, detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
    eng.set_weights(d['w'])
    if extra == 'dedup':
        nT = d['Input'].shape[0]
        idx = torch.arange(nT, dtype=torch.int32)
        eng.set_dedup(0, d['Input'], idx, torch.arange(nT + 1, dtype=torch.int32), idx)
    if extra == 'flux':
        fx = flux_rows(seed + 1, d_in, dim, 60)
        eng.set_flux_bc(fx['X'], fx['normal'], fx['coef'], fx['label'], 2.0)
    return eng, d


def read_grad(eng):
    gb = eng.bind_grad_buffer()
    torch.cuda.synchronize()
    return gb.cpu().numpy()[:eng.P].copy()


_RUNS = {}


def run(name):
    """ITERS calls from vn_params_init(seed 0); per call: info, (theta_k, g_k) before it, (theta, gradient buffer) after it, the
    step counter.  Shared by the parity and the contract test."""
    if name in _RUNS:
        return _RUNS[name]
    eng, _ = make_engine(name)
    try:
        eng.bind_grad_buffer()                       # the gradient buffer the test reads
        eng.grad(0)                                  # g_0 (the optimizer evaluates it again, for itself)
        theta, g = eng.get_params(), read_grad(eng)
        calls = []
        for _ in range(ITERS):
            info = eng.lbfgs_step(0, 20)
            theta1, g1 = eng.get_params(), read_grad(eng)
            calls.append(dict(info=info, theta=theta, g=g, theta1=theta1, g1=g1, step=eng.step))
            if info['status'] == 0:
                theta, g = theta1, g1
        _RUNS[name] = calls
    finally:
        eng.close()
    return calls


@pytest.mark.parametrize('name', list(NETS))
def test_step_parity_teacher_forced(name):
    """The restatement gets the DEVICE's theta_k, g_k, pairs (rebuilt in fp32 from what was read back) and accepted t; its
    theta_k + t d against the device's theta_{k+1}: max |diff| <= 1e-6 max(|theta_{k+1}|_inf, |t d|_inf)."""
    calls = run(name)
    pairs, worst, accepted = [], 0.0, 0
    for k, c in enumerate(calls):
        info = c['info']
        if info['status'] != 0:
            assert np.array_equal(c['theta1'], c['theta'])
            del pairs[:]
            continue
        accepted += 1
        d, gd, used = ref.direction(c['g'].astype(np.float64), pairs)
        assert used == info['pairs'], (name, k, used, info)
        t = info['t']
        want = c['theta'].astype(np.float64) + t * d
        scale = max(float(np.max(np.abs(c['theta1']))), float(np.max(np.abs(t * d))))
        ratio = float(np.max(np.abs(want - c['theta1'].astype(np.float64)))) / (PARITY_BAR * scale)
        worst = max(worst, ratio)
        assert abs(gd - info['gd']) <= 1e-6 * abs(gd), (name, k, gd, info['gd'])
        ref.push_pair(pairs, c['theta1'] - c['theta'], c['g1'] - c['g'])          # fp32 differences: fl32(.) as specified
    print('%s: %d accepted iterations, largest parity ratio %.3f of the bar' % (name, accepted, worst))
    record('parity_ratio_' + name, dict(largest_ratio_of_bar=worst, bar=PARITY_BAR, accepted=accepted, calls=len(calls)))
    assert accepted >= ITERS // 2                    # (the comparison is not vacuous)
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize('name', list(NETS))
def test_line_search_contract(name):
    calls = run(name)
    pairs_len, accepted, f_prev = 0, 0, None
    for k, c in enumerate(calls):
        info = c['info']
        t0 = 1.0 if info['pairs'] else min(1.0, 1.0 / float(np.sum(np.abs(c['g'].astype(np.float64)))))
        assert info['gd'] < 0.0
        assert info['pairs'] in (pairs_len, 0), (name, k, info, pairs_len)      # (0: dropped for g.d >= 0)
        if f_prev is not None:
            assert info['f_k'] == f_prev, (name, k)               # bit for bit
        if info['status'] == 0:
            accepted += 1
            j = info['trials'] - 1
            assert 0 <= j < 20
            assert abs(info['t'] - t0 * 0.5 ** j) <= 1e-12 * info['t'], (name, k, info, t0)
            assert info['f_next'] <= info['f_k'] + ref.C1 * info['t'] * info['gd']
            assert info['f_next'] <= info['f_k']
            kept = ref.keeps_pair(c['theta1'] - c['theta'], c['g1'] - c['g'])
            pairs_len = min(info['pairs'] + (1 if kept else 0), ref.HISTORY)
            f_prev = info['f_next']
        else:
            assert info['status'] == (1 if info['pairs'] else 2) and info['trials'] == 20
            pairs_len, f_prev = 0, info['f_k']
        assert c['step'] == accepted
    # the ring fills: 10 pairs from the 11th accepted iteration on unless something was dropped
    assert max(c['info']['pairs'] for c in calls) == ref.HISTORY


@pytest.mark.parametrize('name', ['w20_din2', '5x50'])
def test_bitwise_repeatability(name):
    out = []
    for _ in range(2):
        eng, _ = make_engine(name)
        try:
            infos = [eng.lbfgs_step(0, 20) for _ in range(40)]
            out.append((infos, eng.get_params()))
        finally:
            eng.close()
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


def test_invalidation():
    eng, d = make_engine('3x20')
    try:
        def warm():
            for _ in range(4):
                assert eng.lbfgs_step(0)['status'] == 0
            assert eng.lbfgs_step(0)['pairs'] >= 3

        def check(what):
            info = eng.lbfgs_step(0)
            assert info['pairs'] == 0, (what, info)
            return info

        warm()
        eng.set_weights([1.0, 4.0, 2.0])
        want = eng.eval_loss(0)[0][0]
        info = check('set_weights')
        assert abs(info['f_k'] - want) <= 1e-5 * abs(want)
        warm()
        eng.set_params(eng.get_params() * np.float32(0.9))
        want = eng.eval_loss(0)[0][0]
        info = check('set_params')
        assert abs(info['f_k'] - want) <= 1e-5 * abs(want)
        warm()
        n_k = NETS['3x20'][4]
        eng.set_interior(0, d['Input'][::-1].copy(), d['gcoef'], None, n_k=n_k, detJ=d['detJ'])
        want = eng.eval_loss(0)[0][0]
        info = check('set_interior')
        assert abs(info['f_k'] - want) <= 1e-5 * abs(want)
        # weights changed and put back between two calls (what train()'s monitors do) leave the optimizer alone
        warm()
        w = [1.0, 4.0, 2.0]
        eng.set_weights([1.0, 1.0, 1.0])
        eng.eval_loss(0)
        eng.set_weights(w)
        assert eng.lbfgs_step(0)['pairs'] >= 3
        # a caller's vn_grad between two calls does not disturb g_k, and a checkpoint restarts from steepest descent
        f = eng.lbfgs_step(0)['f_next']
        eng.grad(0)
        assert eng.lbfgs_step(0)['f_k'] == f
        state = eng.export_state()
        P = eng.P
        assert not np.any(state[8 + 4 * P:]) and int(state[:8].view(np.int64)[0]) == eng.step
        eng.import_state(state)
        check('import_state')
    finally:
        eng.close()


def test_refusals():
    eng, _ = make_engine('w20_din2')
    try:
        acc = torch.zeros((), dtype=torch.float32, device='cuda')
        with pytest.raises(VNError, match='error 3: vn_train_epoch'):
            eng.train_epoch([0], acc)
        with pytest.raises(VNError, match='error 3: vn_train_step'):
            eng.train_step(0)
        with pytest.raises(VNError, match='error 3: vn_apply'):
            eng.apply()
        with pytest.raises(VNError, match='error 3: vn_state_snapshot'):
            eng.state_snapshot()
        with pytest.raises(VNError, match='error 3: vn_state_rollback'):
            eng.state_rollback()
        eng.comm_init(0, 1, VNEngine.comm_unique_id())
        with pytest.raises(VNError, match='error 5: vn_lbfgs_step under a communicator'):
            eng.lbfgs_step(0)
    finally:
        eng.close()
    eng, _ = make_engine('w20_din2', optimizer='adam')
    try:
        with pytest.raises(VNError, match='error 3: vn_lbfgs_step needs an engine created with optimizer = VN_OPT_LBFGS'):
            eng.lbfgs_step(0)
    finally:
        eng.close()


def op1dt(tDiscNum, **kw):
    pde = ADPDE(Domain1D(), diff=0.1 / pi, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x),
                cEx=cExact)
    return VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=tDiscNum, **kw)


def test_failed_search_restores_theta(tmp_path):
    """max_trials = 1 until the first call whose only trial is rejected: theta comes back bit for bit, the step counter stands,
    status 1 with pairs in the ring (and the next direction is formed without them), 2 without."""
    vn = op1dt(20, optimizer='lbfgs')
    eng = vn.engine
    try:
        vn.train(str(tmp_path), weight=[10., 10., 1.], epochNum=1, tol=0.0, saveFreq=10 ** 6, verbose=False)
        hit = None
        for k in range(100):
            theta, step = eng.get_params(), eng.step
            info = eng.lbfgs_step(0, 1)
            if info['status'] != 0:
                hit = k
                break
        assert hit is not None, 'no rejected first trial in 100 calls'
        assert np.array_equal(eng.get_params().view(np.uint32), theta.view(np.uint32)) and eng.step == step
        assert info['status'] == (1 if info['pairs'] else 2) and info['trials'] == 1 and info['f_next'] == info['f_k']
        nxt = eng.lbfgs_step(0, 20)
        assert nxt['pairs'] == 0 and nxt['f_k'] == info['f_k']
        record('first_rejected_first_trial', dict(call=hit, status=info['status'], pairs=info['pairs']))
    finally:
        eng.close()


E2E_EPOCHS = 8000


def test_end_to_end_operator_1dt(tmp_path):
    """Operator_1Dt size ([20], discNum 20, tDiscNum 300, uniform, weights [10, 10, 1]), 8 000 epochs of L-BFGS:
    l2Err(fixData.cEx, evaluate()) <= 0.05 (CFG1_BAR).
    The fp64 restatement (tests/lbfgs_ref.py under VarNet.train, on the oracle engine; no history restarts) on this problem:
    l2Err 0.064 at epoch 4 500, 0.048 at 4 750 (the first sample below the bar; sampled every 250 epochs), between 0.036 and 0.043
    at every sample from there to 8 000, 0.0415 at epoch 8 000 (8 896 gradient evaluations, 1.11 per epoch, no status != 0): it stays
    below the bar from its crossing to the end, so the test looks at the end.  The device's run (fp32 losses) takes another
    path through the same landscape: it reports 'stalled' at epoch 6 690 with l2Err 0.023 (profiles/lbfgs_parity.json)."""
    vn = op1dt(300, optimizer='lbfgs')
    eng = vn.engine
    try:
        assert vn.fixData.nT == 96000 and eng.P == 81
        trials = []
        step = eng.lbfgs_step

        def counted(*a, **kw):
            info = step(*a, **kw)
            trials.append(info['trials'])
            return info
        eng.lbfgs_step = counted
        res = vn.train(str(tmp_path), weight=[10., 10., 1.], epochNum=E2E_EPOCHS, tol=0.0, saveFreq=1000, verbose=False)
        err = float(uf.l2Err(vn.fixData.cEx, vn.evaluate()))
        losses = np.asarray(res.lossAll, dtype=float)
        per_it = float(np.sum(trials)) / max(1, eng.step)
        print('L-BFGS, %d epochs (%d accepted): loss %.4e -> %.4e, l2Err(cExact) %.5f, %.3f trials per accepted iteration'
              % (len(losses), eng.step, losses[0], losses[-1], err, per_it))
        record('end_to_end_operator_1dt', dict(epochs=int(len(losses)), accepted=int(eng.step), l2Err_cExact=err, bar=CFG1_BAR,
                                               loss_first_last=[float(losses[0]), float(losses[-1])],
                                               trials_per_accepted_iteration=per_it))
        assert np.all(np.diff(losses) <= 0.0)
        assert err <= CFG1_BAR
    finally:
        eng.close()
