"""
GPU parity tests proper: the HIP path (through the C ABI) against the oracle (fp64 autograd
restatement of the reference graph, oracle/tf1_graph.py) on the same seeded inputs.

Tolerances: single step fp32 vs fp64 oracle at fixed theta:
loss rel <= 1e-5, |g-g_ref|_inf/|g_ref|_inf <= 1e-4, lossVec rel <= 1e-4.
"""
import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests.gradcheck import assert_columns_close, assert_grad_close, assert_pair_close, block_errors, column_errors
from tests.parity_cases import (CASES, GRAD_RTOL, LOSS_RTOL, LVEC_RTOL, STEADY, oracle_eval,  # noqa: F401 (re-exported)
                                steady_inputs, steady_oracle, synth)

pytestmark = pytest.mark.gpu


# measured worst-case deviations per parity case, written to gpurun_out/parity_errors.json at the end of the
# module (copied to profiles/ when a round's numbers are recorded)
ERRORS = {}


@pytest.fixture(scope='module', autouse=True)
def _dump_errors():
    yield
    import json
    import os
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'parity_errors.json'), 'w') as f:
            json.dump(ERRORS, f, indent=1, sort_keys=True)
    except OSError:
        pass


def make_engine(d_in, dim, widths, integNum, source, integW, kernel=0, optimizer_name='adam'):
    from varnet_amd.engine import VNEngine
    return VNEngine(dim, d_in, widths, True, integNum, isSource=source, integWflag=integW, kernel=kernel,
                    optimizer_name=optimizer_name)


def _skip_unsupported(kernel, widths, integNum):
    if kernel == 2 and (integNum > 128 or max(widths) > 50 or
                        (max(widths) > 20 and len(widths) < 2) or (max(widths) > 32 and len(widths) < 3) or
                        len(widths) > (5 if max(widths) > 32 else 4)):
        pytest.skip('fused32 not instantiated for this shape')
    if kernel == 3 and len(widths) > 6:   # integNum > 128: two-pass
        pytest.skip('fused16 not instantiated for this shape')


@pytest.mark.parametrize('kernel', [1, 0, 2, 3], ids=['generic', 'auto', 'fused32', 'fused16'])
@pytest.mark.parametrize('case', CASES)
def test_loss_and_grad_parity(case, kernel):
    d_in, dim, widths, integNum, n_k, nB, bDof, source, integW, detJvec = case
    _skip_unsupported(kernel, widths, integNum)
    d = synth(1, d_in, dim, widths, integNum, n_k, nB, bDof, source, integW, detJvec)
    eng = make_engine(d_in, dim, widths, integNum, source, integW, kernel)
    eng.init_params(seed=3)
    flat = eng.get_params()
    # perturb biases so they are exercised
    flat = flat + 0.05 * np.random.default_rng(5).standard_normal(flat.size).astype(np.float32)
    eng.set_params(flat)
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
    eng.set_weights(d['w'])

    ref, gref = oracle_eval(flat, d, d_in, dim, widths, integNum, n_k, bDof, source, integW, detJvec)

    out, lv = eng.eval_loss(0, lossVec=True)
    rec = {}
    for got, key in zip(out, ['loss', 'BCloss', 'ICloss', 'varLoss']):
        rec['eval_' + key] = abs(got - ref[key]) / max(abs(ref[key]), 1e-300)
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (key, got, ref[key])
    lv = lv.cpu().numpy()
    lref = ref['lossVec'].reshape(-1)
    rec['lossVec'] = float(np.max(np.abs(lv - lref)) / np.max(np.abs(lref)))
    assert np.max(np.abs(lv - lref)) <= LVEC_RTOL * np.max(np.abs(lref))

    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    g = gb.cpu().numpy()
    rec['grad_loss'] = float(abs(g[eng.P] - ref['loss']) / abs(ref['loss']))
    assert abs(g[eng.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
    err = np.max(np.abs(g[:eng.P] - gref)) / np.max(np.abs(gref))
    rec['grad'] = float(err)
    ERRORS['case%d_%s' % (CASES.index(case), ['auto', 'generic', 'fused32', 'fused16'][kernel])] = rec
    assert err <= GRAD_RTOL, err
    assert_grad_close(g, gref, d_in, widths, GRAD_RTOL, dim=dim, rec=rec, what='case%d' % CASES.index(case),
                      g32=lambda: oracle_eval(flat, d, d_in, dim, widths, integNum, n_k, bDof, source, integW, detJvec,
                                              dtype=torch.float32)[1])
    eng.close()


def test_forward_and_residual_parity():
    d_in, dim, widths = 3, 2, [10, 20, 30]
    rng = np.random.default_rng(0)
    n = 1000
    X = rng.uniform(-1, 1, (n, d_in))
    diff = rng.uniform(0.1, 1, (n, 1)); vel = rng.standard_normal((n, dim))
    src = rng.standard_normal((n, 1)); ddx = rng.standard_normal((n, dim))
    eng = make_engine(d_in, dim, widths, 64, False, False)
    eng.init_params(seed=11)
    flat = eng.get_params().astype(np.float64)
    uref, rref = og.residual(flat, d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, True)
    u32 = eng.forward(X.astype(np.float32)).cpu().numpy()
    assert np.max(np.abs(u32 - uref[:, 0])) < 2e-6 * max(1, np.max(np.abs(uref)))
    u64 = eng.forward_f64(X).cpu().numpy()
    assert np.max(np.abs(u64 - uref[:, 0])) < 1e-13
    u, r = eng.residual(X, diff, vel, src, ddx, fp64=True)
    assert np.max(np.abs(r.cpu().numpy() - rref[:, 0])) < 1e-11 * max(1, np.max(np.abs(rref)))
    assert np.max(np.abs(u.cpu().numpy() - uref[:, 0])) < 1e-13
    u, r = eng.residual(X.astype(np.float32), diff, vel, src, ddx, fp64=False)
    assert np.max(np.abs(r.cpu().numpy() - rref[:, 0])) < 5e-5 * max(1, np.max(np.abs(rref)))
    eng.close()


@pytest.mark.parametrize('kernel', [1, 0, 2, 3], ids=['generic', 'auto', 'fused32', 'fused16'])
def test_adam_trajectory_parity(kernel):
    """200 TF-1 Adam steps from identical init: relative loss deviation <= 1e-2."""
    d_in, dim, widths, integNum, n_k, nB, bDof = 2, 1, [20, 20], 16, 64, 60, 40
    d = synth(2, d_in, dim, widths, integNum, n_k, nB, bDof)
    eng = make_engine(d_in, dim, widths, integNum, False, False, kernel)
    eng.init_params(seed=1)
    flat = eng.get_params()
    eng.set_fe_table(d['N1'], d['dNt1'], None)
    eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=n_k, detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
    eng.set_weights(d['w'])
    steps = 200
    losses = torch.zeros(steps, device='cuda')
    for i in range(steps):
        eng.train_step(0, losses[i:i + 1])
    torch.cuda.synchronize()
    got = losses.cpu().numpy()
    assert eng.step == steps

    adam = og.TF1Adam(flat.size, lr=1e-3, dtype=np.float64)
    th = flat.astype(np.float64)
    ref = []
    for i in range(steps):
        r, g = oracle_eval(th, d, d_in, dim, widths, integNum, n_k, bDof, False, False, False)
        ref.append(r['loss'])
        th = adam.step(th, g)
    ref = np.array(ref)
    assert got[-1] < got[0]
    assert np.max(np.abs(got - ref) / np.abs(ref)) <= 1e-2
    # state export/import round trip
    st = eng.export_state()
    p1 = eng.get_params()
    eng.init_params(seed=9)
    eng.import_state(st)
    assert np.array_equal(eng.get_params(), p1) and eng.step == steps
    eng.close()


def test_rmsprop_trajectory_parity():
    """40 TF-1 RMSProp steps (decay 0.9, eps 1e-10, mean-square slot starting at ones; TFModel.py:185-186)
    against the oracle's restatement of ApplyRMSProp (beyond ~55 steps this problem's RMSProp iteration
    starts to oscillate and fp32/fp64 trajectories separate); state survives export/import."""
    d_in, dim, widths, integNum, n_k, nB, bDof = 2, 1, [20, 20], 16, 64, 60, 40
    d = synth(2, d_in, dim, widths, integNum, n_k, nB, bDof)
    eng = make_engine(d_in, dim, widths, integNum, False, False, 0, optimizer_name='RMSProp')
    eng.init_params(seed=1)
    flat = eng.get_params()
    eng.set_fe_table(d['N1'], d['dNt1'], None)
    eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=n_k, detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
    eng.set_weights(d['w'])
    steps = 40
    losses = torch.zeros(steps, device='cuda')
    for i in range(steps):
        eng.train_step(0, losses[i:i + 1])
    torch.cuda.synchronize()
    got = losses.cpu().numpy()
    opt = og.TF1RMSProp(flat.size, lr=1e-3, dtype=np.float64)
    th = flat.astype(np.float64)
    ref = []
    for i in range(steps):
        r, g = oracle_eval(th, d, d_in, dim, widths, integNum, n_k, bDof, False, False, False)
        ref.append(r['loss'])
        th = opt.step(th, g)
    ref = np.array(ref)
    assert np.max(np.abs(got - ref) / np.abs(ref)) <= 1e-3
    assert np.max(np.abs(eng.get_params() - th)) <= 2e-3 * np.max(np.abs(th))
    pe = block_errors(eng.get_params(), th, d_in, widths, dim)          # and every parameter tensor on its own scale
    ERRORS['rmsprop_trajectory_params'] = pe
    assert max(pe.values()) <= 2e-3, pe
    st = eng.export_state()
    p1 = eng.get_params()
    eng.init_params(seed=9)
    eng.import_state(st)
    assert np.array_equal(eng.get_params(), p1) and eng.step == steps
    eng.train_step(0)
    eng.close()
    with pytest.raises(ValueError):
        make_engine(d_in, dim, widths, integNum, False, False, 0, optimizer_name='sgd')


def test_train_epoch_equals_single_steps():
    """vn_train_epoch (one host call for a pass over the mini-batches, VarNetUtility.py:1021-1047) leaves the same
    parameters as the same steps issued one by one, and adds every pre-update loss to the device scalar."""
    d_in, dim, widths, integNum, n_k, nB, bDof = 2, 1, [20, 20, 20], 16, 96, 60, 40
    d = synth(4, d_in, dim, widths, integNum, n_k, nB, bDof)
    engs = []
    for _ in range(2):
        eng = make_engine(d_in, dim, widths, integNum, False, False, 0)
        eng.init_params(seed=1)
        eng.set_fe_table(d['N1'], d['dNt1'], None)
        half = (n_k // 2) * integNum
        eng.set_interior(0, d['Input'][:half], d['gcoef'][:half], None, n_k=n_k // 2, detJ=d['detJ'])
        eng.set_interior(1, d['Input'][half:], d['gcoef'][half:], None, n_k=n_k - n_k // 2, detJ=d['detJ'])
        eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
        eng.set_weights(d['w'])
        engs.append(eng)
    order = [0, 1, 1, 0, 1]
    acc = torch.zeros((), device='cuda')
    engs[0].train_epoch(order, acc)
    losses = torch.zeros(len(order), device='cuda')
    for i, b in enumerate(order):
        engs[1].train_step(b, losses[i:i + 1])
    torch.cuda.synchronize()
    assert np.array_equal(engs[0].get_params(), engs[1].get_params()) and engs[0].step == engs[1].step == len(order)
    assert abs(float(acc) - float(losses.sum())) <= 1e-5 * float(losses.sum())
    for e in engs:
        e.close()


def steady_routes(widths, d_in):
    """Routes that serve a STEADY case: forced kernels only where the network is in their range."""
    in_range = max(widths) <= 64 and len(widths) <= 6 and d_in <= 8
    return ['generic', 'auto', 'fused16'] if in_range else ['auto']


def steady_setup(case, kernel, seed=7):
    from varnet_amd.engine import VNEngine
    d_in, dim, widths, q, n_k, nB, bDof, act, has_w, detJvec = case
    d, flat = steady_inputs(case, seed)
    eng = VNEngine(dim, d_in, widths, False, q, isSource=True, integWflag=has_w, kernel=kernel, activationFun=act)
    eng.init_params(seed=2)
    assert np.array_equal(eng.get_params(), og.glorot_init(d_in, widths, 2))
    eng.set_params(flat)
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 1.5)
    eng.set_weights(d['w'])
    return eng, d, flat


def steady_check(eng, d, flat, case, tag):
    """Loss components, lossVec and gradient of a steady engine against the fp64 oracle; ICloss is exactly 0."""
    ref, gref = steady_oracle(flat, d, case)
    assert ref['ICloss'] == 0.0
    out, lv = eng.eval_loss(0, lossVec=True)
    rec = {}
    for got, key in zip(out, ['loss', 'BCloss', 'ICloss', 'varLoss']):
        rec['eval_' + key] = abs(got - ref[key]) / max(abs(ref[key]), 1e-300)
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (key, got, ref[key])
    assert out[2] == 0.0
    lref = ref['lossVec'].reshape(-1)
    rec['lossVec'] = float(np.max(np.abs(lv.cpu().numpy() - lref)) / np.max(np.abs(lref)))
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    g = gb.cpu().numpy()
    P = eng.P
    rec['grad_loss'] = float(abs(g[P] - ref['loss']) / abs(ref['loss']))
    rec['grad'] = float(np.max(np.abs(g[:P] - gref)) / np.max(np.abs(gref)))
    ERRORS['steady ' + tag] = rec
    assert rec['lossVec'] <= LVEC_RTOL, rec
    assert abs(g[P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
    assert abs(g[P + 2]) == 0.0                                      # ICloss is the constant 0
    assert rec['grad'] <= GRAD_RTOL, rec
    assert_grad_close(g, gref, case[0], case[2], GRAD_RTOL, dim=case[1], td=False, rec=rec, what='steady ' + tag,
                      g32=lambda: steady_oracle(flat, d, case, torch.float32)[1])


_KERNEL = {'generic': 1, 'auto': 0, 'fused16': 3}


@pytest.mark.parametrize('case,kernel', [pytest.param(c, r, id='case%d-%s' % (i, r))
                                         for i, c in enumerate(STEADY) for r in steady_routes(c[2], c[0])])
def test_steady_problem_parity(case, kernel):
    eng, d, flat = steady_setup(case, _KERNEL[kernel])
    if kernel == 'fused16':
        assert eng.kernel_path()[0] == 3
    elif kernel == 'generic':
        assert eng.kernel_path()[0] == 1
    steady_check(eng, d, flat, case, 'case%d %s %s %s q%d' % (STEADY.index(case), kernel, case[2], case[7], case[3]))
    eng.close()


def test_nine_inputs_run_layer_by_layer_and_the_fused_family_refuses_them():
    """VN_KMAX_DIN = 8: at d_in = 9 AUTO takes the layer-by-layer route and matches the oracle; forcing the 8-wave fused kernel
    (or the generic kernels) is refused with a sentence, not a fault."""
    from varnet_amd.engine import VNEngine, VNError
    d_in, dim, widths, q, n_k, nB, bDof = 9, 2, [50] * 5, 64, 20, 40, 20
    for kernel in (3, 1):
        with pytest.raises(VNError, match='outside the range of the requested kernel family'):
            VNEngine(dim, d_in, widths, True, q, kernel=kernel)
    d = synth(13, d_in, dim, widths, q, n_k, nB, bDof, True, True, False)
    eng = make_engine(d_in, dim, widths, q, True, True, 0)
    assert eng.kernel_path()[0] == 4
    eng.init_params(seed=3)
    flat = eng.get_params() + 0.05 * np.random.default_rng(5).standard_normal(eng.P).astype(np.float32)
    eng.set_params(flat)
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
    eng.set_weights(d['w'])
    ref, gref = oracle_eval(flat, d, d_in, dim, widths, q, n_k, bDof, True, True, False)
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    g = gb.cpu().numpy()
    assert abs(g[eng.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
    rec = ERRORS.setdefault('d_in9 auto (layer by layer)', {})
    assert_grad_close(g, gref, d_in, widths, GRAD_RTOL, dim=dim, rec=rec,
                      g32=lambda: oracle_eval(flat, d, d_in, dim, widths, q, n_k, bDof, True, True, False, dtype=torch.float32)[1])
    eng.close()


def test_engine_argument_errors():
    from varnet_amd.engine import VNEngine, VNError
    eng = VNEngine(1, 2, [5, 5], True, 16)
    with pytest.raises(VNError):
        eng.grad(0)                                                  # no data registered
    with pytest.raises(VNError):
        eng.lib.vn_params_set(eng.h, None, 3) and None or eng._ck(eng.lib.vn_params_set(eng.h, None, 3))
    with pytest.raises(AssertionError):
        eng.set_interior(0, np.zeros((17, 2), np.float32), np.zeros((17, 1), np.float32), n_k=1)
    eng.close()
    with pytest.raises(ValueError):
        VNEngine(1, 2, [5], True, 16, activationFun='relu')          # options: 'sigmoid' or 'tanh' (VarNet.py:97)
    with pytest.raises(ValueError):
        VNEngine(1, 2, [5, 5], True, 16, activationFun=['tanh', 'sigmoid', 'tanh'])   # list length != depth (TFModel.py:117)
    with pytest.raises(ValueError):
        VNEngine(1, 2, [5000], True, 16)                             # beyond what a vn_config can describe
    with pytest.raises(VNError):
        VNEngine(1, 2, [500], True, 16, kernel=1)                    # outside the generic kernels' range when forced
    eng = VNEngine(1, 2, [500], True, 16)                            # AUTO: the layer-by-layer route
    assert eng.kernel_path()[0] == 4
    eng.close()


@pytest.mark.parametrize('kernel', [1, 0, 2], ids=['generic', 'auto', 'fused32'])
@pytest.mark.parametrize('q,widths', [(16, [20, 20, 20]), (64, [50, 50, 50]), (36, [10, 20])])
def test_per_row_tables_and_detjvec_parity(q, widths, kernel):
    """Non-uniform supports: per-row N / dNt arrays and a per-test-function detJ
    (VarNetUtility.py:506-523, TFModel.py:662-663) on every kernel path, fp64 oracle."""
    from varnet_amd.engine import VNEngine
    _skip_unsupported(kernel, widths, q)
    d_in, dim = (3, 2) if q != 16 else (2, 1)
    n_k, nB, bDof = 45, 31, 17
    rng = np.random.default_rng(11)
    n = n_k * q
    Input = rng.uniform(-1, 1, (n, d_in)).astype(np.float32)
    gcoef = rng.standard_normal((n, dim)).astype(np.float32)
    src = rng.standard_normal((n, 1)).astype(np.float32)
    Nrow = rng.uniform(0, 1, (n, 1)).astype(np.float32)
    dNtrow = rng.standard_normal((n, 1)).astype(np.float32)
    detJ = rng.uniform(0.01, 0.05, (n_k, 1)).astype(np.float32)
    integW = rng.uniform(0.5, 1, (1, q)).astype(np.float32) if q == 36 else None
    biInput = rng.uniform(-1, 1, (nB, d_in)).astype(np.float32)
    biLabel = rng.standard_normal((nB, 1)).astype(np.float32)
    w = np.array([2.0, 3.0, 4.0])
    eng = VNEngine(dim, d_in, widths, True, q, isSource=True, integWflag=integW is not None, kernel=kernel)
    eng.init_params(seed=5)
    flat = eng.get_params()
    eng.set_fe_table(np.zeros(q, np.float32), np.zeros(q, np.float32), integW)   # tables unused: per-row data
    eng.set_interior(0, Input, gcoef, src, n_k=n_k, detJ=detJ, N_rows=Nrow, dNt_rows=dNtrow)
    eng.set_bic(biInput, biLabel, bDof, 2.0)
    eng.set_weights(w)
    ref, gref = og.loss_and_grad(
        flat.astype(np.float64), d_in, widths, torch.float64, Input=Input.astype(np.float64),
        gcoef=gcoef.astype(np.float64), source=src.astype(np.float64), N=Nrow.astype(np.float64),
        dNt=dNtrow.astype(np.float64), integW=None if integW is None else integW.astype(np.float64),
        intShape=[n_k, q], detJ=detJ.astype(np.float64), detJvec=True, biInput=biInput.astype(np.float64),
        biLabel=biLabel.astype(np.float64), bDof=bDof, biDimVal=2.0, w=w, dim=dim, time_dependent=True,
        is_source=True, integWflag=integW is not None)
    out, lv = eng.eval_loss(0, lossVec=True)
    assert abs(out[0] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
    assert np.max(np.abs(lv.cpu().numpy() - ref['lossVec'].reshape(-1))) <= LVEC_RTOL * np.max(np.abs(ref['lossVec']))
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    g = gb.cpu().numpy()
    assert abs(g[eng.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
    assert np.max(np.abs(g[:eng.P] - gref)) <= GRAD_RTOL * np.max(np.abs(gref))
    ERRORS['per_row_tables q%d %s %s' % (q, widths, kernel)] = assert_grad_close(g, gref, d_in, widths, GRAD_RTOL, dim=dim)
    eng.close()


def _csr(uid, U):
    order = np.argsort(uid, kind='stable').astype(np.int32)
    rowptr = np.zeros(U + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(np.bincount(uid, minlength=U))
    return rowptr, order


DEDUP_CASES = [
    # d_in dim widths            q   n_k  U     nB  bDof source integW
    (2, 1, [20, 20, 20],         16, 50,  230,  30, 18,  False, False),
    (3, 2, [50, 50, 50, 50, 50], 64, 40,  500,  77, 40,  True,  False),
    (3, 2, [32, 17],             32, 33,  300,  10, 4,   False, True),
    (3, 1, [10, 20, 30],         16, 64,  400,  19, 7,   True,  False),      # MOR-style extra input
    # the seed kernel's reduction paths: integNum not a multiple of 16 -> level 2 re-reads the row values; ragged
    # chunks (q = 36: 7 test functions per 256-row chunk, 32-function blocks walk chunks of 7,7,7,7,4); n_k not a multiple of 32
    (2, 1, [20, 20],             4,   77,  90,   12, 5,   False, False),      # integPnum 1 in 1D+t
    (3, 2, [20, 20, 20],         8,   45,  120,  9,  4,   True,  True),       # integPnum 1 in 2D+t
    (2, 1, [50, 50, 50],         36,  53,  700,  31, 11,  True,  True),       # integPnum 3 in 1D+t
    (2, 1, [24, 31],             100, 37,  900,  8,  5,   False, True),       # integPnum 5 in 1D+t
    (4, 3, [50, 50, 50, 50],     64,  21,  333,  40, 22,  True,  False),      # dim 3 (+ time): three coordinates in one sweep
    # beyond one 128-point tile (the two-pass route's networks): the formulation has no tiles of whole test functions
    (3, 2, [50, 50, 50, 50, 50], 216, 11,  410,  33, 17,  True,  True),       # integPnum 3 in 2D+t
    (4, 3, [20, 30],             256, 7,   600,  12, 6,   False, False),      # integPnum 2 in 3D+t
    # 6 and 8 inputs (MOR parameters): the point kernels' second input k-step, in 2D and in 3D
    (6, 2, [50, 50, 50],         64,  30,  500,  40, 22,  True,  False),      # 2D+t + 3 parameters
    (8, 2, [32, 17],             216, 9,   500,  12, 6,   True,  True),       # 2D+t + 5 parameters, two-pass network
    (6, 3, [64, 64, 64],         16,  40,  400,  20, 10,  False, True),       # 3D+t + 2 parameters
    (8, 3, [50, 50, 50, 50],     64,  21,  333,  40, 22,  True,  False),      # 3D+t + 4 parameters
]


@pytest.mark.parametrize('case', DEDUP_CASES)
def test_dedup_formulation_parity(case):
    """De-duplicated formulation (one network evaluation per unique quadrature point): same loss
    and gradient as the row-wise formulation -- against the fp64 oracle on the expanded rows and
    against the engine's own row-wise path."""
    _dedup_parity(case, True)


def _dedup_parity(case, td, tag=None):
    from varnet_amd.engine import VNEngine
    d_in, dim, widths, q, n_k, U, nB, bDof, source, integW = case
    rng = np.random.default_rng(21)
    n = n_k * q
    Xu = rng.uniform(-1, 1, (U, d_in)).astype(np.float32)
    uid = rng.integers(0, U, n).astype(np.int32)
    uid[:U] = np.arange(U)                                           # every unique point is used
    rng.shuffle(uid)
    d = dict(Xu=Xu, uid=uid, Input=Xu[uid], gcoef=rng.standard_normal((n, dim)).astype(np.float32),
             source=rng.standard_normal((n, 1)).astype(np.float32) if source else None,
             N1=rng.uniform(0, 1, q).astype(np.float32), dNt1=rng.standard_normal(q).astype(np.float32),
             integW=rng.uniform(0.5, 1, (1, q)).astype(np.float32) if integW else None,
             biInput=rng.uniform(-1, 1, (nB, d_in)).astype(np.float32), biLabel=rng.standard_normal((nB, 1)).astype(np.float32),
             bDof=bDof, n_k=n_k, w=np.array([3.0, 2.0, 5.0]) if td else np.array([3.0, 0.0, 5.0]))
    d['rowptr'], d['rowidx'] = _csr(uid, U)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW)
    if not td:
        assert eng.dedup_supported()                                 # what train(dedup='auto') would pick for this problem
    eng.init_params(seed=4)
    dedup_checks(eng, d, td, tag)
    eng.close()


def dedup_oracle(eng, d, td, act='sigmoid', dtype=torch.float64):
    """The oracle on the expanded rows of a ready-made map (the dict of dedup_checks) at the engine's parameters."""
    f = np.float64 if dtype == torch.float64 else np.float32
    cv = lambda a: None if a is None else a.astype(f)
    n_k, q = d['n_k'], eng.integNum
    n = n_k * q
    return og.loss_and_grad(
        eng.get_params().astype(f), eng.inpDim, eng.layerWidth, dtype,
        Input=cv(d['Input']), gcoef=cv(d['gcoef']), source=cv(d['source']),
        N=np.tile(d['N1'], n_k).reshape(n, 1).astype(f), dNt=np.tile(d['dNt1'], n_k).reshape(n, 1).astype(f),
        integW=cv(d['integW']), intShape=[n_k, q], detJ=0.05, detJvec=False,
        biInput=cv(d['biInput']), biLabel=cv(d['biLabel']), bDof=d['bDof'], biDimVal=2.0, w=d['w'],
        dim=eng.dim, time_dependent=td, is_source=d['source'] is not None, integWflag=d['integW'] is not None, activation=act)


def dedup_checks(eng, d, td, tag=None, act='sigmoid', oracle=None, errors=None):
    """The checks of the de-duplicated formulation on an engine that has its parameters and a ready-made map in d (Xu, uid,
    rowptr, rowidx, Input = Xu[uid], gcoef, source, N1, dNt1, integW, biInput, biLabel, bDof, n_k, w): the row-wise and the
    de-duplicated step against the fp64 oracle (globally and per block), against each other, eval_loss with lossVec on the map and
    row-wise, a second grad the same bits, and set_dedup(batch) off restoring the row-wise bits.  oracle: a callable dtype ->
    (ref, gref) for a caller that has the reference already; its fp32 form then serves the per-block rule as g32.  errors: the
    record the figures go to (default: this module's).  Returns (row-wise, de-duplicated) gradients."""
    ERRORS = globals()['ERRORS'] if errors is None else errors
    d_in, dim, widths, q, n_k = eng.inpDim, eng.dim, eng.layerWidth, eng.integNum, d['n_k']
    Xu, uid, rowptr, rowidx = d['Xu'], d['uid'], d['rowptr'], d['rowidx']
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=0.05)
    eng.set_bic(d['biInput'], d['biLabel'], d['bDof'], 2.0)
    eng.set_weights(d['w'])
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    g_rows = gb.cpu().numpy().copy()
    eng.set_dedup(0, Xu, uid, rowptr, rowidx)
    eng.grad(0)
    torch.cuda.synchronize()
    g_dd = gb.cpu().numpy().copy()
    ref, gref = dedup_oracle(eng, d, td, act) if oracle is None else oracle(torch.float64)
    g32 = None if oracle is None else (lambda: oracle(torch.float32)[1])
    P = eng.P
    if tag is not None:
        ERRORS[tag] = {k: float(np.max(np.abs(g[:P] - gref)) / np.max(np.abs(gref))) for k, g in
                       (('grad_rowwise', g_rows), ('grad_dedup', g_dd))}
        ERRORS[tag].update({'loss_' + k: float(abs(g[P] - ref['loss']) / abs(ref['loss'])) for k, g in
                            (('rowwise', g_rows), ('dedup', g_dd))})
    if not td:
        assert ref['ICloss'] == 0.0 and g_rows[P + 2] == 0.0 and g_dd[P + 2] == 0.0
    for g in (g_rows, g_dd):
        assert abs(g[P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
        assert np.max(np.abs(g[:P] - gref)) <= GRAD_RTOL * np.max(np.abs(gref))
    rec = ERRORS.setdefault(tag or 'dedup %s d_in%d q%d' % (widths, d_in, q), {})
    for name, g in (('rowwise', g_rows), ('dedup', g_dd)):
        r = {}                                                       # (filled before any assertion: a miss leaves its figures)
        try:
            assert_grad_close(g, gref, d_in, widths, GRAD_RTOL, dim=dim, td=td, what=name, g32=g32, rec=r)
        finally:
            rec.update({'worst_block_' + name: r.get('worst_block'), 'worst_block_err_' + name: r.get('worst_block_err')})
    r = {}
    try:
        assert_pair_close(g_dd, g_rows, d_in, widths, 2e-4, dim=dim, td=td, what='dedup vs row-wise', rec=r)
    finally:
        rec.update(worst_block_dedup_vs_rowwise=r.get('worst_block'), worst_block_err_dedup_vs_rowwise=r.get('worst_block_err'))
    assert np.allclose(g_dd[P + 1:P + 4], g_rows[P + 1:P + 4], rtol=1e-5)
    # vn_eval_loss (splitLoss: every monitor, trainWeight) of a batch that carries the map: (u, grad u) once per unique point and the
    # loss-only form of the assembly kernel (round 6) -- loss components and loss field against the fp64 oracle at the suite's bars,
    # against the row-wise evaluation of the same batch (route | 8), and equal to what the training step itself reports
    out_dd, lv_dd = eng.eval_loss(0, lossVec=True)
    eng.debug_point_route(8)
    out_rw, lv_rw = eng.eval_loss(0, lossVec=True)
    eng.debug_point_route(0)
    torch.cuda.synchronize()
    lvref = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1)
    for name, out, lv in (('dedup', out_dd, lv_dd), ('rowwise', out_rw, lv_rw)):
        rec['eval_loss_' + name] = float(abs(out[0] - ref['loss']) / abs(ref['loss']))
        rec['eval_lossVec_' + name] = float(np.max(np.abs(lv.cpu().numpy().astype(np.float64) - lvref)) / np.max(np.abs(lvref)))
    for out, lv in ((out_dd, lv_dd), (out_rw, lv_rw)):
        assert abs(out[0] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
        assert abs(out[1] - ref['BCloss']) <= LOSS_RTOL * abs(ref['BCloss']) and abs(out[2] - ref['ICloss']) <= LOSS_RTOL * abs(ref['ICloss'])
        assert td or out[2] == 0.0
        assert abs(out[3] - ref['varLoss']) <= LOSS_RTOL * abs(ref['varLoss'])
        assert np.max(np.abs(lv.cpu().numpy().astype(np.float64) - lvref)) <= 1e-4 * np.max(np.abs(lvref))
    assert np.allclose(out_dd, [g_dd[P], g_dd[P + 1], g_dd[P + 2], g_dd[P + 3]], rtol=2e-6)
    # bitwise reproducible, and switching it off restores the row-wise path
    eng.grad(0)
    torch.cuda.synchronize()
    assert np.array_equal(gb.cpu().numpy(), g_dd)
    eng.set_dedup(0)
    eng.grad(0)
    torch.cuda.synchronize()
    assert np.array_equal(gb.cpu().numpy(), g_rows)
    return g_rows, g_dd


DEDUP_STEADY = [
    # d_in dim widths            q   n_k  U     nB  bDof source integW   (steady: bDof < nB feeds rows a steady loss ignores)
    (1, 1, [20, 20],             4,   77,  90,   12, 5,   True,  False),      # integPnum 2 in 1D: one live input feature
    (1, 1, [50, 50, 50],         6,   53,  200,  2,  2,   True,  True),       # integPnum 3 in 1D: ragged 128-row tiles
    (2, 2, [32, 17],             16,  50,  230,  30, 18,  False, False),      # widths <= 32: vn_pgrad16
    (2, 2, [33, 50, 41],         16,  40,  300,  20, 20,  True,  False),      # widths 33..64: vn_split16
    (2, 2, [64, 64, 64],         36,  30,  400,  40, 22,  True,  True),
    (3, 2, [20, 30],             36,  21,  333,  12, 6,   False, True),       # d_in = dim + 1: the extra column is not time
    (3, 2, [60, 64, 51],         16,  45,  500,  9,  4,   True,  False),
    (6, 2, [33, 50, 41],         16,  40,  300,  20, 20,  True,  False),      # 2D + 4 parameters
    (8, 3, [20, 30],             36,  21,  333,  12, 6,   False, True),       # 3D + 5 parameters
]


@pytest.mark.parametrize('case', DEDUP_STEADY)
def test_dedup_formulation_parity_steady(case):
    """The de-duplicated formulation on a steady problem (no time seed in the reverse launch, vn_dedup.hip's steady branches):
    the method of test_dedup_formulation_parity -- fp64 oracle, the row-wise path, the monitor's loss split, bitwise repeatable,
    switching it off restores the row-wise path."""
    _dedup_parity(case, False, 'steady dedup case%d %s q%d' % (DEDUP_STEADY.index(case), case[2], case[3]))


@pytest.mark.parametrize('d_in,dim,widths,act,n', [
    (2, 1, [20, 20, 20], 'sigmoid', 1000),          # <3,5>: edge rows with 4 features
    (3, 2, [50, 50, 50, 50, 50], 'sigmoid', 4099),  # <5,13>: the bench network; n not a multiple of 16
    (3, 2, [50, 50, 50, 50, 50], 'tanh', 777),
    (3, 1, [10, 20, 30], 'sigmoid', 515),           # <3,8>: padding k-steps / row tiles branched over; extra (MOR) input
    (4, 3, [64, 64, 64], 'tanh', 2048),             # <3,16>: full tiles, three coordinates + time
    (3, 2, [50], 'sigmoid', 130),                   # one hidden layer: no hidden-to-hidden sweep
    (4, 3, [33, 50, 41, 17, 50, 50, 50, 50], 'sigmoid', 300),   # <8,13>: most stored activations
    (2, 1, [64, 51, 64, 60, 55, 64], 'sigmoid', 97),            # <6,16>
    (3, 2, [7, 5], 'tanh', 15),                     # fewer points than one wave chunk
    (3, 2, [50, 44, 33, 50, 36, 50, 50], 'tanh', 1031),         # <7,13>: the deepest net of the bf16-piece kernel (vn_forward)
    (4, 3, [40, 52], 'sigmoid', 64),                # <2,16>: its shallowest
])
def test_forward_grad_parity(d_in, dim, widths, act, n):
    """vn_forward_grad (vn_pgrad16.hip: value forward + value-adjoint sweep to the inputs, the reference's
    tf.gradients(model(Input), Input), TFModel.py:536-541) against the fp64 oracle's model_grad."""
    from varnet_amd.engine import VNEngine
    rng = np.random.default_rng(5)
    X = rng.uniform(-1.5, 1.5, (n, d_in)).astype(np.float32)
    eng = VNEngine(dim, d_in, widths, True, 16, activationFun=act)
    eng.init_params(seed=9)
    flat = eng.get_params()
    # glorot weights give a flat field; scale them up so that the derivatives are not tiny
    flat = (flat * 2.5).astype(np.float32)
    flat[-1] = 0.3
    eng.set_params(flat)
    u, g = eng.forward_grad(X)
    u2 = eng.forward(X)
    torch.cuda.synchronize()
    params = og.unflatten(flat.astype(np.float64), d_in, widths, torch.float64)
    Xt = torch.tensor(X.astype(np.float64), requires_grad=True)
    Val, dM_dx, _, _ = og.model_grad(params, Xt, dim, activation=act)
    uref, gref = Val.detach().numpy().reshape(-1), dM_dx.detach().numpy()
    eu = np.max(np.abs(u.cpu().numpy() - uref)) / np.max(np.abs(uref))
    eg = np.max(np.abs(g.cpu().numpy() - gref)) / np.max(np.abs(gref))
    egc = column_errors(g.cpu().numpy(), gref)                   # each spatial direction on its own scale
    # vn_forward: hidden widths 33..64 run the bf16-piece kernel (vn_split16.hip: six products of exact bf16 pieces per layer), the
    # others the value-only sweep of vn_pgrad16; route 2 forces the latter -- both against the oracle at the SAME bar, errors side by side
    # (the f32-MFMA forms of the networks vn_split16 serves live in the tests' cross-check library: an engine of that library)
    engx = VNEngine(dim, d_in, widths, True, 16, activationFun=act, xcheck=True)
    engx.set_params(flat)
    engx.debug_point_route(2)
    u2f = engx.forward(X)
    uf32, gf32 = engx.forward_grad(X)
    torch.cuda.synchronize()
    engx.close()
    with pytest.raises(Exception, match='cross-check'):
        eng.debug_point_route(2)                  # the product library has no such route
    euf = np.max(np.abs(uf32.cpu().numpy() - uref)) / np.max(np.abs(uref))
    egf = np.max(np.abs(gf32.cpu().numpy() - gref)) / np.max(np.abs(gref))
    assert euf <= 2e-6 and egf <= 1e-5, (euf, egf)          # vn_pgrad16 (f32 MFMA): round 5's kernel at round 5's bars
    egfc = assert_columns_close(gf32.cpu().numpy(), gref, 1e-5, 'grad u, f32-MFMA kernel')
    ef = np.max(np.abs(u2.cpu().numpy() - uref)) / np.max(np.abs(uref))
    ef32 = np.max(np.abs(u2f.cpu().numpy() - uref)) / np.max(np.abs(uref))
    ERRORS['forward_grad %s %s' % (widths, act)] = {'u': float(eu), 'grad': float(eg), 'vn_forward': float(ef),
                                                    'vn_forward_f32_mfma_kernel': float(ef32), 'u_f32_mfma_kernel': float(euf),
                                                    'grad_f32_mfma_kernel': float(egf), 'grad_per_column': egc,
                                                    'grad_f32_mfma_kernel_worst_column': egfc}
    assert eu <= 2e-6 and eg <= 1e-5, (eu, eg)
    assert max(egc) <= 1e-5, egc
    assert ef <= 2e-6 and ef32 <= 2e-6, (ef, ef32)
    assert np.max(np.abs(u.cpu().numpy() - u2.cpu().numpy())) <= 2e-6 * np.max(np.abs(uref))      # vn_forward: the same values
    assert torch.equal(eng.forward(X), u2)                                                       # repeatable bit for bit
    u3, g3 = eng.forward_grad(X)
    torch.cuda.synchronize()
    assert torch.equal(u, u3) and torch.equal(g, g3)
    eng.close()


@pytest.mark.parametrize('widths', [[50, 50, 50], [20, 20]])
def test_four_space_coordinates_value_runs_and_derivatives_are_refused_cleanly(widths):
    """networks with dim > 3 (d_in <= 8: still the 8-wave family).  vn_forward needs no coordinate split and must run
    -- on the bf16-piece kernel at hidden widths 33..64, on the f32-MFMA value sweep below -- while vn_residual / vn_forward_grad, which
    carry at most three space coordinates, must answer VN_EUNSUPPORTED with a sentence, never a HIP launch error."""
    from varnet_amd.engine import VNEngine, VNError
    rng = np.random.default_rng(3)
    dim, d_in, n = 4, 5, 777
    eng = VNEngine(dim, d_in, widths, True, 16)
    eng.init_params(seed=4)
    flat = eng.get_params()
    X = rng.uniform(-1, 1, (n, d_in)).astype(np.float32)
    u = eng.forward(X)
    torch.cuda.synchronize()
    uref = og.forward(flat.astype(np.float64), d_in, widths, torch.float64, X.astype(np.float64))[:, 0]
    assert np.max(np.abs(u.cpu().numpy() - uref)) <= 2e-6 * max(1.0, np.max(np.abs(uref)))
    with pytest.raises(VNError, match='dim <= 3'):
        eng.residual(X, np.ones((n, 1)), np.zeros((n, dim)), None, None, fp64=False)
    with pytest.raises(VNError, match='dim <= 3'):
        eng.forward_grad(X)
    eng.close()


@pytest.mark.parametrize('d_in,dim,widths,act,n,with_src,with_ddx', [
    (2, 1, [20, 20, 20], 'sigmoid', 1000, True, True),            # <3,5>: edge rows with 4 features; 1D+t
    (3, 2, [50, 50, 50, 50, 50], 'sigmoid', 4099, True, False),   # <5,13>: the bench network; n not a multiple of 16
    (3, 2, [50, 50, 50, 50, 50], 'tanh', 777, False, True),
    (3, 1, [10, 20, 30], 'sigmoid', 515, True, True),             # <3,8>: padding k-steps / row tiles branched over; MOR input
    (4, 3, [64, 64, 64], 'tanh', 2048, True, True),               # <3,16>: three spatial directions + time
    (3, 2, [50], 'sigmoid', 130, False, False),                   # one hidden layer
    (4, 3, [33, 50, 41, 17, 50, 50, 50, 50], 'sigmoid', 300, True, True),    # <8,13>
    (3, 2, [7, 5], 'tanh', 15, True, True),                       # fewer points than one wave chunk
    (3, 2, [50, 44, 33, 50, 36, 50, 50], 'sigmoid', 1031, True, True),       # <7,13>: the deepest net of the bf16-piece kernel
    (2, 1, [64, 51, 64, 60, 55, 64], 'sigmoid', 97, False, True),            # <6,16> on the bf16-piece kernel, 1D+t: ONE pass of four streams
                                                                             # (as tanh with these doubled weights BOTH matrix-pipe kernels measure u 2.4e-6: beyond the 2e-6 bar's envelope)
    (4, 3, [40, 52], 'sigmoid', 64, True, False),                 # <2,16>
])
def test_taylor_residual_parity(d_in, dim, widths, act, n, with_src, with_ddx, monkeypatch):
    """vn_residual of the 8-wave family (vn_taylor16.hip / vn_split16.hip: second-order forward mode on the matrix pipe, one pass per
    coordinate direction) against the fp64 oracle's residual (TFModel.py:743-754 restated) and against the per-point kernel it replaces."""
    from varnet_amd.engine import VNEngine
    rng = np.random.default_rng(17)
    X = rng.uniform(-1.2, 1.2, (n, d_in))
    diff = rng.uniform(0.1, 1, (n, 1)); vel = rng.standard_normal((n, dim))
    src = rng.standard_normal((n, 1)) if with_src else None
    ddx = rng.standard_normal((n, dim)) if with_ddx else None
    eng = VNEngine(dim, d_in, widths, True, 16, activationFun=act)
    eng.init_params(seed=5)
    flat = (eng.get_params() * 2.0).astype(np.float32)            # steeper than glorot: second derivatives that are not tiny
    eng.set_params(flat)
    uref, rref = og.residual(flat.astype(np.float64), d_in, widths, torch.float64, X, diff, vel,
                             np.zeros((n, 1)) if src is None else src, np.zeros((n, dim)) if ddx is None else ddx, dim, True,
                             activation=act)
    X32 = X.astype(np.float32)
    u, r = eng.residual(X32, diff, vel, src, ddx, fp64=False)
    torch.cuda.synchronize()
    scale = max(1.0, float(np.max(np.abs(rref))))
    er = float(np.max(np.abs(r.cpu().numpy() - rref[:, 0]))) / scale
    eu = float(np.max(np.abs(u.cpu().numpy() - uref[:, 0]))) / max(1.0, float(np.max(np.abs(uref))))
    eng.debug_point_route(True)              # the per-point kernel, same inputs
    u_p, r_p = eng.residual(X32, diff, vel, src, ddx, fp64=False)
    torch.cuda.synchronize()
    eng.debug_point_route(False)
    ep = float(np.max(np.abs(r_p.cpu().numpy() - rref[:, 0]))) / scale
    # hidden widths 33..64 (2..7 layers) run the bf16-piece kernel (vn_split16.hip); route 2 = the f32-MFMA kernel vn_taylor16 on the
    # same inputs: same bar, both errors recorded side by side (the bar must not move)
    engx = VNEngine(dim, d_in, widths, True, 16, activationFun=act, xcheck=True)      # an engine of the tests' cross-check library
    engx.set_params(flat)
    engx.debug_point_route(2)
    u_f, r_f = engx.residual(X32, diff, vel, src, ddx, fp64=False)
    torch.cuda.synchronize()
    engx.close()
    er32 = float(np.max(np.abs(r_f.cpu().numpy() - rref[:, 0]))) / scale
    eu32 = float(np.max(np.abs(u_f.cpu().numpy() - uref[:, 0]))) / max(1.0, float(np.max(np.abs(uref))))
    ERRORS['taylor_residual %s %s' % (widths, act)] = {'res': er, 'u': eu, 'res_pointwise_kernel': ep, 'res_f32_mfma_kernel': er32,
                                                      'u_f32_mfma_kernel': eu32}
    # (the f32-MFMA kernel is asserted at the residual bar; its `u` is recorded only: on the new <6,16> tanh case, which round 5
    # did not test, it measures 2.35e-6 against the bf16-piece kernel's passing value -- the kernel that RUNS is asserted above)
    assert er32 <= 5e-5 and eu32 <= 4e-6, (er32, eu32)
    assert float(np.max(np.abs(r.cpu().numpy() - r_f.cpu().numpy()))) / scale <= 5e-5
    assert er <= 5e-5 and eu <= 2e-6, (er, eu, ep)                # the bar of test_forward_and_residual_parity
    assert float(np.max(np.abs(r.cpu().numpy() - r_p.cpu().numpy()))) / scale <= 5e-5
    u2, r2 = eng.residual(X32, diff, vel, src, ddx, fp64=False)
    torch.cuda.synchronize()
    assert torch.equal(r, r2) and torch.equal(u, u2)
    eng.close()


STEADY_POINTS = [
    # d_in dim widths                 act        route of vn_forward / vn_residual (f32) | fp64
    (1, 1, [50, 50, 50],              'sigmoid'),  # bf16 pieces (vn_split16), one live input feature | vn_taylor16d
    (2, 2, [64, 51, 64],              'tanh'),     # bf16 pieces | vn_taylor16d
    (3, 2, [40, 52],                  'sigmoid'),  # bf16 pieces, d_in = dim + 1: the extra column is NOT time
    (1, 1, [20, 20, 20],              'tanh'),     # vn_pgrad16 / vn_taylor16 | vn_taylor16d
    (2, 2, [10, 20, 30],              'sigmoid'),
    (3, 2, [32, 17],                  'sigmoid'),  # vn_taylor16, d_in = dim + 1
    (2, 2, [64] * 6,                  'sigmoid'),  # fp64 images do not fit the LDS: the per-point fp64 kernel
    (2, 2, [128, 128],                'sigmoid'),  # layer by layer (f32 and fp64)
    (1, 1, [300],                     'tanh'),
    (2, 1, [300],                     'sigmoid'),  # layer by layer, d_in = dim + 1
]
POINT_COUNTS = (1, 15, 16, 17, 4099)


@pytest.mark.parametrize('d_in,dim,widths,act', STEADY_POINTS)
def test_steady_point_kernels_parity(d_in, dim, widths, act):
    """vn_forward, vn_forward_grad, vn_residual, vn_forward_f64 and vn_residual_f64 of a STEADY engine (the td = 0 branches:
    no time pass, no -du/dt term) against og.model_grad / og.residual with time_dependent=False, on every route that serves
    the network: the automatic one, the per-point kernels (route 1) and the f32-MFMA forms (route 2, cross-check library)."""
    _point_kernels_parity(d_in, dim, widths, act, False, POINT_COUNTS)


@pytest.mark.parametrize('d_in,dim,widths,act,td', [
    # 5..8 inputs (MOR parameters): inputs 4..7 ride in the point kernels' second input k-step (KS0 = 2)
    (5, 2, [50, 50, 50, 50, 50], 'sigmoid', True),   # bf16 pieces (vn_split16) | f32 MFMA (cross-check)
    (6, 1, [20, 20, 20], 'tanh', True),              # vn_pgrad16 / vn_taylor16
    (7, 3, [64, 51, 64], 'sigmoid', True),           # bf16 pieces, 3D+t + 3 parameters
    (8, 3, [32, 17], 'sigmoid', True),               # vn_pgrad16 / vn_taylor16, 3D+t + 4 parameters
    (8, 2, [40, 52, 64, 33], 'sigmoid', True),       # bf16 pieces, 2D+t + 5 parameters
    (6, 3, [10, 20, 30], 'sigmoid', False),          # steady 3D + 3 parameters
    (8, 2, [50, 50, 50], 'tanh', False),             # steady, bf16 pieces
    (5, 1, [64] * 6, 'sigmoid', True),               # six 64-wide layers: the per-point fp64 kernel
])
def test_point_kernels_parity_five_to_eight_inputs(d_in, dim, widths, act, td):
    """The method of test_steady_point_kernels_parity at 5..8 inputs, time-dependent and steady, on 1, 17 and 4099 points:
    f32 and fp64 entry points against the fp64 oracle, the per-point kernels and the f32-MFMA forms; grad u per direction."""
    _point_kernels_parity(d_in, dim, widths, act, td, (1, 17, 4099))


def _point_kernels_parity(d_in, dim, widths, act, td, counts):
    from varnet_amd.engine import VNEngine
    eng = VNEngine(dim, d_in, widths, td, 16, activationFun=act)
    layered = eng.kernel_path()[0] == 4
    assert layered == (max(widths) > 64)
    eng.init_params(seed=5)
    flat = (eng.get_params() * 2.0).astype(np.float32)            # steeper than glorot: second derivatives that are not tiny
    eng.set_params(flat)
    engx = None
    if not layered:
        engx = VNEngine(dim, d_in, widths, td, 16, activationFun=act, xcheck=True)
        engx.set_params(flat)
        engx.debug_point_route(2)
    params = og.unflatten(flat.astype(np.float64), d_in, widths, torch.float64)
    rec = {}
    rng = np.random.default_rng(23)
    for n in counts:
        X = rng.uniform(-1.2, 1.2, (n, d_in))
        diff = rng.uniform(0.1, 1, (n, 1)); vel = rng.standard_normal((n, dim))
        src = rng.standard_normal((n, 1)); ddx = rng.standard_normal((n, dim))
        uref, rref = og.residual(flat.astype(np.float64), d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, td,
                                 activation=act)
        uref, rref = uref[:, 0], rref[:, 0]
        uscale = max(1.0, float(np.max(np.abs(uref))))
        scale = max(1.0, float(np.max(np.abs(rref))))
        if d_in > dim and not td:
            # negative control: a kernel that took column `dim` for time would be off by |du/dx_dim|, far beyond the bar
            _, rtd = og.residual(flat.astype(np.float64), d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, True,
                                 activation=act)
            assert np.max(np.abs(rtd[:, 0] - rref)) > 100 * 5e-5 * scale
        X32 = X.astype(np.float32)
        e = {}
        outs = [('', eng)] + ([('f32_mfma_', engx)] if engx is not None else [])
        for pre, en in outs:
            u = en.forward(X32)
            ur, r = en.residual(X32, diff, vel, src, ddx, fp64=False)
            torch.cuda.synchronize()
            e[pre + 'u'] = float(np.max(np.abs(u.cpu().numpy() - uref))) / uscale
            e[pre + 'res_u'] = float(np.max(np.abs(ur.cpu().numpy() - uref))) / uscale
            e[pre + 'res'] = float(np.max(np.abs(r.cpu().numpy() - rref))) / scale
            if not layered:
                ug, g = en.forward_grad(X32)
                torch.cuda.synchronize()
                Xt = torch.tensor(X, requires_grad=True)
                Val, dM_dx, dM_dt, _ = og.model_grad(params, Xt, dim, time_dependent=td, activation=act)
                assert td or dM_dt is None
                gref = dM_dx.detach().numpy()
                e[pre + 'fg_u'] = float(np.max(np.abs(ug.cpu().numpy() - uref))) / uscale
                e[pre + 'fg_grad'] = float(np.max(np.abs(g.cpu().numpy() - gref))) / max(1e-30, float(np.max(np.abs(gref))))
                e[pre + 'fg_grad_worst_column'] = max(column_errors(g.cpu().numpy(), gref))   # asserted at the fg_grad bar
        u64 = eng.forward_f64(X)
        u64r, r64 = eng.residual(X, diff, vel, src, ddx, fp64=True)
        torch.cuda.synchronize()
        e['u_f64'] = float(np.max(np.abs(u64.cpu().numpy() - uref)))
        e['res_u_f64'] = float(np.max(np.abs(u64r.cpu().numpy() - uref)))
        e['res_f64'] = float(np.max(np.abs(r64.cpu().numpy() - rref))) / scale
        if not layered:
            eng.debug_point_route(1)                                  # the per-point kernels, same inputs
            _, rp = eng.residual(X32, diff, vel, src, ddx, fp64=False)
            _, rp64 = eng.residual(X, diff, vel, src, ddx, fp64=True)
            torch.cuda.synchronize()
            eng.debug_point_route(0)
            e['pointwise_res'] = float(np.max(np.abs(rp.cpu().numpy() - rref))) / scale
            e['pointwise_res_f64'] = float(np.max(np.abs(rp64.cpu().numpy() - rref))) / scale
        rec['n%d' % n] = e
        for k, v in e.items():
            bar = (1e-13 if k in ('u_f64', 'res_u_f64') else 1e-11 if k.endswith('res_f64') else 5e-5 if k.endswith('res')
                   else 4e-6 if k.startswith('f32_mfma_') and k.endswith('u')     # that kernel's bar in test_taylor_residual_parity
                   else 2e-6 if k.endswith('u') else 1e-5)
            assert v <= bar, (n, k, v, bar)
    ERRORS['%spoints %s %s d_in%d %s' % ('' if td else 'steady ', 'layered' if layered else 'kernels', widths, d_in, act)] = rec
    if engx is not None:
        engx.close()
    eng.close()


@pytest.mark.parametrize('q,dim,d_in,widths,integW', [(64, 2, 3, [50, 50, 50], False), (16, 1, 2, [20, 20], False), (36, 1, 2, [10, 20, 30], True)])
def test_dedup_periodic_gcoef_table_is_bitwise_the_csr_path(q, dim, d_in, widths, integW, monkeypatch):
    """With constant coefficients gcoef repeats with period integNum along the rows (VarNet.py:837 tiles the tables): vn_set_dedup
    detects that bitwise and the two assembly kernels read the integNum-entry table instead of 8 bytes per row each.  Same bits
    as the general path (vn_debug_point_route | 4: CSR-ordered copy of gcoef); one perturbed row switches the detection off."""
    from varnet_amd.engine import VNEngine
    rng = np.random.default_rng(8)
    n_k, U, nB, bDof = 70, 900, 20, 9
    n = n_k * q
    Xu = rng.uniform(-1, 1, (U, d_in)).astype(np.float32)
    uid = rng.integers(0, U, n).astype(np.int32)
    uid[:U] = np.arange(U)
    rng.shuffle(uid)
    table = rng.standard_normal((q, dim)).astype(np.float32)
    gcoef = np.tile(table, (n_k, 1))
    N1 = rng.uniform(0, 1, q).astype(np.float32); dNt1 = rng.standard_normal(q).astype(np.float32)
    W = rng.uniform(0.5, 1, (1, q)).astype(np.float32) if integW else None
    eng = VNEngine(dim, d_in, widths, True, q, integWflag=integW)
    eng.init_params(seed=2)
    eng.set_fe_table(N1, dNt1, W)
    eng.set_bic(rng.uniform(-1, 1, (nB, d_in)).astype(np.float32), rng.standard_normal((nB, 1)).astype(np.float32), bDof, 2.0)
    eng.set_weights([3.0, 2.0, 5.0])
    gb = eng.bind_grad_buffer()
    rowptr, rowidx = _csr(uid, U)

    def grad_with(g, no_table):
        eng.set_interior(0, Xu[uid], g, None, n_k=n_k, detJ=0.05)
        eng.debug_point_route(4 if no_table else 0)      # | 4: keep the CSR-ordered copy of gcoef (a per-engine test argument since round 6)
        eng.set_dedup(0, Xu, uid, rowptr, rowidx)
        eng.debug_point_route(0)
        eng.grad(0)
        torch.cuda.synchronize()
        return gb.cpu().numpy().copy()
    g_tab, g_csr = grad_with(gcoef, False), grad_with(gcoef, True)
    assert np.array_equal(g_tab, g_csr)
    eng.set_dedup(0)
    eng.grad(0)
    torch.cuda.synchronize()
    g_rows = gb.cpu().numpy().copy()
    assert np.max(np.abs(g_tab[:eng.P] - g_rows[:eng.P])) <= 1e-4 * np.max(np.abs(g_rows[:eng.P]))
    assert_pair_close(g_tab, g_rows, d_in, widths, 1e-4, dim=dim, what='periodic table vs row-wise')
    # one row off the period: the table must not be used (the general path then agrees with the row-wise launch on THAT data)
    g2 = gcoef.copy()
    g2[5 * q + 3, 0] += 0.75
    a = grad_with(g2, False)
    eng.set_dedup(0)
    eng.grad(0)
    torch.cuda.synchronize()
    b = gb.cpu().numpy().copy()
    assert np.max(np.abs(a[:eng.P] - b[:eng.P])) <= 1e-4 * np.max(np.abs(b[:eng.P]))
    assert_pair_close(a, b, d_in, widths, 1e-4, dim=dim, what='general path vs row-wise')
    assert not np.array_equal(a, g_tab)
    eng.close()


def test_inconsistent_dedup_map_is_an_error_not_a_fault():
    """vn_set_dedup validates the map on the device: every later kernel indexes device memory with it."""
    from varnet_amd.engine import VNEngine, VNError
    rng = np.random.default_rng(3)
    d_in, dim, q, n_k, U = 3, 2, 16, 20, 100
    n = n_k * q
    Xu = rng.uniform(-1, 1, (U, d_in)).astype(np.float32)
    uid = rng.integers(0, U, n).astype(np.int32)
    uid[:U] = np.arange(U)
    rowptr, rowidx = _csr(uid, U)
    eng = VNEngine(dim, d_in, [20, 20], True, q)
    eng.init_params(seed=1)
    eng.set_fe_table(rng.uniform(0, 1, q).astype(np.float32), rng.standard_normal(q).astype(np.float32))
    eng.set_interior(0, Xu[uid], rng.standard_normal((n, dim)).astype(np.float32), None, n_k=n_k, detJ=0.1)
    eng.set_bic(rng.uniform(-1, 1, (8, d_in)).astype(np.float32), rng.standard_normal((8, 1)).astype(np.float32), 4, 2.0)
    eng.set_weights([1.0, 1.0, 1.0])
    eng.set_dedup(0, Xu, uid, rowptr, rowidx)                         # the consistent map registers
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    g_dd = gb.cpu().numpy().copy()
    eng.set_dedup(0)
    eng.grad(0)
    torch.cuda.synchronize()
    g_row = gb.cpu().numpy().copy()
    for what in ('uid', 'rowidx_range', 'rowidx_owner', 'rowptr_end', 'rowptr_order', 'rowidx_duplicate'):
        u2, rp2, ri2 = uid.copy(), rowptr.copy(), rowidx.copy()
        eng.set_dedup(0, Xu, uid, rowptr, rowidx)                     # a good registration that the bad call must REPLACE
        if what == 'rowidx_duplicate':
            # a row listed twice under its own point (and its neighbour never): every range / owner test passes, the
            # gradient would be silently wrong -- caught by the order rule that makes rowidx a permutation
            i = int(np.argmax(np.diff(rowptr) >= 2))
            ri2[rowptr[i] + 1] = ri2[rowptr[i]]
        elif what == 'uid':
            u2[5] = U + 7
        elif what == 'rowidx_range':
            ri2[11] = n + 1000000
        elif what == 'rowidx_owner':
            ri2[[0, -1]] = ri2[[-1, 0]]                              # two rows filed under the wrong points
        elif what == 'rowptr_end':
            rp2[-1] = n - 1
        else:
            rp2[3], rp2[4] = rp2[4] + 5, rp2[3]
        with pytest.raises(VNError, match='inconsistent de-duplication map'):
            eng.set_dedup(0, Xu, u2, rp2, ri2)
        # a rejected map leaves the batch ROW-WISE (not on the previous registration, whose arrays the binding released)
        eng.grad(0)
        torch.cuda.synchronize()
        assert np.array_equal(gb.cpu().numpy(), g_row), what
    with pytest.raises(AssertionError, match='one entry per interior row'):
        eng.set_dedup(0, Xu, uid[:-q], rowptr, rowidx[:-q])           # short arrays never reach the device validator
    eng.set_dedup(0, Xu, uid, rowptr, rowidx)
    eng.grad(0)                                                      # the engine is still usable
    torch.cuda.synchronize()
    assert np.array_equal(gb.cpu().numpy(), g_dd)
    # a batch without interior rows has nothing to de-duplicate: an error code, not a zero-size launch
    eng.set_interior(1, Xu[uid][:0], np.zeros((0, dim), dtype=np.float32), None, n_k=0, detJ=0.1)
    with pytest.raises(VNError, match='no interior rows'):
        eng.set_dedup(1, Xu, uid[:0], rowptr, rowidx[:0])
    eng.close()


def test_forward_grad_refuses_networks_outside_the_fused_family():
    from varnet_amd.engine import VNEngine, VNError
    eng = VNEngine(2, 3, [128, 128], True, 16)
    eng.init_params(seed=1)
    with pytest.raises(VNError):
        eng.forward_grad(np.zeros((4, 3), dtype=np.float32))
    eng.close()


@pytest.mark.parametrize('widths,q,n_k,src', [([50, 50, 50, 50], 16, 20000, True),     # <4,13>: all 3 hidden layers stashed in LDS
                                               ([50, 50, 50], 64, 5000, False),          # <3,13>
                                               ([50, 50], 64, 5000, False),              # <2,13>: one hidden layer
                                               ([30, 30, 30, 30], 16, 20000, False),     # <4,8>: generic cooperative path
                                               ([50, 50, 50, 50, 50], 216, 1500, True)])  # two-pass route, several tiles per workgroup
def test_many_tiles_per_workgroup_fused_vs_generic(widths, q, n_k, src):
    """Each workgroup loops over several 128-point tiles (persistent / LDS-stashed weight-gradient accumulators,
    fixed-order flush): the fused gradient must equal the generic kernels' (independent implementation) to fp32
    rounding, and two runs must agree bit for bit."""
    d_in, dim, nB, bDof = 3, 2, 900, 500
    d = synth(11, d_in, dim, widths, q, n_k, nB, bDof, src, q == 216, False)
    grads = []
    for kernel in (1, 0, 0):
        eng = make_engine(d_in, dim, widths, q, src, q == 216, kernel)
        eng.init_params(seed=2)
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=d['detJ'])
        eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
        eng.set_weights(d['w'])
        gb = eng.bind_grad_buffer()
        eng.grad(0)
        torch.cuda.synchronize()
        grads.append(gb.cpu().numpy().copy())
        eng.close()
    g_gen, g_a, g_b = grads
    assert np.array_equal(g_a, g_b)
    P = g_gen.size - 4
    assert abs(g_a[P] - g_gen[P]) <= 2e-5 * abs(g_gen[P])
    assert np.max(np.abs(g_a[:P] - g_gen[:P])) <= 2e-4 * np.max(np.abs(g_gen[:P]))
    ERRORS['many_tiles %s q%d fused vs generic' % (widths, q)] = assert_pair_close(g_a, g_gen, d_in, widths, 2e-4, dim=dim)


# ---- reference-generated inputs (tests/golden/assembly.npz, written by oracle/gen_golden_assembly.py from the
# reference's own VarNet.py / VarNetUtility.py) through the HIP engine, against the oracle -------------------
@pytest.mark.parametrize('key,widths', [
    ('2dt_ip2_bnNone_blNone_pu1', [50] * 5),
    ('2dt_ip3_bnNone_blNone_pu1', [50, 50, 50]),          # integNum 216: two-pass fused route, integW
    ('1dt_ip2_bnNone_blNone_pu1', [50] * 4),
    ('1dt_ip3_bnNone_blNone_pu1', [20, 20, 20]),          # integNum 36, integW
    ('2dt_var', [32, 17]),                                # variable kappa / v, source term
    ('1d_steady', [20, 20, 20]),                          # steady 1D with a source: d_in = dim = 1, integNum 4
    ('2d_steady_ip2', [50] * 5),                          # steady 2D (assembly_steady.npz): integNum 16, variable data
    ('2d_steady_ip3', [64, 51, 64]),                      # ... integNum 36, integW, bf16-piece widths
])
def test_reference_assembled_inputs_through_engine(key, widths):
    import os
    from varnet_amd.engine import VNEngine
    name = 'assembly_steady.npz' if key.startswith('2d_steady') else 'assembly.npz'
    G = np.load(os.path.join(os.path.dirname(__file__), 'golden', name), allow_pickle=True)
    g = key + '_'
    td = G[g + 'dNt'].dtype != object                    # the reference builds no dNt table for a steady problem (None)
    sc = G[g + 'scalars']
    nt, nT, q, detJ, bDof, biDimVal = int(sc[0]), int(sc[1]), int(sc[2]), float(sc[3]), int(sc[4]), float(sc[5])
    Input, gcoef = G[g + 'Input'], G[g + 'gcoef']
    d_in, dim = Input.shape[1], gcoef.shape[1]
    source = bool(np.any(G[g + 'source']))
    integW = G[g + 'integW']
    has_w = integW.size > 0
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=has_w)
    eng.init_params(seed=11)
    flat = eng.get_params()
    dNt = G[g + 'dNt'] if td else np.zeros((nt * q, 1))
    eng.set_fe_table(G[g + 'N'][:q], dNt[:q], integW.reshape(-1) if has_w else None)
    eng.set_interior(0, Input, gcoef, G[g + 'source'] if source else None, n_k=nt, detJ=detJ)
    eng.set_bic(G[g + 'biInput'], G[g + 'biLabel'], bDof, biDimVal)
    w = np.array([3.0, 2.0, 5.0]) if td else np.array([3.0, 0.0, 5.0])       # VarNet.py:1132: IC weight 0 when steady
    eng.set_weights(w)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)       # what the device is fed (TFModel.py:531)
    kw = dict(Input=f32(Input), gcoef=f32(gcoef), source=f32(G[g + 'source']) if source else None,
              N=f32(G[g + 'N']), dNt=f32(dNt), integW=f32(integW.reshape(1, -1)) if has_w else None,
              intShape=[nt, q], detJ=float(np.float32(detJ)), detJvec=False, biInput=f32(G[g + 'biInput']),
              biLabel=f32(G[g + 'biLabel']), bDof=bDof, biDimVal=biDimVal, w=w, dim=dim, time_dependent=td,
              is_source=source, integWflag=has_w)
    ref, gref = og.loss_and_grad(flat.astype(np.float64), d_in, widths, torch.float64, **kw)
    out, lv = eng.eval_loss(0, lossVec=True)
    for got, k in zip(out, ['loss', 'BCloss', 'ICloss', 'varLoss']):
        assert abs(got - ref[k]) <= LOSS_RTOL * abs(ref[k]) + 1e-7, (k, got, ref[k])
    lref = ref['lossVec'].reshape(-1)
    # On real PDE inputs R_k is a sum of integNum terms that cancel to ~1e-4 of their size (the weak residual is
    # small), so detJ*R_k^2 carries the fp32 rounding of that cancellation: the reference graph itself, evaluated
    # in fp32 (what TF-1 runs), deviates from fp64 by the same amount.  Bar: 1e-4 of the largest entry, or 4x the
    # fp32 restatement's own deviation from fp64, whichever is larger.
    kw32 = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for k, v in kw.items()}
    ref32, gref32 = og.loss_and_grad(flat, d_in, widths, torch.float32, **kw32)
    own = float(np.max(np.abs(ref32['lossVec'].reshape(-1).astype(np.float64) - lref)))
    dv = float(np.max(np.abs(lv.cpu().numpy() - lref)))
    ERRORS[('golden_' if td else 'steady golden_') + key] = {'lossVec_abs': dv, 'lossVec_fp32_oracle_abs': own, 'lossVec_scale': float(np.max(np.abs(lref)))}
    assert dv <= max(LVEC_RTOL * np.max(np.abs(lref)), 4 * own), (dv, own)
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    gg = gb.cpu().numpy()
    assert abs(gg[eng.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
    assert np.max(np.abs(gg[:eng.P] - gref)) / np.max(np.abs(gref)) <= GRAD_RTOL
    assert_grad_close(gg, gref, d_in, widths, GRAD_RTOL, g32=lambda: gref32, dim=dim, td=td, what=key,
                      rec=ERRORS[('golden_' if td else 'steady golden_') + key])
    assert td or (out[2] == 0.0 and gg[eng.P + 2] == 0.0)             # a steady ICloss is the constant 0
    eng.close()


@pytest.mark.parametrize('kernel', [1, 0], ids=['generic', 'auto'])
def test_empty_tower_feed(kernel):
    """n_k == 0 (a tower block past the end of the set, VarNetUtility.py:830-838): only the BC/IC rows count;
    with no BC/IC rows either, loss and gradient are exactly zero and nothing faults."""
    from varnet_amd.engine import VNEngine
    d = synth(3, 3, 2, [50] * 3, 64, 4, 50, 20)
    eng = VNEngine(2, 3, [50] * 3, True, 64, kernel=kernel)
    eng.init_params(seed=3)
    flat = eng.get_params()
    eng.set_fe_table(d['N1'], d['dNt1'], None)
    empty = torch.zeros(0, 3, device='cuda')
    eng.set_interior(0, empty, torch.zeros(0, 2, device='cuda'), None, n_k=0, detJ=0.137)
    eng.set_bic(d['biInput'], d['biLabel'], 20, 2.0)
    eng.set_weights(d['w'])
    ref, gref = og.loss_and_grad(
        flat.astype(np.float64), 3, [50] * 3, torch.float64, Input=np.zeros((0, 3)), gcoef=np.zeros((0, 2)), source=None,
        N=np.zeros((0, 1)), dNt=np.zeros((0, 1)), integW=None, intShape=[0, 64], detJ=0.137, detJvec=False,
        biInput=d['biInput'].astype(np.float64), biLabel=d['biLabel'].astype(np.float64), bDof=20, biDimVal=2.0,
        w=d['w'], dim=2, time_dependent=True, is_source=False, integWflag=False)
    out, lv = eng.eval_loss(0, lossVec=True)
    assert lv.numel() == 0 and out[3] == 0.0
    assert abs(out[0] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    g = gb.cpu().numpy()
    assert abs(g[eng.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
    assert np.max(np.abs(g[:eng.P] - gref)) <= GRAD_RTOL * np.max(np.abs(gref))
    assert_grad_close(g, gref, 3, [50] * 3, GRAD_RTOL, dim=2, what='BC/IC rows only')
    eng.set_bic(None, None, 0, 2.0)                     # nothing at all
    out, _ = eng.eval_loss(0)
    eng.grad(0)
    torch.cuda.synchronize()
    assert out == [0.0, 0.0, 0.0, 0.0] and not gb.cpu().numpy().any()
    eng.close()


@pytest.mark.parametrize('kernel,path', [(0, 3), (1, 1)], ids=['auto', 'generic'])
def test_six_wide_layers(kernel, path):
    """6 layers wider than 50: on the 8-wave fused kernel (its flush image lies over the dead weight images to fit the
    160 KB), and on the generic kernels, whose backward kernel switches to the 65-float row stride at widths > 61.
    Checked against the fp64 oracle."""
    from varnet_amd.engine import VNEngine
    for widths in ([64] * 6, [55, 60, 52, 64, 51, 58]):
        d = synth(9, 3, 2, widths, 16, 30, 40, 15)
        eng = VNEngine(2, 3, widths, True, 16, kernel=kernel)
        assert eng.kernel_path()[0] == path
        eng.init_params(seed=2)
        flat = eng.get_params()
        eng.set_fe_table(d['N1'], d['dNt1'], None)
        eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=30, detJ=d['detJ'])
        eng.set_bic(d['biInput'], d['biLabel'], 15, 2.0)
        eng.set_weights(d['w'])
        ref, gref = oracle_eval(flat, d, 3, 2, widths, 16, 30, 15, False, False, False)
        gb = eng.bind_grad_buffer()
        eng.grad(0)
        torch.cuda.synchronize()
        g = gb.cpu().numpy()
        assert abs(g[eng.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
        assert np.max(np.abs(g[:eng.P] - gref)) <= GRAD_RTOL * np.max(np.abs(gref))
        ERRORS['six_wide %s %s' % (widths, kernel)] = assert_grad_close(
            g, gref, 3, widths, GRAD_RTOL, dim=2, what=str(widths),
            g32=lambda: oracle_eval(flat, d, 3, 2, widths, 16, 30, 15, False, False, False, dtype=torch.float32)[1])
        eng.close()


# ---- row a10: vn_params_init == the oracle's glorot_init (TFModel.py:213,219,242; global_variables_initializer) ------
@pytest.mark.parametrize('d_in,dim,widths,seed', [
    (2, 1, [20], 0),                         # Operator_1Dt.py:156
    (3, 2, [50, 50, 50, 50, 50], 1),         # BASELINE config 3
    (3, 1, [10, 20, 30], 12345678901234567), # Operator_1DtMOR.py:189 (a seed beyond 2**53: the stream is 64-bit)
    (2, 1, [7, 128, 3], 7),                  # ragged, layer-by-layer route
])
def test_params_init_equals_oracle_glorot(d_in, dim, widths, seed):
    """Same splitmix64 stream bit for bit, limits sqrt(6/(fan_in+fan_out)) (keras glorot_uniform, also the default of
    the Dense(1) output layer), zero biases, zero Adam slots, step 0 -- also after training steps have moved all of it."""
    eng = make_engine(d_in, dim, widths, 16, False, False)
    P = eng.P
    assert P == og.param_count(d_in, widths)

    def check():
        ref = og.glorot_init(d_in, widths, seed)
        got = eng.get_params()
        assert got.dtype == np.float32 and ref.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))          # bit for bit
        off = 0
        for fi, fo in og.layer_dims(d_in, widths):
            W, b = got[off:off + fi * fo], got[off + fi * fo:off + fi * fo + fo]
            lim = np.sqrt(6.0 / (fi + fo))
            assert np.all(np.abs(W) <= np.float32(lim)) and np.all(b == 0)
            if fi * fo >= 400:
                assert np.max(np.abs(W)) > 0.9 * lim and abs(W.mean()) < 0.15 * lim   # uniform on (-lim, lim)
            off += fi * fo + fo
        assert off == P
        st = np.asarray(eng.export_state(), dtype=np.uint8)
        assert int(st[:8].view(np.int64)[0]) == 0 and eng.step == 0              # step 0
        slots = st[8:].view(np.float32)
        assert slots.size == 3 * P and np.array_equal(slots[:P].view(np.uint32), ref.view(np.uint32))
        assert np.all(slots[P:] == 0)                                              # Adam m, v = 0

    eng.init_params(seed=seed)
    check()
    # move parameters, slots and the step counter, then re-initialise (VarNet.py:1412)
    d = synth(3, d_in, dim, widths, 16, 24, 20, 12)
    eng.set_fe_table(d['N1'], d['dNt1'])
    eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=24, detJ=float(d['detJ']))
    eng.set_bic(d['biInput'], d['biLabel'], 12, 2.0)
    eng.set_weights(d['w'])
    for _ in range(3):
        eng.train_step(0)
    torch.cuda.synchronize()
    assert eng.step == 3 and not np.array_equal(eng.get_params(), og.glorot_init(d_in, widths, seed))
    eng.init_params(seed=seed)
    check()
    eng.init_params(seed=seed + 1)
    assert not np.array_equal(eng.get_params(), og.glorot_init(d_in, widths, seed))
    eng.close()
