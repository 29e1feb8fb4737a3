"""
GPU tier of vn_objective_f64 (VNEngine.objective64): the weak-form objective of a batch and its gradient, evaluated in double
precision on the device, against the fp64 oracle (oracle/tf1_graph.py, tests/flux_ref.py).

Bars (fixed by the issue that asked for the path, from CPU runs of two independent fp64 evaluations of the same cases, which
differ by at most 5.8e-14):
    gradient   tests/gradcheck.block_errors, every block <= 1e-11
    lossVec    <= 1e-11 of its maximum
    loss, BC, IC, var   relative 1e-12
    central difference of the loss along v at h = 1e-5 against g.v: 1e-8 (relative to |g.v|; the oracle's own worst is 8.7e-11)
An evaluation with a single-precision stage misses the first three by four orders of magnitude (the lowest deviation recorded
for an fp32 evaluation is 9.8e-8), and an fp32 loss resolves the difference quotient to a few percent only.

Inputs as tests/parity_cases.py builds them: synth(100 + i, ...) for CASES[i] with n_k cut so that n_k * integNum <= 3000, and
parameters glorot_init(d_in, widths, 2) + 0.05 * default_rng(5).standard_normal(P) kept in fp64 -- not fp32-representable, so
the theta argument is exercised.  The worst deviations seen are written to obj64_parity.json in the directory VN_RECORD_DIR names
(default: profile_out/ beside tests/; the committed copy: profiles/obj64_parity.json).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests import flux_ref
from tests.gradcheck import block_errors
from tests.parity_cases import CASES, GRAD_RTOL, LOSS_RTOL, STEADY, oracle_eval, steady_inputs, steady_oracle, synth

pytestmark = pytest.mark.gpu

GRAD_BAR = 1e-11
LVEC_BAR = 1e-11
LOSS_BAR = 1e-12
FD_BAR = 1e-8
KEYS = ['loss', 'BCloss', 'ICloss', 'varLoss']

WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _dump_worst():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'obj64_parity.json'), 'w') as f:
            json.dump(WORST, f, indent=1, sort_keys=True)
    except OSError:
        pass


def theta64(d_in, widths):
    flat = og.glorot_init(d_in, widths, 2).astype(np.float64)
    return flat + 0.05 * np.random.default_rng(5).standard_normal(flat.size)


def cut(case, rows=3000):
    d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec = case
    return (d_in, dim, widths, q, max(1, min(n_k, rows // q)), nB, bDof, source, integW, detJvec)


@functools.lru_cache(maxsize=None)
def case_data(i, rows=3000):
    """(cut case, inputs, theta, oracle result, oracle gradient) of CASES[i]: computed once, shared, never modified."""
    case = cut(CASES[i], rows)
    d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec = case
    d = synth(100 + i, d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec)
    th = theta64(d_in, widths)
    ref, gref = oracle_eval(th, d, d_in, dim, widths, q, n_k, bDof, source, integW, detJvec)
    return case, d, th, ref, gref


def engine_for(case, d, td=True, act='sigmoid', biDimVal=2.0, **kw):
    from varnet_amd.engine import VNEngine
    d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec = case
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW, activationFun=act, **kw)
    eng.init_params(seed=3)
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, biDimVal)
    eng.set_weights(d['w'])
    return eng


def check(tag, out, g, lv, ref, gref, d_in, widths, dim, td=True):
    """Prints every figure, records it, then asserts the bars."""
    rec = {}
    for got, key in zip(out, KEYS):
        rec[key] = abs(got - ref[key]) / max(abs(ref[key]), 1e-300) if ref[key] != 0.0 else abs(got)
    if lv is not None:
        lref = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1)
        lvn = lv.cpu().numpy()
        assert lvn.shape == lref.shape
        rec['lossVec'] = float(np.max(np.abs(lvn - lref)) / np.max(np.abs(lref))) if lref.size else 0.0
    if g is not None:
        errs = block_errors(g.cpu().numpy(), gref, d_in, widths, dim, td)
        worst = max(errs, key=errs.get)
        rec['worst_block'], rec['worst_block_err'] = worst, errs[worst]
    WORST[tag] = rec
    print('obj64 %s: %s' % (tag, json.dumps(rec, sort_keys=True)))
    for key in KEYS:
        assert rec[key] <= LOSS_BAR, (tag, key, rec[key])
    if lv is not None:
        assert rec['lossVec'] <= LVEC_BAR, (tag, rec['lossVec'])
    if g is not None:
        assert rec['worst_block_err'] <= GRAD_BAR, (tag, rec['worst_block'], rec['worst_block_err'])
    return rec


# 19: one layer [20] | 4: [7], source, integW, detJ vector, integNum 36 (tiles straddle test functions) | 1: 5x50, 13 k-steps |
# 27: six ragged layers 51..64 | 26: [64]*6 (the weight images exceed the LDS as doubles) | 5: integNum 216 | 29: widths 17..32,
# detJ vector | 33: d_in 6 | 35: d_in 8, dim 3, 216 | 3: MOR-style input
@pytest.mark.parametrize('i', [19, 4, 1, 27, 26, 5, 29, 33, 35, 3])
def test_parity_with_the_oracle(i):
    case, d, th, ref, gref = case_data(i)
    eng = engine_for(case, d)
    try:
        out, g, lv = eng.objective64(0, theta=th, grad=True, lossVec=True)
        check('case%d' % i, out, g, lv, ref, gref, case[0], case[2], case[1])
    finally:
        eng.close()


# 0 | 5: tanh, five layers, detJ vector | 6: rows behind bDof must be ignored | 14: d_in = dim + 5
@pytest.mark.parametrize('i', [0, 5, 6, 14])
def test_parity_steady(i):
    full = STEADY[i]
    d_in, dim, widths, q, n_k, nB, bDof, act, has_w, detJvec = full
    case = (d_in, dim, widths, q, max(1, min(n_k, 3000 // q)), nB, bDof, act, has_w, detJvec)
    d, _ = steady_inputs(case)
    th = theta64(d_in, widths)
    ref, gref = steady_oracle(th, d, case)
    assert ref['ICloss'] == 0.0
    ecase = (d_in, dim, widths, q, case[4], nB, bDof, True, has_w, detJvec)
    eng = engine_for(ecase, d, td=False, act=act, biDimVal=1.5)
    try:
        out, g, lv = eng.objective64(0, theta=th, grad=True, lossVec=True)
        assert out[2] == 0.0
        check('steady%d' % i, out, g, lv, ref, gref, d_in, widths, dim, td=False)
    finally:
        eng.close()


def test_parity_per_row_tables():
    """Per-row N_rows / dNt_rows in place of the FE table, with a detJ vector, a source term and integW (integNum 36)."""
    from varnet_amd.engine import VNEngine
    d_in, dim, widths, q, n_k, nB, bDof = 3, 2, [10, 20], 36, 45, 31, 17
    rng = np.random.default_rng(11)
    n = n_k * q
    f32 = np.float32
    Input = rng.uniform(-1, 1, (n, d_in)).astype(f32)
    gcoef = rng.standard_normal((n, dim)).astype(f32)
    src = rng.standard_normal((n, 1)).astype(f32)
    Nrow = rng.uniform(0, 1, (n, 1)).astype(f32)
    dNtrow = rng.standard_normal((n, 1)).astype(f32)
    detJ = rng.uniform(0.01, 0.05, (n_k, 1)).astype(f32)
    integW = rng.uniform(0.5, 1, (1, q)).astype(f32)
    biInput = rng.uniform(-1, 1, (nB, d_in)).astype(f32)
    biLabel = rng.standard_normal((nB, 1)).astype(f32)
    w = np.array([2.0, 3.0, 4.0])
    th = theta64(d_in, widths)
    f64 = np.float64
    ref, gref = og.loss_and_grad(
        th, d_in, widths, torch.float64, Input=Input.astype(f64), gcoef=gcoef.astype(f64), source=src.astype(f64),
        N=Nrow.astype(f64), dNt=dNtrow.astype(f64), integW=integW.astype(f64), intShape=[n_k, q], detJ=detJ.astype(f64),
        detJvec=True, biInput=biInput.astype(f64), biLabel=biLabel.astype(f64), bDof=bDof, biDimVal=2.0, w=w, dim=dim,
        time_dependent=True, is_source=True, integWflag=True)
    eng = VNEngine(dim, d_in, widths, True, q, isSource=True, integWflag=True)
    try:
        eng.init_params(seed=5)
        eng.set_fe_table(np.zeros(q, f32), np.zeros(q, f32), integW)      # tables unused: per-row data
        eng.set_interior(0, Input, gcoef, src, n_k=n_k, detJ=detJ, N_rows=Nrow, dNt_rows=dNtrow)
        eng.set_bic(biInput, biLabel, bDof, 2.0)
        eng.set_weights(w)
        out, g, lv = eng.objective64(0, theta=th, grad=True, lossVec=True)
        check('per_row_tables', out, g, lv, ref, gref, d_in, widths, dim)
    finally:
        eng.close()


def test_parity_batch_bic_and_empty_feed():
    """The batch's own copy of the BC/IC rows (vn_set_batch_bic) is what the evaluation reads; an empty feed (n_k == 0) leaves
    the BC/IC rows alone."""
    case, d, th, ref, gref = case_data(0)
    d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec = case
    rng = np.random.default_rng(21)
    d2 = dict(d)
    d2['biInput'] = rng.uniform(-1, 1, (nB, d_in)).astype(np.float32)
    d2['biLabel'] = rng.standard_normal((nB, 1)).astype(np.float32)
    ref2, gref2 = oracle_eval(th, d2, d_in, dim, widths, q, n_k, bDof, source, integW, detJvec)
    assert abs(ref2['BCloss'] - ref['BCloss']) > 1e-3 * abs(ref['BCloss'])
    eng = engine_for(case, d)
    try:
        eng.set_batch_bic(0, d2['biInput'], d2['biLabel'])
        out, g, lv = eng.objective64(0, theta=th, grad=True, lossVec=True)
        check('batch_bic', out, g, lv, ref2, gref2, d_in, widths, dim)
        # batch 1: an empty feed
        dev = eng.device
        eng.set_interior(1, torch.zeros(0, d_in, device=dev), torch.zeros(0, dim, device=dev), None, n_k=0, detJ=0.137)
        ref0, gref0 = og.loss_and_grad(
            th, d_in, widths, torch.float64, Input=np.zeros((0, d_in)), gcoef=np.zeros((0, dim)), source=None,
            N=np.zeros((0, 1)), dNt=np.zeros((0, 1)), integW=None, intShape=[0, q], detJ=0.137, detJvec=False,
            biInput=d['biInput'].astype(np.float64), biLabel=d['biLabel'].astype(np.float64), bDof=bDof, biDimVal=2.0,
            w=d['w'], dim=dim, time_dependent=True, is_source=False, integWflag=False)
        out, g, lv = eng.objective64(1, theta=th, grad=True, lossVec=True)
        assert lv.numel() == 0 and out[3] == 0.0
        ref0['lossVec'] = np.zeros(0)
        check('empty_feed', out, g, lv, ref0, gref0, d_in, widths, dim)
    finally:
        eng.close()


FLUX = [
    # d_in dim widths             integNum n_k nB  bDof nF  td     act        integW      (two networks of tests/test_flux_bc_gpu.py)
    (2, 1, [20],                  16,      40, 50, 30,  30, True,  'tanh',    False),
    (3, 2, [50, 50, 50, 50, 50],  64,      9,  77, 40,  60, True,  'sigmoid', False),
]


@pytest.mark.parametrize('fcase', FLUX, ids=['1dt_tanh', '2dt_50x5'])
def test_parity_flux_rows(fcase):
    from varnet_amd.engine import VNEngine
    d_in, dim, widths, q, n_k, nB, bDof, nF, td, act, integW = fcase
    d = synth(11, d_in, dim, widths, q, n_k, nB, bDof, integW=integW)
    rng = np.random.default_rng(12)
    nrm = rng.standard_normal((nF, dim))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    coef = rng.uniform(0.5, 2.0, nF)
    coef[:nF // 2] = 0.0
    # rounded to fp32 first: the engine registers fp32 rows and widens them exactly
    fx = {k: np.asarray(v).astype(np.float32) for k, v in
          dict(X=rng.uniform(-1, 1, (nF, d_in)), normal=nrm, coef=coef, label=rng.standard_normal(nF)).items()}
    th = theta64(d_in, widths)
    f = np.float64
    kw = dict(Input=d['Input'].astype(f), gcoef=d['gcoef'].astype(f), source=None, N=d['N'].astype(f), dNt=d['dNt'].astype(f),
              integW=None, intShape=[n_k, q], detJ=float(d['detJ']), detJvec=False, biInput=d['biInput'].astype(f),
              biLabel=d['biLabel'].astype(f), bDof=bDof, biDimVal=2.0, w=d['w'], dim=dim, time_dependent=td, is_source=False,
              integWflag=False, activation=act)
    ref, gref = flux_ref.loss_and_grad(th, d_in, widths, {k: v.astype(f) for k, v in fx.items()}, dtype=torch.float64, **kw)
    ref0, _ = og.loss_and_grad(th, d_in, widths, torch.float64, **kw)
    assert abs(ref['BCloss'] - ref0['BCloss']) > 1e-2 * abs(ref['BCloss'])        # the flux term is a real part of BC here
    eng = VNEngine(dim, d_in, widths, td, q, integWflag=integW, activationFun=act)
    try:
        eng.init_params(seed=3)
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=n_k, detJ=d['detJ'])
        eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
        eng.set_weights(d['w'])
        eng.set_flux_bc(fx['X'], fx['normal'], fx['coef'], fx['label'], 2.0)
        out, g, lv = eng.objective64(0, theta=th, grad=True, lossVec=True)
        check('flux_%s' % 'x'.join(map(str, widths)), out, g, lv, ref, gref, d_in, widths, dim, td)
    finally:
        eng.close()


@pytest.mark.parametrize('i', [0, 3, 4, 19, 35])
def test_finite_differences_through_theta(i):
    """(f(theta + h v) - f(theta - h v)) / 2h against g.v at h = 1e-5, the shifted calls in their loss-only form."""
    case, d, th, _, _ = case_data(i, 2000)
    eng = engine_for(case, d)
    try:
        v = np.random.default_rng(9).standard_normal(th.size)
        v /= np.max(np.abs(v))
        h = 1e-5
        _, g, _ = eng.objective64(0, theta=th, grad=True)
        fp, gp, _ = eng.objective64(0, theta=th + h * v, grad=False)
        fm, gm, _ = eng.objective64(0, theta=th - h * v, grad=False)
        assert gp is None and gm is None
        gv = float(np.dot(g.cpu().numpy(), v))
        fd = (fp[0] - fm[0]) / (2 * h)
        err = abs(fd - gv) / abs(gv)
        WORST['fd_case%d' % i] = {'g.v': gv, 'difference_quotient': fd, 'rel_err': err}
        print('obj64 fd case%d: g.v = %.15e  fd = %.15e  rel err %.3e' % (i, gv, fd, err))
        assert err <= FD_BAR, (i, gv, fd, err)
    finally:
        eng.close()


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def test_contract_bits_and_arguments():
    case, d, th, _, _ = case_data(1)
    d_in, dim, widths, q, n_k = case[:5]
    eng = engine_for(case, d)
    try:
        out1, g1, lv1 = eng.objective64(0, theta=th, grad=True, lossVec=True)
        out2, g2, lv2 = eng.objective64(0, theta=th, grad=True, lossVec=True)
        assert out1 == out2 and _bits(g1) == _bits(g2) and _bits(lv1) == _bits(lv2)          # two calls: identical bits
        out3, g3, _ = eng.objective64(0, theta=th, grad=False)
        assert g3 is None and out3 == out1                                                   # loss only: the same scalars
        # theta = None: the engine's own parameters, widened
        p32 = eng.get_params()
        outn, gn, lvn = eng.objective64(0, grad=True, lossVec=True)
        outw, gw, lvw = eng.objective64(0, theta=p32.astype(np.float64), grad=True, lossVec=True)
        assert outn == outw and _bits(gn) == _bits(gw) and _bits(lvn) == _bits(lvw)
        assert outn != out1
        # a de-duplication map on the batch is ignored (identity map: every row its own point)
        nT = d['Input'].shape[0]
        idx = torch.arange(nT, dtype=torch.int32)
        eng.set_dedup(0, d['Input'], idx, torch.arange(nT + 1, dtype=torch.int32), idx)
        outd, gd, lvd = eng.objective64(0, theta=th, grad=True, lossVec=True)
        assert outd == out1 and _bits(gd) == _bits(g1) and _bits(lvd) == _bits(lv1)
        eng.set_dedup(0)
    finally:
        eng.close()


def test_contract_engine_state_is_left_alone():
    case, d, th, _, _ = case_data(1)
    eng = engine_for(case, d)
    try:
        gb = eng.bind_grad_buffer()
        eng.train_step(0)                                  # a step behind it: optimizer slots and step counter are not trivial
        eng.grad(0)
        torch.cuda.synchronize()
        before = (eng.get_params().tobytes(), eng.export_state().tobytes(), eng.step, _bits(gb))
        eng.objective64(0, theta=th, grad=True, lossVec=True)
        eng.objective64(0, grad=True)
        eng.eval_loss(0, lossVec=True, fp64=True)
        torch.cuda.synchronize()
        after = (eng.get_params().tobytes(), eng.export_state().tobytes(), eng.step, _bits(gb))
        assert before == after
        eng.grad(0)
        torch.cuda.synchronize()
        assert _bits(gb) == before[3]                      # vn_grad on the same batch afterwards: bitwise what it was
        out64, lv64 = eng.eval_loss(0, lossVec=True, fp64=True)
        assert lv64.dtype == torch.float64
        out32, lv32 = eng.eval_loss(0, lossVec=True)
        assert lv32.dtype == torch.float32 and abs(out32[0] - out64[0]) <= LOSS_RTOL * abs(out64[0])
    finally:
        eng.close()


def test_contract_errors():
    from varnet_amd.engine import VNEngine, VNError
    case, d, th, _, _ = case_data(19)
    eng = engine_for(case, d)
    try:
        with pytest.raises(VNError, match='error 3'):      # VN_ESTATE: batch 5 was never registered
            eng.objective64(5, theta=th)
        with pytest.raises(ValueError):
            eng.objective64(0, theta=th[:-1])
        assert eng.lib.vn_objective_f64(eng.h, 0, None, None, None, None) == 1      # out == NULL: VN_EINVAL
    finally:
        eng.close()
    dd = synth(1, 3, 2, [20], 16, 4, 10, 5)
    for widths, act in (([128, 128], 'sigmoid'), ([20] * 7, 'sigmoid'), ([20, 20], ['tanh', 'sigmoid'])):
        eng = VNEngine(2, 3, widths, True, 16, activationFun=act)
        try:
            eng.init_params(seed=1)
            eng.set_fe_table(dd['N1'], dd['dNt1'], None)
            eng.set_interior(0, dd['Input'], dd['gcoef'], None, n_k=4, detJ=dd['detJ'])
            eng.set_bic(dd['biInput'], dd['biLabel'], 5, 2.0)
            with pytest.raises(VNError, match='error 5.*outside that range'):     # VN_EUNSUPPORTED, with a sentence that says so
                eng.objective64(0)
            eng.eval_loss(0)                               # ... and everything else of such an engine works
        finally:
            eng.close()


def test_fp32_step_against_device_fp64():
    """The fp32 vn_grad meets the suite's bars (LOSS_RTOL, GRAD_RTOL) against vn_objective_f64 at the engine's own parameters:
    the device evaluation serves where the CPU oracle did (the arithmetic of VarNet.precisionReport)."""
    case, d, _, _, _ = case_data(1)
    d_in, dim, widths = case[0], case[1], case[2]
    eng = engine_for(case, d)
    try:
        flat = eng.get_params() + 0.05 * np.random.default_rng(5).standard_normal(eng.P).astype(np.float32)
        eng.set_params(flat)
        gb = eng.bind_grad_buffer()
        eng.grad(0)
        torch.cuda.synchronize()
        a = gb.cpu().numpy().astype(np.float64)
        out, g, _ = eng.objective64(0, grad=True)
        g64 = g.cpu().numpy()
        for k in range(4):
            assert abs(a[eng.P + k] - out[k]) <= LOSS_RTOL * abs(out[k]) + 1e-7, (KEYS[k], a[eng.P + k], out[k])
        errs = block_errors(a, g64, d_in, widths, dim)
        glob = float(np.max(np.abs(a[:eng.P] - g64)) / np.max(np.abs(g64)))
        print('obj64 fp32 step against device fp64: global %.3e, worst block %.3e' % (glob, max(errs.values())))
        assert glob <= GRAD_RTOL
        assert max(errs.values()) <= GRAD_RTOL, errs
    finally:
        eng.close()


# ---- the opt-in L-BFGS line search on the fp64 loss (vn_lbfgs_loss64, VarNet(optimizer='lbfgs', lbfgsLoss64=True)) ----------
def _op1dt(**kw):
    from varnet_amd.adpde import ADPDE
    from varnet_amd.domain import Domain1D
    from varnet_amd.varnet import VarNet
    pde = ADPDE(Domain1D(), diff=0.1 / np.pi, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(np.pi * x))
    return VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=20, **kw)       # the [20] 1D+t problem, smallest size


def _lbfgs_run(tmp, n, **kw):
    """n iterations after train()'s own first epoch (weights scaled as train() scales them): infos and parameters per call."""
    vn = _op1dt(optimizer='lbfgs', **kw)
    eng = vn.engine
    try:
        vn.train(str(tmp), weight=[10., 10., 1.], epochNum=1, tol=0.0, saveFreq=10 ** 6, verbose=False)
        rows = []
        for _ in range(n):
            theta = eng.get_params()
            f64, _, _ = eng.objective64(0, grad=False)
            info = eng.lbfgs_step(0, 20)
            rows.append((info, theta, f64[0]))
        return rows, eng.get_params()
    finally:
        eng.close()


def test_lbfgs_line_search_on_the_fp64_loss(tmp_path):
    rows, _ = _lbfgs_run(tmp_path / 'on', 40, lbfgsLoss64=True)
    prev = None
    for k, (info, theta, f_at_theta) in enumerate(rows):
        # f_k is the fp64 objective at theta_k
        assert abs(info['f_k'] - f_at_theta) <= 1e-12 * abs(f_at_theta), (k, info['f_k'], f_at_theta)
        if prev is not None:
            assert info['f_k'] == prev                     # ... and the value the previous call left
        if info['status'] == 0:                            # Armijo in double with those values
            assert info['f_next'] <= info['f_k'] + 1e-4 * info['t'] * info['gd'], (k, info)
            assert info['f_next'] <= info['f_k']
        else:
            assert info['f_next'] == info['f_k']
        prev = info['f_next']
    assert sum(1 for info, _, _ in rows if info['status'] == 0) >= 30
    fs = [rows[0][0]['f_k']] + [info['f_next'] for info, _, _ in rows]
    assert np.all(np.diff(fs) <= 0.0)                      # the sequence never increases


def test_lbfgs_flag_off_is_bitwise_the_engine_without_it(tmp_path):
    from varnet_amd.engine import VNEngine, VNError
    plain, theta_plain = _lbfgs_run(tmp_path / 'plain', 40)

    def off(vn_kw_tmp):
        vn = _op1dt(optimizer='lbfgs')
        eng = vn.engine
        try:
            eng.lbfgs_loss64(True)
            eng.lbfgs_loss64(False)                        # heard of the flag, runs without it
            vn.train(str(vn_kw_tmp), weight=[10., 10., 1.], epochNum=1, tol=0.0, saveFreq=10 ** 6, verbose=False)
            infos = [eng.lbfgs_step(0, 20) for _ in range(40)]
            return infos, eng.get_params()
        finally:
            eng.close()
    infos, theta_off = off(tmp_path / 'off')
    assert [i for i, _, _ in plain] == infos
    assert theta_plain.tobytes() == theta_off.tobytes()
    # refusals: where the fp64 evaluation is refused, and on engines that are not L-BFGS engines
    eng = VNEngine(2, 3, [128, 128], True, 16, optimizer_name='lbfgs')
    try:
        with pytest.raises(VNError, match='error 5'):
            eng.lbfgs_loss64(True)
        eng.lbfgs_loss64(False)
    finally:
        eng.close()
    eng = VNEngine(1, 2, [20], True, 16)
    try:
        with pytest.raises(VNError, match='error 3'):
            eng.lbfgs_loss64(True)
    finally:
        eng.close()
