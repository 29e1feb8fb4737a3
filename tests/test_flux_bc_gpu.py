"""
GPU tier of the boundary-flux term (vn_set_flux_bc, `VarNet(fluxBC=True)`): parity of the loss components and the gradient
against the fp64 restatement (tests/flux_ref.py) on every route the kernels' range maps to, the composition of the step's
entry points with flux rows registered, the register-then-clear contract, the refusal outside the kernels' range, and three
small problems whose Neumann / Robin edge is now determined (the reference leaves it free).
"""
import numpy as np
import pytest
import torch

from tests import flux_ref
from tests.gradcheck import assert_grad_close
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, synth
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import (VN_KERNEL_AUTO, VN_KERNEL_FUSED, VN_KERNEL_GENERIC, VNEngine, VNError)
from varnet_amd.varnet import VarNet

pytestmark = pytest.mark.gpu

pi = np.pi

CASES = [
    # d_in dim widths             integNum n_k nB  bDof nF  td     act        integW
    (1, 1, [20],                  4,       37, 1,  1,   1,  False, 'sigmoid', False),   # 1D steady
    (2, 1, [20],                  16,      40, 50, 30,  30, True,  'tanh',    False),   # 1D+t
    (3, 2, [10, 20],              64,      5,  33, 20,  40, True,  'sigmoid', False),   # 2D+t: a Neumann wall and a Robin edge
    (3, 2, [50, 50, 50, 50, 50],  64,      9,  77, 40,  60, True,  'sigmoid', False),   # 2D+t, the bench network
    (3, 2, [64, 64],              216,     3,  5,  2,   25, True,  'sigmoid', True),    # integPnum = 3: the two-pass route
]
IDS = ['1d_steady', '1dt_tanh', '2dt_10_20', '2dt_50x5', '2dt_gauss3']


def flux_rows(seed, d_in, dim, nF):
    """Rows of a Neumann wall (coef 0, first half) and a Robin edge (coef != 0): points in [-1,1], unit normals."""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((nF, dim))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    coef = rng.uniform(0.5, 2.0, nF)
    coef[:nF // 2] = 0.0
    return dict(X=rng.uniform(-1, 1, (nF, d_in)), normal=n, coef=coef, label=rng.standard_normal(nF))


def setup(case, kernel=VN_KERNEL_AUTO, xcheck=False, flux=True, seed=11):
    d_in, dim, widths, q, n_k, nB, bDof, nF, td, act, integW = case
    d = synth(seed, d_in, dim, widths, q, n_k, nB, bDof, integW=integW)
    fx = flux_rows(seed + 1, d_in, dim, nF)
    eng = VNEngine(dim, d_in, widths, td, q, integWflag=integW, kernel=kernel, activationFun=act, xcheck=xcheck)
    eng.init_params(seed=3)
    flat = eng.get_params() + 0.05 * np.random.default_rng(5).standard_normal(eng.P).astype(np.float32)
    eng.set_params(flat)
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=n_k, detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
    eng.set_weights(d['w'])
    if flux:
        eng.set_flux_bc(fx['X'], fx['normal'], fx['coef'], fx['label'], 2.0)
    return eng, flat, d, fx


def reference(case, flat, d, fx, dtype=torch.float64):
    d_in, dim, widths, q, n_k, nB, bDof, nF, td, act, integW = case
    f = np.float64 if dtype == torch.float64 else np.float32
    kw = dict(Input=d['Input'].astype(f), gcoef=d['gcoef'].astype(f), source=None, N=d['N'].astype(f), dNt=d['dNt'].astype(f),
              integW=None if d['integW'] is None else d['integW'].astype(f), intShape=[n_k, q], detJ=float(d['detJ']),
              detJvec=False, biInput=d['biInput'][:nB if td else bDof].astype(f), biLabel=d['biLabel'][:nB if td else bDof].astype(f),
              bDof=bDof, biDimVal=2.0, w=d['w'], dim=dim, time_dependent=td, is_source=False, integWflag=integW, activation=act)
    fxc = {k: np.asarray(v).astype(f) for k, v in fx.items()}
    return flux_ref.loss_and_grad(flat.astype(f), d_in, widths, fxc, dtype=dtype, **kw)


def check_parity(case, eng, flat, d, fx, what):
    d_in, dim, widths, td = case[0], case[1], case[2], case[8]
    ref, gref = reference(case, flat, d, fx)
    out, _ = eng.eval_loss(0)
    for got, key in zip(out, ['loss', 'BCloss', 'ICloss', 'varLoss']):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (what, 'eval', key, got, ref[key])
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    g = gb.cpu().numpy().astype(np.float64)
    for got, key in zip(g[eng.P:], ['loss', 'BCloss', 'ICloss', 'varLoss']):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (what, 'grad', key, got, ref[key])
    assert_grad_close(g[:eng.P], gref, d_in, widths, GRAD_RTOL, dim=dim, td=td, what=what,
                      g32=lambda: reference(case, flat, d, fx, dtype=torch.float32)[1])
    # the flux term is a real part of the BC component here, not a rounding-sized one
    ref0, _ = reference(case, flat, d, {k: v[:0] for k, v in fx.items()})
    assert abs(ref['BCloss'] - ref0['BCloss']) > 1e-2 * abs(ref['BCloss'])


@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_flux_parity(case, kernel):
    eng, flat, d, fx = setup(case, kernel)
    try:
        check_parity(case, eng, flat, d, fx, '%s/%s' % (IDS[CASES.index(case)], kernel))
    finally:
        eng.close()


def test_flux_parity_with_dedup_map():
    """The de-duplicated formulation (identity point map: every row its own point) carries the flux rows too."""
    case = CASES[3]
    eng, flat, d, fx = setup(case)
    try:
        nT = d['Input'].shape[0]
        idx = torch.arange(nT, dtype=torch.int32)
        eng.set_dedup(0, d['Input'], idx, torch.arange(nT + 1, dtype=torch.int32), idx)
        check_parity(case, eng, flat, d, fx, 'dedup')
    finally:
        eng.close()


def test_flux_parity_on_crosscheck_fused32():
    case = CASES[2]
    eng, flat, d, fx = setup(case, VN_KERNEL_FUSED)
    try:
        check_parity(case, eng, flat, d, fx, 'fused32')
    finally:
        eng.close()


def _theta_after(eng, state, fn):
    eng.import_state(state)
    fn()
    torch.cuda.synchronize()
    return eng.get_params()


def test_train_step_equals_grad_then_apply():
    """train_step folds the update into the gradient reduction; grad + apply runs it as its own kernel.  Their relation is
    measured first without flux rows, then required to hold with them: a flux gradient that missed the fused update would move
    theta by about one Adam step (~lr) on every parameter."""
    case = CASES[2]
    eng, flat, d, fx = setup(case, flux=False)
    try:
        s0 = eng.export_state()
        gap = []
        for with_flux in (False, True):
            if with_flux:
                eng.set_flux_bc(fx['X'], fx['normal'], fx['coef'], fx['label'], 2.0)
            a = _theta_after(eng, s0, lambda: eng.train_step(0))
            b = _theta_after(eng, s0, lambda: (eng.grad(0), eng.apply()))
            assert np.max(np.abs(a - flat)) > 1e-4                       # the step moved theta
            gap.append(float(np.max(np.abs(a - b))))
        bar = max(2.0 * gap[0], 1e-6)
        assert gap[1] <= bar, gap
    finally:
        eng.close()


def test_train_epoch_is_k_single_steps():
    case = CASES[3]
    eng, flat, d, fx = setup(case)
    try:
        q = case[3]
        rng = np.random.default_rng(9)
        for b in (1, 2):                                                # batches 1 and 2: their own, shorter, interior sets
            n = (case[4] - b) * q
            eng.set_interior(b, rng.uniform(-1, 1, (n, case[0])).astype(np.float32), d['gcoef'][:n], None, n_k=case[4] - b,
                             detJ=d['detJ'])
        s0 = eng.export_state()
        acc = torch.zeros(1, device='cuda')
        a = _theta_after(eng, s0, lambda: eng.train_epoch((0, 1, 2, 0), acc))
        b = _theta_after(eng, s0, lambda: [eng.train_step(i) for i in (0, 1, 2, 0)])
        assert np.array_equal(a, b)
        assert eng.step == 4
    finally:
        eng.close()


def test_eval_loss_agrees_with_grad_buffer():
    for case in (CASES[1], CASES[4]):
        eng, flat, d, fx = setup(case)
        try:
            out, _ = eng.eval_loss(0)
            gb = eng.bind_grad_buffer()
            eng.grad(0)
            torch.cuda.synchronize()
            g = gb.cpu().numpy()[eng.P:]
            for i in range(4):
                assert abs(out[i] - g[i]) <= LOSS_RTOL * abs(g[i]) + 1e-7, (i, out, g)
        finally:
            eng.close()


@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
def test_register_then_clear_is_bitwise_untouched(kernel):
    case = CASES[2]
    runs = []
    for touched in (False, True):
        eng, flat, d, fx = setup(case, kernel, flux=touched)
        try:
            if touched:
                eng.grad(0)                                             # a step with the rows registered ...
                eng.set_flux_bc(None)                                   # ... then cleared
            out, _ = eng.eval_loss(0)
            gb = eng.bind_grad_buffer()
            eng.grad(0)
            torch.cuda.synchronize()
            g = gb.cpu().numpy().copy()
            for _ in range(3):
                eng.train_step(0)
            runs.append((np.array(out), g, eng.get_params()))
        finally:
            eng.close()
    for x, y in zip(runs[0], runs[1]):
        assert np.array_equal(x, y)


def test_refusal_outside_the_kernels_range(tmp_path):
    eng = VNEngine(1, 2, [128, 128], True, 16)
    try:
        X = np.zeros((4, 2)); n = np.ones((4, 1))
        with pytest.raises(VNError, match='error 5: boundary-flux rows need a network of the hand-written kernels'):
            eng.set_flux_bc(X, n, np.zeros(4), np.zeros(4), 1.0)
        eng.set_flux_bc(None)                                           # clearing is always accepted
    finally:
        eng.close()
    pde = ADPDE(Domain1D(np.array([0.0, 1.0])), diff=0.1, vel=0.0, tInterval=[0, 1.0], BCs=[[], [1.0, 0.0, 0.0]],
                IC=lambda x: np.sin(pi * x / 2))
    with pytest.raises(VNError, match='boundary-flux rows need a network of the hand-written kernels'):
        VarNet(pde, layerWidth=[128], discNum=10, bDiscNum=None, tDiscNum=10, fluxBC=True)


# ---- end to end: the Neumann / Robin edge is now determined ----------------------------------------------------------------
KAPPA = 0.5


def _steady(BCs):
    src = lambda x: KAPPA * (pi / 2) ** 2 * np.sin(pi * x / 2)
    return ADPDE(Domain1D(np.array([0.0, 1.0])), diff=KAPPA, vel=0.0, source=src, BCs=BCs, cEx=lambda x: np.sin(pi * x / 2))


def _train(pde, tmp_path, epochs, **kw):
    np.random.seed(0)
    vn = VarNet(pde, fluxBC=True, **kw)
    vn.train(str(tmp_path), epochNum=epochs, tol=0.0, saveFreq=epochs, verbose=False)
    err = vn.residual()[2]
    vn.engine.close()
    return err


E2E = dict(layerWidth=[20], discNum=40, bDiscNum=None, activationFun='tanh', learning_rate=0.01)


def test_steady_neumann_end_to_end(tmp_path):
    err = _train(_steady([[], [1.0, 0.0, 0.0]]), tmp_path, 3000, **E2E)
    print('steady Neumann l2 error %.4f (bar 0.02)' % err)
    assert err <= 0.02


def test_steady_robin_end_to_end(tmp_path):
    # u'(1) + u(1) = 0 + 1 = 1 for u = sin(pi x / 2)
    err = _train(_steady([[], [1.0, 1.0, 1.0]]), tmp_path, 3000, **E2E)
    print('steady Robin l2 error %.4f (bar 0.02)' % err)
    assert err <= 0.02


def test_transient_neumann_end_to_end(tmp_path):
    pde = ADPDE(Domain1D(np.array([0.0, 1.0])), diff=KAPPA, vel=0.0, tInterval=[0, 1.0], BCs=[[], [1.0, 0.0, 0.0]],
                IC=lambda x: np.sin(pi * x / 2), cEx=lambda x, t: np.exp(-KAPPA * pi ** 2 * t / 4) * np.sin(pi * x / 2))
    err = _train(pde, tmp_path, 3000, tDiscNum=20, **E2E)
    print('transient Neumann l2 error %.4f (bar 0.05)' % err)
    assert err <= 0.05
