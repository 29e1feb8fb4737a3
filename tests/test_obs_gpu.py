"""
GPU tier of the observation term (vn_set_observations, `VarNet(..., observations=...)`): parity of the loss, the misfit and the
gradient against the fp64 restatement (tests/obs_ref.py) on every route the kernels' range maps to, with and without a derivative
part, next to flux rows and periodic pairs, with a de-duplication map, the composition of the step's entry points, the
register-then-clear contract, the weight, the fp64 objective, the L-BFGS invalidation, the refusals, and a heat equation whose
initial condition is withheld and recovered from sensors.

The cases are the five shapes of tests/test_periodic_gpu.py::CASES with nO observations in place of nP pairs (tests/obs_cases.py:
their layouts, the weight rule lambda = (loss without the term) / O, and the shared reference); tests/test_obs_host.py asserts from
the reference alone that every case feels the term.  The worst figures are written to obs_parity.json in the directory
VN_RECORD_DIR names (default: profile_out/ beside tests/; the committed copy: profiles/obs_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests import obs_cases
from tests.gradcheck import assert_grad_close, block_errors
from tests.obs_cases import CASES, IDS, ref_of
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL
from tests.test_flux_bc_gpu import flux_rows
from tests.test_obj64_gpu import GRAD_BAR, LOSS_BAR, LVEC_BAR
from tests.test_periodic_gpu import BDV, THETA_SCALE, periodic_rows, perturbed
from tests import flux_ref
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import VN_KERNEL_AUTO, VN_KERNEL_FUSED, VN_KERNEL_GENERIC, VNEngine, VNError
from varnet_amd.varnet import VarNet

pytestmark = pytest.mark.gpu

pi = np.pi
KEYS = ['loss', 'BCloss', 'ICloss', 'varLoss']
KNAME = {VN_KERNEL_AUTO: 'auto', VN_KERNEL_GENERIC: 'generic'}
RECORD = {}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'obs_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True, default=str)
    except OSError:
        pass


def register(eng, obs, lam):
    eng.set_observations(obs['X'], obs['value'], q=obs['q'], dir=obs['dir'], rowptr=obs['rowptr'], wgt=obs['wgt'], weight=lam)


def setup(ci, kernel=VN_KERNEL_AUTO, optimizer='adam', case=None, xcheck=False):
    """An engine on CASES[ci] (or `case`, of the same shape) at the parameters of the shared reference, without observations."""
    d_in, dim, widths, q, n_k, nB, bDof, nO, td, act, integW = case or CASES[ci]
    d = obs_cases.case_data(ci)
    eng = VNEngine(dim, d_in, widths, td, q, integWflag=integW, kernel=kernel, activationFun=act, xcheck=xcheck,
                   optimizer_name=optimizer)
    eng.init_params(seed=3)
    flat = perturbed(eng.get_params())
    eng.set_params(flat)
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=n_k, detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, BDV)
    eng.set_weights(d['w'])
    return eng, flat, d


def evaluate(eng):
    """(eval_loss components, misfit after eval_loss or None, gradient buffer as fp64, misfit after grad or None)."""
    out, _ = eng.eval_loss(0)
    have = eng._keep.get('obs') is not None
    m0 = eng.obs_misfit() if have else None
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    m1 = eng.obs_misfit() if have else None
    return np.array(out), m0, gb.cpu().numpy().astype(np.float64), m1


def check_parity(ci, eng, flat, d, with_dir, plain, what):
    case = CASES[ci]
    d_in, dim, widths, td = case[0], case[1], case[2], case[8]
    flat0, obs, lam, ref, gref, ref0, gref0 = ref_of(ci, with_dir, plain)
    assert np.array_equal(flat0, flat)                                  # the shared reference is this engine's
    out0, _, g0, _ = evaluate(eng)                                      # without the registration
    register(eng, obs, lam)
    out, m0, g, m1 = evaluate(eng)
    P = eng.P
    rec = RECORD.setdefault(what, {})
    rec.update({'lambda': lam, 'O_ref': ref['obs'],
                'loss_eval': abs(out[0] - ref['loss']) / abs(ref['loss']), 'loss_grad': abs(g[P] - ref['loss']) / abs(ref['loss']),
                'misfit_eval': abs(m0 - ref['obs']) / ref['obs'], 'misfit_grad': abs(m1 - ref['obs']) / ref['obs']})
    print('obs %s: loss eval %.9e grad %.9e ref %.9e; O eval %.9e grad %.9e ref %.9e'
          % (what, out[0], g[P], ref['loss'], m0, m1, ref['obs']))
    assert abs(out[0] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7, (what, 'eval', out[0], ref['loss'])
    assert abs(g[P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7, (what, 'grad', g[P], ref['loss'])
    # BC, IC and var are those of the run without observations, bit for bit, and so against the reference
    assert np.array_equal(out[1:], out0[1:]) and np.array_equal(g[P + 1:P + 4], g0[P + 1:P + 4])
    for k in (1, 2, 3):
        assert abs(out[k] - ref[KEYS[k]]) <= LOSS_RTOL * abs(ref[KEYS[k]]) + 1e-7, (what, KEYS[k], out[k], ref[KEYS[k]])
    for m in (m0, m1):
        assert abs(m - ref['obs']) <= LOSS_RTOL * ref['obs'], (what, 'misfit', m, ref['obs'])
    grec = {}
    try:
        assert_grad_close(g[:P], gref, d_in, widths, GRAD_RTOL, dim=dim, td=td, what=what, rec=grec,
                          g32=lambda: obs_cases.reference(ci, flat, d, obs, lam, dtype=torch.float32)[1])
    finally:
        rec['grad'] = grec
        print('obs %s: gradient %s' % (what, grec))
    # the term alone: (gradient with) - (gradient without), against the reference's difference on the full gradient's scale
    errs = block_errors(g[:P] - g0[:P] + gref0, gref, d_in, widths, dim, td)
    rec['term_worst_block'] = max(errs.values())


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_dir', [False, True], ids=['values', 'dir'])
@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('ci', range(len(CASES)), ids=IDS)
def test_obs_parity(ci, kernel, with_dir):
    eng, flat, d = setup(ci, kernel)
    try:
        check_parity(ci, eng, flat, d, with_dir, False, '%s/%s/%s' % (IDS[ci], KNAME[kernel], 'dir' if with_dir else 'values'))
    finally:
        eng.close()


def test_obs_parity_without_q_and_wgt():
    """q = NULL and wgt = NULL (all 1) on the point sensors with rowptr = NULL: every optional array absent."""
    eng, flat, d = setup(1)
    try:
        assert ref_of(1, False, True)[1]['rowptr'] is None
        check_parity(1, eng, flat, d, False, True, '%s/auto/plain' % IDS[1])
    finally:
        eng.close()


def test_obs_parity_with_dedup_map():
    """The de-duplicated formulation (identity point map: every row its own point) carries the observations too."""
    eng, flat, d = setup(3)
    try:
        nT = d['Input'].shape[0]
        idx = torch.arange(nT, dtype=torch.int32)
        eng.set_dedup(0, d['Input'], idx, torch.arange(nT + 1, dtype=torch.int32), idx)
        check_parity(3, eng, flat, d, True, False, 'dedup')
    finally:
        eng.close()


def test_obs_parity_on_crosscheck_fused32():
    eng, flat, d = setup(2, VN_KERNEL_FUSED, xcheck=False)
    try:
        check_parity(2, eng, flat, d, True, False, 'fused32')
    finally:
        eng.close()


# ---- 2. next to flux rows and periodic pairs ---------------------------------------------------------------------------------
def test_obs_next_to_flux_rows_and_periodic_pairs():
    ci = 2
    case = CASES[ci]
    d_in, dim, widths, td, act = case[0], case[1], case[2], case[8], case[9]
    fx = {k: np.asarray(v).astype(np.float32) for k, v in flux_rows(12, d_in, dim, 40).items()}
    pr = periodic_rows(13, d_in, dim, 50)
    flat0, obs, lam, _, _, _, _ = ref_of(ci, True)
    eng, flat, d = setup(ci)
    try:
        eng.set_flux_bc(fx['X'], fx['normal'], fx['coef'], fx['label'], BDV)
        eng.set_periodic(pr['X'], pr['dir'], 1.0, BDV)
        out0, _, g0, _ = evaluate(eng)
        register(eng, obs, lam)
        out, m0, g, m1 = evaluate(eng)

        def reference(dtype):
            f = np.float64 if dtype == torch.float64 else np.float32
            prc = dict(X=pr['X'].astype(f), dir=pr['dir'].astype(f), gamma=1.0)
            res, gr = obs_cases.reference(ci, flat, d, obs, lam, dtype=dtype, periodic=prc)
            F, gF, _ = flux_ref.flux_term(flat.astype(f), d_in, widths, dim, fx['X'].astype(f), fx['normal'].astype(f),
                                          fx['coef'].astype(f), fx['label'].astype(f), BDV, act, dtype)
            res = dict(res)
            res['BCloss'] = res['BCloss'] + F
            res['loss'] = res['loss'] + d['w'][0] * F
            return res, gr + d['w'][0] * gF
        ref, gref = reference(torch.float64)
        P = eng.P
        print('obs+flux+periodic: loss eval %.9e grad %.9e ref %.9e; O %.9e ref %.9e' % (out[0], g[P], ref['loss'], m1, ref['obs']))
        assert lam * ref['obs'] > 0.1 * ref['loss']
        for k, key in enumerate(KEYS):
            assert abs(out[k] - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, ('eval', key, out[k], ref[key])
            assert abs(g[P + k] - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, ('grad', key, g[P + k], ref[key])
        assert np.array_equal(out[1:], out0[1:]) and np.array_equal(g[P + 1:P + 4], g0[P + 1:P + 4])
        assert abs(m0 - ref['obs']) <= LOSS_RTOL * ref['obs'] and abs(m1 - ref['obs']) <= LOSS_RTOL * ref['obs']
        assert_grad_close(g[:P], gref, d_in, widths, GRAD_RTOL, dim=dim, td=td, what='obs+flux+periodic',
                          g32=lambda: reference(torch.float32)[1])
    finally:
        eng.close()


# ---- 3., 4. the step's entry points ------------------------------------------------------------------------------------------
def _theta_after(eng, state, fn):
    eng.import_state(state)
    fn()
    torch.cuda.synchronize()
    return eng.get_params()


def test_train_step_equals_grad_then_apply():
    """train_step folds the update into the gradient reduction; grad + apply runs it as its own kernel.  Their relation is
    measured first without observations, then required to hold with them: an observation gradient that missed the fused update
    would move theta by about one Adam step (~lr) on every parameter."""
    ci = 2
    _, obs, lam, _, _, _, _ = ref_of(ci, True)
    eng, flat, d = setup(ci)
    try:
        s0 = eng.export_state()
        gap = []
        for with_rows in (False, True):
            if with_rows:
                register(eng, obs, lam)
            a = _theta_after(eng, s0, lambda: eng.train_step(0))
            b = _theta_after(eng, s0, lambda: (eng.grad(0), eng.apply()))
            assert np.max(np.abs(a - flat)) > 1e-4                       # the step moved theta
            gap.append(float(np.max(np.abs(a - b))))
        bar = max(2.0 * gap[0], 1e-6)
        print('train_step vs grad + apply: gap without observations %.3e, with %.3e, bar %.3e' % (gap[0], gap[1], bar))
        assert gap[1] <= bar, gap
    finally:
        eng.close()


def test_train_epoch_is_four_single_steps():
    ci = 3
    case = CASES[ci]
    _, obs, lam, _, _, _, _ = ref_of(ci, True)
    eng, flat, d = setup(ci)
    try:
        register(eng, obs, lam)
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


# ---- 5. register-then-clear, repeatability, the weight -----------------------------------------------------------------------
@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
def test_register_then_clear_is_bitwise_untouched(kernel):
    ci = 2
    _, obs, lam, _, _, _, _ = ref_of(ci, True)
    runs = []
    for touched in (False, True):
        eng, flat, d = setup(ci, kernel)
        try:
            if touched:
                register(eng, obs, lam)
                eng.grad(0)                                             # a step with the observations registered ...
                eng.set_observations(None)                              # ... then cleared
                with pytest.raises(VNError, match='error 3: vn_get_obs_misfit: no observations are registered'):
                    eng.obs_misfit()
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


def test_two_grad_calls_return_the_same_bits():
    ci = 2
    _, obs, lam, _, _, _, _ = ref_of(ci, True)
    eng, flat, d = setup(ci)
    try:
        register(eng, obs, lam)
        gb = eng.bind_grad_buffer()
        bits = []
        for _ in range(2):
            eng.grad(0)
            torch.cuda.synchronize()
            bits.append((gb.cpu().numpy().tobytes(), eng.obs_misfit()))
        assert bits[0] == bits[1]
    finally:
        eng.close()


def test_set_obs_weight_doubles_the_terms_share():
    ci = 3
    case = CASES[ci]
    d_in, dim, widths, td = case[0], case[1], case[2], case[8]
    _, obs, lam, ref, gref, ref0, gref0 = ref_of(ci, True)
    eng, flat, d = setup(ci)
    try:
        register(eng, obs, lam)
        _, _, g1, m1 = evaluate(eng)
        eng.set_obs_weight(2.0 * lam)
        out2, _, g2, m2 = evaluate(eng)
        P = eng.P
        assert m2 == m1                                                 # the unweighted misfit does not see lambda
        want = ref0['loss'] + 2.0 * lam * ref['obs']                    # what the reference says: the term's share doubles
        gwant = gref0 + 2.0 * (gref - gref0)
        print('set_obs_weight(2 lambda): loss eval %.9e grad %.9e ref %.9e' % (out2[0], g2[P], want))
        assert abs(out2[0] - want) <= LOSS_RTOL * want and abs(g2[P] - want) <= LOSS_RTOL * want
        assert abs((g2[P] - g1[P]) - lam * ref['obs']) <= 2 * LOSS_RTOL * want
        assert_grad_close(g2[:P], gwant, d_in, widths, GRAD_RTOL, dim=dim, td=td, what='2 lambda',
                          g32=lambda: obs_cases.reference(ci, flat, d, obs, 2.0 * lam, dtype=torch.float32)[1])
        for bad in (-1.0, float('nan'), float('inf')):
            with pytest.raises(VNError, match='error 1: observations: the weight lambda'):
                eng.set_obs_weight(bad)
    finally:
        eng.close()


# ---- 6. fp64 objective -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci,with_dir', [(1, False), (2, True), (3, True)], ids=['1dt_points', '2dt_long_dir', '2dt_50x5_dir'])
def test_objective64_with_observations(ci, with_dir):
    """The bars of tests/test_obj64_gpu.py: LOSS_BAR on the components and the misfit, LVEC_BAR on the loss field, GRAD_BAR on
    the worst parameter block; identical bits on a second call."""
    case = CASES[ci]
    d_in, dim, widths, td = case[0], case[1], case[2], case[8]
    _, obs, lam, _, _, _, _ = ref_of(ci, with_dir)
    eng, _, d = setup(ci)
    try:
        register(eng, obs, lam)
        th = THETA_SCALE * og.glorot_init(d_in, widths, 2).astype(np.float64)
        th = th + 0.05 * np.random.default_rng(5).standard_normal(th.size)
        ref, gref = obs_cases.reference(ci, th, d, obs, lam)
        assert lam * ref['obs'] > 1e-2 * ref['loss']
        out, g, lv = eng.objective64(0, theta=th, grad=True, lossVec=True)
        O = eng.obs_misfit()
        rec = {key: abs(got - ref[key]) / abs(ref[key]) if ref[key] != 0.0 else abs(got) for got, key in zip(out, KEYS)}
        rec['obs'] = abs(O - ref['obs']) / ref['obs']
        lref = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1)
        rec['lossVec'] = float(np.max(np.abs(lv.cpu().numpy() - lref)) / np.max(np.abs(lref)))
        errs = block_errors(g.cpu().numpy(), gref, d_in, widths, dim, td)
        worst = max(errs, key=errs.get)
        rec['grad_worst_block'] = errs[worst]
        RECORD['obj64/%s' % IDS[ci]] = rec
        print('obj64 obs %s: %s worst block %s %.3e' % (IDS[ci], rec, worst, errs[worst]))
        for key in KEYS + ['obs']:
            assert rec[key] <= LOSS_BAR, (key, rec[key])
        assert rec['lossVec'] <= LVEC_BAR
        assert errs[worst] <= GRAD_BAR, (worst, errs[worst])
        out2, g2, lv2 = eng.objective64(0, theta=th, grad=True, lossVec=True)      # two calls: identical bits
        assert out2 == out and g2.cpu().numpy().tobytes() == g.cpu().numpy().tobytes()
        assert lv2.cpu().numpy().tobytes() == lv.cpu().numpy().tobytes() and eng.obs_misfit() == O
        out3, g3, _ = eng.objective64(0, theta=th, grad=False)                    # loss only: the same scalars
        assert g3 is None and out3 == out and eng.obs_misfit() == O
    finally:
        eng.close()


# ---- 7. L-BFGS ---------------------------------------------------------------------------------------------------------------
def test_lbfgs_restarts_after_set_observations():
    ci = 3
    case = (3, 2, [20, 20, 20], 64, 9, 77, 40, 60, True, 'sigmoid', False)
    obs = obs_cases.obs_rows(ci, True)
    eng, flat, d = setup(ci, optimizer='lbfgs', case=case)
    try:
        for _ in range(4):
            assert eng.lbfgs_step(0)['status'] == 0
        assert eng.lbfgs_step(0)['pairs'] >= 3
        before = eng.eval_loss(0)[0][0]
        register(eng, obs, 0.0)
        eng.eval_loss(0)
        lam = float(np.float32(before / eng.obs_misfit()))                # the rule of the parity cases, at these parameters
        eng.set_obs_weight(lam)
        want = eng.eval_loss(0)[0][0]
        assert want > before * 1.5                                       # the observations changed the objective
        info = eng.lbfgs_step(0)
        assert info['pairs'] == 0, info                                  # a fresh (f, g): the ring was dropped
        assert abs(info['f_k'] - want) <= LOSS_RTOL * abs(want), (info['f_k'], want)
        for _ in range(4):
            assert eng.lbfgs_step(0)['status'] == 0
        assert eng.lbfgs_step(0)['pairs'] >= 3
        eng.set_obs_weight(0.5 * lam)                                    # ... a change of lambda invalidates as well
        want = eng.eval_loss(0)[0][0]
        info = eng.lbfgs_step(0)
        assert info['pairs'] == 0 and abs(info['f_k'] - want) <= LOSS_RTOL * abs(want), (info, want)
        for _ in range(3):
            assert eng.lbfgs_step(0)['status'] == 0
        eng.set_observations(None)                                       # ... and so does clearing
        want = eng.eval_loss(0)[0][0]
        info = eng.lbfgs_step(0)
        assert info['pairs'] == 0 and abs(info['f_k'] - want) <= LOSS_RTOL * abs(want), (info, want)
    finally:
        eng.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    X = np.linspace(0.1, 0.8, 8).reshape(4, 2)
    c = np.ones(4)
    eng = VNEngine(1, 2, [128, 128], True, 16)
    try:
        with pytest.raises(VNError, match='error 5: observations need a network of the hand-written kernels'):
            eng.set_observations(X, c)
        eng.set_observations(None)                                      # clearing is always accepted
    finally:
        eng.close()
    eng = VNEngine(1, 2, [20], True, 16)
    try:
        for lam in (-1.0, float('nan'), float('inf')):
            with pytest.raises(VNError, match='error 1: observations: the weight lambda'):
                eng.set_observations(X, c, weight=lam)
        bad = 'error 1: inconsistent observations: %d violation'
        rp = lambda *a: np.array(a, dtype=np.int32)
        for kw, count in ((dict(rowptr=rp(1, 2, 4)), 1),                 # rowptr[0] != 0
                          (dict(rowptr=rp(0, 2, 3)), 1),                 # rowptr[nO] != n
                          (dict(rowptr=rp(0, 4, 4)), 1),                 # an empty segment
                          (dict(rowptr=rp(0, 5, 4)), 1),                 # not increasing
                          (dict(rowptr=rp(0, 2, 4), value=[1.0, np.nan]), 1),
                          (dict(rowptr=rp(0, 2, 4), wgt=[1.0, -1.0]), 1),
                          (dict(rowptr=rp(0, 2, 4), wgt=[np.inf, 1.0]), 1),
                          (dict(rowptr=rp(0, 2, 4), q=[1.0, np.nan, 1.0, np.inf]), 2),
                          (dict(rowptr=rp(0, 2, 4), dir=[[0.0], [0.0], [np.nan], [0.0]]), 1)):
            kw.setdefault('value', [1.0, 1.0])
            with pytest.raises(VNError, match=bad % count):
                eng.set_observations(X, **kw)
            with pytest.raises(VNError, match='error 3: vn_get_obs_misfit'):      # after an error there is no registration
                eng.obs_misfit()
        Xd, cd = eng.dev(X), eng.dev(c)                                 # at the C level: point sensors need n == nO
        with pytest.raises(VNError, match='error 1: observations: point sensors'):
            eng._ck(eng.lib.vn_set_observations(eng.h, Xd.data_ptr(), None, None, None, cd.data_ptr(), None, 4, 3, 1.0))
        eng.set_observations(X, c, weight=0.0)                          # lambda = 0 is a registration
    finally:
        eng.close()
    pde = ADPDE(Domain1D(np.array([0.0, 1.0])), diff=0.1, vel=0.0, tInterval=[0, 0.5], IC=lambda x: np.zeros([len(x), 1]))
    with pytest.raises(VNError, match='observations need a network of the hand-written kernels'):
        VarNet(pde, layerWidth=[128], discNum=10, bDiscNum=None, tDiscNum=10, observations=(X, c))


# ---- 9. end to end: a heat equation whose initial condition is withheld ------------------------------------------------------
KAPPA, T_END = 0.1, 0.5


def u_star(x, t):
    return np.exp(-KAPPA * pi ** 2 * t) * np.sin(pi * x)


def sensors(seed=0):
    """48 point sensors at random (x, t) and 16 time-averaged sensors (8 points over a window of 0.05, trapezoid weights of the
    mean over the window), values from u*."""
    rng = np.random.default_rng(seed)
    xp, tp = rng.uniform(0, 1, 48), rng.uniform(0, T_END, 48)
    xa, t0 = rng.uniform(0, 1, 16), rng.uniform(0, T_END - 0.05, 16)
    tw = t0[:, None] + np.linspace(0, 0.05, 8)[None, :]
    qw = np.full(8, 1.0 / 7.0)
    qw[[0, -1]] = 0.5 / 7.0                                              # trapezoid rule for (1/0.05) int u dt
    X = np.vstack([np.column_stack([xp, tp]), np.column_stack([np.repeat(xa, 8), tw.reshape(-1)])])
    q = np.concatenate([np.ones(48), np.tile(qw, 16)])
    rowptr = np.concatenate([np.arange(48), 48 + 8 * np.arange(17)])
    value = np.concatenate([u_star(xp, tp), (u_star(xa[:, None], tw) * qw[None, :]).sum(axis=1)])
    return dict(X=X, value=value, rowptr=rowptr, q=q)


def _train_heat(obs, folder):
    np.random.seed(0)
    pde = ADPDE(Domain1D(np.array([0.0, 1.0])), diff=KAPPA, vel=0.0, tInterval=[0, T_END], IC=lambda x: np.zeros([len(x), 1]),
                cEx=u_star)
    vn = VarNet(pde, layerWidth=[20], activationFun='tanh', discNum=40, bDiscNum=None, tDiscNum=20, learning_rate=0.01,
                observations=obs)
    before = vn.obsMisfit() if obs is not None else None
    vn.train(str(folder), weight=[10.0, 0.0, 1.0], epochNum=3000, tol=0.0, saveFreq=3000, verbose=False)
    after = vn.obsMisfit() if obs is not None else None
    err = vn.residual()[2]
    vn.engine.close()
    return err, before, after


def test_heat_equation_with_withheld_initial_condition(tmp_path):
    """c_t = kappa c_xx on [0,1] x [0,0.5], homogeneous Dirichlet ends, the initial condition under zero weight: u = 0 minimises
    the twin's loss exactly, the sensors (obsWeight 1, the default) carry what the initial condition would have.
    Measured on one MI355X (seed fixed): 0.0069 with the sensors, twin 1.0010 (ratio 0.007); misfit 2.596e-1 -> 1.519e-5
    (DESIGN.md section 20)."""
    err, before, after = _train_heat(sensors(), tmp_path / 'obs')
    err_twin, _, _ = _train_heat(None, tmp_path / 'twin')
    RECORD['end_to_end'] = {'error': float(err), 'error_twin': float(err_twin), 'misfit_before': before, 'misfit_after': after}
    print('heat equation, IC withheld: l2 error %.4f with sensors, twin %.4f, ratio %.3f; misfit %.4e -> %.4e'
          % (err, err_twin, err / err_twin, before, after))
    assert err_twin > 0.5                                                # a condition on the problem, not on the code
    assert err <= err_twin / 3.0
    assert after < before
