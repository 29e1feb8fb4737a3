"""
GPU tier of the inverse mode (vn_set_coef_learn, vn_get_coefs, vn_set_coefs; `VarNet(learnCoef=...)`): the coefficient gradient of
vn_learnt.hip against the fp64 restatement tests/inverse_ref.py on the ten cases of tests/dedup_term_cases.py -- row-wise on the
automatic route (the two-pass sequence; for integ_num > 128 the two-pass route itself) and on the generic kernels, de-duplicated on
the case's shared-point map (for the EMPTY cases also the map with row-less points) -- that nothing else moves, the Adam step of
the coefficients, snapshot / rollback, the fp64 objective at the device coefficients, every refusal, and two recoveries end to end.
The 4-wave cross-check kernel (VN_KERNEL_FUSED) carries none of the three terms (vn_set_reaction ... refuse it), so it has no
coefficient gradient to check: test_refusals asserts that refusal stays.

Bar per component (tests/inverse_cases.py): |g - g64| <= GRAD_RTOL * max(|g64|, 0.01 S_m).  The worst errors are written to
inverse_parity.json in the directory VN_RECORD_DIR names (default: profile_out/ beside tests/; committed copy:
profiles/inverse_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import inverse_cases as ic
from tests.dedup_term_cases import BIDIMVAL, CASES, DETJ, EMPTY, IDS, empty_map, inputs, terms_of, theta
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import VN_COMM_ID_BYTES, VN_KERNEL_AUTO, VN_KERNEL_FUSED, VN_KERNEL_GENERIC, VNEngine, VNError
from varnet_amd.varnet import VarNet

pytestmark = pytest.mark.gpu

pi = np.pi
RECORD = {}
ALL9 = [1] * 9
THREE = [0, 1, 0, 1, 0, 0, 1, 0, 0]                                      # c2, f1, d0
ROUTES = ['auto', 'generic', 'dedup']


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'inverse_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


# ---- engine-level helpers -------------------------------------------------------------------------------------------
def make_engine(i, variant='all', route='auto', empty=False, optimizer='adam', lr=0.001, learn_first=None, coefs=None):
    """An engine of CASES[i] with the terms of `variant`; route 'dedup' adds the case's shared-point map.  learn_first: a
    (mask, init) registered BEFORE the terms; coefs: nine values the terms are registered with instead of the case's."""
    d_in, dim, widths, q, n_k, U, nB, bDof, source, integW, td, act = CASES[i][:12]
    d = inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW, activationFun=act, optimizer_name=optimizer,
                   learning_rate=lr, kernel=VN_KERNEL_GENERIC if route == 'generic' else VN_KERNEL_AUTO)
    eng.set_params(theta(i))
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, BIDIMVAL)
    eng.set_weights(d['w'])
    eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=DETJ)
    if learn_first is not None:
        eng.set_coef_learn(learn_first[0], learn_first[1], lr=0.01)
    nldiff, nlflux, reaction = terms_of(i, variant)
    c = ic.coefs_of(i, variant) if coefs is None else np.asarray(coefs, dtype=np.float64)
    if reaction is not None:
        eng.set_reaction(0, reaction[0], c[0:3])
    if nlflux is not None:
        eng.set_nlflux(0, nlflux[0], c[3:6])
    if nldiff is not None:
        eng.set_nldiff(0, nldiff[0], c[6:9])
    if route == 'dedup':
        Xu, rowptr = empty_map(i) if empty else (d['Xu'], d['rowptr'])
        eng.set_dedup(0, Xu, d['uid'], rowptr, d['rowidx'])
    return eng


def grad_of(eng):
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    return gb.cpu().numpy().copy()


def loss_field(eng):
    out, lv = eng.eval_loss(0, lossVec=True)
    return np.asarray(out, dtype=np.float64), lv.cpu().numpy().copy()


def check_coef_grad(tag, gc, i, variant):
    """gc against the fp64 reference within the bar, printed and recorded before the assertion."""
    _, _, g64, S = ic.reference64(i, variant)
    on = ic.present(variant)
    bar = ic.bars(g64, S)
    err = np.abs(gc - g64)
    rel = np.where(on, err / np.where(bar > 0, bar, 1.0), 0.0)
    RECORD[tag] = {'worst_err_over_bar': float(rel.max()), 'worst_component': ic.NAMES[int(rel.argmax())],
                   'worst_rel_of_g': float(np.max(np.where(on, err / np.maximum(np.abs(g64), 1e-300), 0.0))),
                   'worst_rel_of_S': float(np.max(np.where(on, err / np.maximum(S, 1e-300), 0.0)))}
    print('inverse %s: %s' % (tag, json.dumps(RECORD[tag], sort_keys=True)))
    assert np.all(np.isfinite(gc))
    assert np.all(gc[~on] == 0.0), (tag, gc)
    assert np.all(err[on] <= bar[on]), (tag, gc, g64, bar)


def gradient_checks(i, variant, route, empty=False):
    tag = '%s/%s/%s%s' % (IDS[i], variant, route, '/empty_points' if empty else '')
    eng = make_engine(i, variant, route, empty)
    try:
        c0 = ic.coefs_of(i, variant)
        g_off, (l_off, lv_off) = grad_of(eng), loss_field(eng)
        eng.set_coef_learn(ALL9, c0, lr=0.01)
        g_on, (l_on, lv_on) = grad_of(eng), loss_field(eng)
        # nothing else moves: loss pieces, lossVec and the theta-gradient are bitwise those of learning off
        assert np.array_equal(g_on, g_off), tag
        assert np.array_equal(l_on, l_off) and np.array_equal(lv_on, lv_off), tag
        coef, gc = eng.get_coefs(grad=True)
        assert np.array_equal(coef, c0.astype(np.float32).astype(np.float64))
        check_coef_grad(tag, gc, i, variant)
        grad_of(eng)
        assert np.array_equal(eng.get_coefs(grad=True)[1], gc), tag          # two evaluations: the same nine doubles
        if variant == 'all':
            eng.set_coef_learn(THREE, c0, lr=0.01)
            assert np.array_equal(grad_of(eng), g_off), tag
            g3 = eng.get_coefs(grad=True)[1]
            m3 = np.array(THREE, dtype=bool)
            assert np.all(g3[~m3] == 0.0) and np.array_equal(g3[m3], gc[m3]), (tag, g3, gc)
        eng.set_coef_learn(None)
        assert np.array_equal(grad_of(eng), g_off), tag                       # learning off again: the parent's bits
        with pytest.raises(VNError, match='error 3: no learnt coefficients'):
            eng.get_coefs()
    finally:
        eng.close()


# ---- 1. the coefficient gradient ------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_coefficient_gradient(i, route):
    gradient_checks(i, 'all', route)


@pytest.mark.parametrize('i', EMPTY, ids=[IDS[k] for k in EMPTY])
def test_coefficient_gradient_with_rowless_points(i):
    gradient_checks(i, 'all', 'dedup', empty=True)


@pytest.mark.parametrize('route', ['auto', 'dedup'])
@pytest.mark.parametrize('variant', ['d', 'flux', 'react'])
@pytest.mark.parametrize('i', [0, 6], ids=[IDS[0], IDS[6]])
def test_each_term_alone(i, variant, route):
    """A batch that carries one term: the entries of the other two read back 0 although they are masked."""
    gradient_checks(i, variant, route)


def test_routes_taken():
    """The automatic route of the cases with integ_num > 128 is the two-pass route; GENERIC is the generic kernels."""
    for i in (2, 4):
        eng = make_engine(i)
        try:
            assert eng.kernel_path()[1] == 1, IDS[i]
        finally:
            eng.close()
    eng = make_engine(0, route='generic')
    try:
        assert eng.kernel_path()[0] == VN_KERNEL_GENERIC
    finally:
        eng.close()


def test_zero_initial_guess_trains():
    """c = (0, 0, 0) as the initial guess: the term stays registered (the 'equal to the off values' shortcut does not fire for a
    term with a mask entry) and its gradient is the reference's at c = 0."""
    i = 0
    c0 = np.zeros(9)
    c0[6] = 1.0
    mask = [1, 0, 0, 0, 0, 0, 0, 0, 0]
    for route in ('auto', 'dedup'):
        eng = make_engine(i, 'react', route, learn_first=(mask, c0), coefs=c0)
        try:
            grad_of(eng)
            gc = eng.get_coefs(grad=True)[1]
            _, _, g64, S = ic.evaluate(i, 'react', coef=c0)
            print('zero guess %s: g %.6e g64 %.6e' % (route, gc[0], g64[0]))
            assert g64[0] != 0.0 and gc[0] != 0.0
            assert abs(gc[0] - g64[0]) <= ic.bars(g64, S)[0]
            assert np.all(gc[1:] == 0.0)
        finally:
            eng.close()


def test_next_to_flux_rows_periodic_pairs_and_observations():
    """The boundary passes do not contain the coefficients: with all three registered the coefficient gradient is what it was."""
    i = 0
    d_in, dim = CASES[i][0], CASES[i][1]
    rng = np.random.default_rng(31)
    for route in ('auto', 'dedup'):
        eng = make_engine(i, 'all', route)
        try:
            eng.set_coef_learn(ALL9, ic.coefs_of(i, 'all'), lr=0.01)
            grad_of(eng)
            before = eng.get_coefs(grad=True)[1]
            nrm = rng.standard_normal((17, dim)).astype(np.float32)
            eng.set_flux_bc(rng.uniform(-1, 1, (17, d_in)).astype(np.float32), nrm, rng.uniform(0, 1, 17).astype(np.float32),
                            rng.standard_normal(17).astype(np.float32), BIDIMVAL)
            eng.set_periodic(rng.uniform(-1, 1, (22, d_in)).astype(np.float32), rng.standard_normal((22, dim)).astype(np.float32), 1.0,
                             BIDIMVAL)
            eng.set_observations(rng.uniform(-1, 1, (33, d_in)).astype(np.float32), rng.standard_normal(33).astype(np.float32), weight=2.0)
            grad_of(eng)
            gc = eng.get_coefs(grad=True)[1]
            check_coef_grad('%s/all/%s/edge_passes' % (IDS[i], route), gc, i, 'all')
            assert np.array_equal(gc, before)
        finally:
            eng.close()


# ---- 2. the step ----------------------------------------------------------------------------------------------------------
STEP_MASK = [1, 0, 1, 0, 1, 0, 1, 1, 0]
STEP_LR = 0.1     # 1e-6 of lr = 1e-7: above the half-ulp of an fp32 coefficient of magnitude <= 1.2 (6e-8) plus the fp32 step arithmetic


@pytest.mark.parametrize('route', ['auto', 'dedup'])
@pytest.mark.parametrize('i', [0, 6], ids=[IDS[0], IDS[6]])
def test_train_step_is_adam_on_the_masked_coefficients(i, route):
    """One vn_train_step from zero slots moves each masked coefficient as Adam in fp64 says (the engine's beta1, beta2, eps as
    the kernel receives them, in fp32; step 1), within 1e-6 of lr; unmasked ones keep their bits; a bound that is hit is held exactly."""
    c0 = ic.coefs_of(i, 'all')
    c32 = c0.astype(np.float32).astype(np.float64)
    lo, hi = np.full(9, -np.inf), np.full(9, np.inf)
    lo[6], hi[6] = c0[6] - 0.004, c0[6] + 0.004                         # the first Adam step is lr in size: d0 hits one of them
    eng = make_engine(i, 'all', route)
    try:
        eng.set_coef_learn(STEP_MASK, c0, lo, hi, lr=STEP_LR)
        grad_of(eng)
        gc = eng.get_coefs(grad=True)[1]
        eng.train_step(0)
        torch.cuda.synchronize()
        got, gc2 = eng.get_coefs(grad=True)
        assert np.array_equal(gc, gc2) and eng.step == 1
        # the hyper-parameters as the kernel receives them: beta1, beta2, eps and lr_t (formed in double) rounded to fp32 --
        # 1 - fp32(0.999) is 1.3e-5 away from 0.001, which alone is 6.4e-6 of the step
        b1, b2, eps = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8))
        gi = gc.astype(np.float32).astype(np.float64)
        lr_t = float(np.float32(STEP_LR * np.sqrt(1 - 0.999) / (1 - 0.9)))
        want = c32 - lr_t * ((1 - b1) * gi) / (np.sqrt((1 - b2) * gi * gi) + eps)
        for m in range(9):
            print('step %s/%s %s: %.9g -> %.9g (Adam %.9g)' % (IDS[i], route, ic.NAMES[m], c32[m], got[m], want[m]))
            if not STEP_MASK[m]:
                assert got[m] == c32[m]
            elif m == 6:
                bound = lo[6] if gi[6] > 0 else hi[6]
                assert got[m] == float(np.float32(bound))
            else:
                assert gi[m] != 0.0 and abs(got[m] - want[m]) <= 1e-6 * STEP_LR, (ic.NAMES[m], got[m], want[m])
        # grad + apply takes the same step
        eng.set_coef_learn(STEP_MASK, c0, lo, hi, lr=STEP_LR)
        eng.set_params(theta(i))
        eng.grad(0)
        eng.apply()
        torch.cuda.synchronize()
        # (the step counter went on: lr_t of step 2 with fresh slots differs, so compare against the formula, not the bits)
        t = 2.0
        lr2 = float(np.float32(STEP_LR * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)))
        got2 = eng.get_coefs()
        want2 = c32 - lr2 * ((1 - b1) * gi) / (np.sqrt((1 - b2) * gi * gi) + eps)
        for m in (0, 2, 4, 7):
            assert abs(got2[m] - want2[m]) <= 1e-6 * STEP_LR, (ic.NAMES[m], got2[m], want2[m])
    finally:
        eng.close()


def _state(eng):
    torch.cuda.synchronize()
    return np.asarray(eng.export_state()).copy(), eng.get_coefs()


@pytest.mark.parametrize('route', ['auto', 'dedup'])
def test_train_epoch_snapshot_and_rollback(route):
    """vn_train_epoch over [0, 0, 0, 0] is bitwise four single steps, parameters, slots and coefficients; snapshot -> three steps
    -> rollback restores coefficients, their slots and the step counter bitwise (the replayed steps end in the same bits);
    vn_set_coefs invalidates the snapshot."""
    i = 6
    c0 = ic.coefs_of(i, 'all')
    a, b = make_engine(i, 'all', route, lr=0.01), make_engine(i, 'all', route, lr=0.01)
    try:
        for e in (a, b):
            e.set_coef_learn(ALL9, c0, lr=0.02)
        a.train_epoch([0, 0, 0, 0])
        for _ in range(4):
            b.train_step(0)
        sa, ca = _state(a)
        sb, cb = _state(b)
        assert np.array_equal(sa, sb) and np.array_equal(ca, cb)
        assert not np.array_equal(ca, c0.astype(np.float32).astype(np.float64))
        a.state_snapshot()
        a.train_epoch([0, 0, 0])
        s3, c3 = _state(a)
        assert a.step == 7 and not np.array_equal(c3, ca)
        a.state_rollback()
        s0, cr = _state(a)
        assert a.step == 4 and np.array_equal(s0, sa) and np.array_equal(cr, ca)
        a.train_epoch([0, 0, 0])                                           # same slots, same counter: the same three steps
        s3b, c3b = _state(a)
        assert np.array_equal(s3b, s3) and np.array_equal(c3b, c3)
        a.state_snapshot()
        a.set_coefs(c0)
        with pytest.raises(VNError, match='error 3: no snapshot to roll back to'):
            a.state_rollback()
    finally:
        a.close()
        b.close()


# ---- 3. the fp64 objective ------------------------------------------------------------------------------------------------
def test_objective_f64_at_the_device_coefficients():
    """After vn_set_coefs(c') vn_objective_f64 equals that of an engine registered with c' and learning off, at the bars of
    tests/test_obj64_gpu.py (loss pieces 1e-12, gradient 1e-11 of its maximum)."""
    i = 1
    c0 = ic.coefs_of(i, 'all')
    c1 = (c0 * np.array([1.5, 0.5, -1.0, 0.75, 2.0, 1.25, 1.5, -0.5, 2.0])).astype(np.float32).astype(np.float64)
    a, b = make_engine(i, 'all'), make_engine(i, 'all', coefs=c1)
    try:
        a.set_coef_learn(ALL9, c0, lr=0.01)
        out0, g0 = a.objective64(0)[:2]
        a.set_coefs(c1)
        out_a, g_a = a.objective64(0)[:2]
        out_b, g_b = b.objective64(0)[:2]
        g_a, g_b, g0 = (x.cpu().numpy() for x in (g_a, g_b, g0))
        assert not np.allclose(out0[0], out_a[0], rtol=1e-6)               # the coefficients count
        for k in range(4):
            assert abs(out_a[k] - out_b[k]) <= 1e-12 * abs(out_b[k]), (k, out_a[k], out_b[k])
        assert np.max(np.abs(g_a - g_b)) <= 1e-11 * np.max(np.abs(g_b))
    finally:
        a.close()
        b.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals():
    i = 6
    c0 = ic.coefs_of(i, 'all')
    inf = np.full(9, np.inf)
    for opt, word in (('rmsprop', 'an RMSProp'), ('lbfgs', 'an L-BFGS')):
        eng = make_engine(i, 'all', optimizer=opt)
        try:
            with pytest.raises(VNError, match='error 5: vn_set_coef_learn on %s engine' % word):
                eng.set_coef_learn(ALL9, c0, lr=0.01)
        finally:
            eng.close()
    eng = make_engine(i, 'all')
    try:
        n_k = CASES[i][4]
        bad = c0.copy()
        bad[4] = np.nan
        with pytest.raises(VNError, match='error 1: initial coefficient 4'):
            eng.set_coef_learn(ALL9, bad, lr=0.01)
        lo = -inf.copy()
        lo[2] = 1.0
        hi = inf.copy()
        hi[2] = 0.5
        with pytest.raises(VNError, match='error 1: bounds of coefficient 2'):
            eng.set_coef_learn(ALL9, c0, lo, hi, lr=0.01)
        for lr in (0.0, -1.0, float('nan')):
            with pytest.raises(VNError, match='error 1: coefficient learning rate'):
                eng.set_coef_learn(ALL9, c0, lr=lr)
        with pytest.raises(VNError, match='error 3: no learnt coefficients'):
            eng.set_coefs(c0)
        # per-test-function weights first, learning second -- and the other way round
        eng.set_tf_weights(0, np.ones(n_k, dtype=np.float32))
        with pytest.raises(VNError, match=r'error 5: learnt coefficients \(vn_set_coef_learn\) next to per-test-function loss weights'):
            eng.set_coef_learn(ALL9, c0, lr=0.01)
        eng.set_tf_weights(0, None)
        eng.set_coef_learn(ALL9, c0, lr=0.01)
        with pytest.raises(VNError, match='error 5: learnt coefficients .* next to per-test-function loss weights'):
            eng.set_tf_weights(0, np.ones(n_k, dtype=np.float32))
        if CASES[i][10]:
            with pytest.raises(VNError, match='error 5: learnt coefficients .* next to per-test-function loss weights'):
                eng.set_causal(0, np.zeros(n_k, dtype=np.int32), 1, 1.0)
        with pytest.raises(VNError, match='error 5: vn_comm_init while coefficients are learnt'):
            eng.comm_init(0, 1, bytes(VN_COMM_ID_BYTES))
        with pytest.raises(VNError, match='error 1: coefficient 0'):
            eng.set_coefs(bad * np.array([np.inf] + [1.0] * 8))
        grad_of(eng)                                                        # the engine still works
    finally:
        eng.close()
    # the 4-wave cross-check geometry carries none of the terms: nothing there for the coefficients to act on
    d_in, dim, widths, q, n_k, U, nB, bDof, source, integW, td, act = CASES[0][:12]
    d = inputs(0)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW, activationFun=act, kernel=VN_KERNEL_FUSED)
    try:
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=DETJ)
        with pytest.raises(VNError, match='error 5: the reaction term is not built for VN_KERNEL_FUSED'):
            eng.set_reaction(0, d['rate'], [1.0, -1.0, 0.5])
    finally:
        eng.close()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
KAPPA, T_END = 0.1, 0.5
EPOCHS = 3000


def sensors(u_star, seed=0):
    rng = np.random.default_rng(seed)
    x, t = rng.uniform(0, 1, 64), rng.uniform(0, T_END, 64)
    return np.column_stack([x, t]), u_star(x, t)


def _train(pde_kw, u_star, folder, **vn_kw):
    np.random.seed(0)
    pde = ADPDE(Domain1D(np.array([0.0, 1.0])), diff=KAPPA, vel=0.0, tInterval=[0, T_END], IC=lambda x: np.sin(pi * x), cEx=u_star,
                **pde_kw)
    vn = VarNet(pde, layerWidth=[20], activationFun='tanh', discNum=40, bDiscNum=None, tDiscNum=20, learning_rate=0.01,
                observations=sensors(u_star), **vn_kw)
    vn.train(str(folder), weight=[10.0, 10.0, 1.0], epochNum=EPOCHS, tol=0.0, saveFreq=EPOCHS, verbose=False)
    out = vn.coefficients(), vn.obsMisfit(), vn.residual()[2]
    vn.engine.close()
    return out


def test_recovers_a_decay_rate(tmp_path):
    """c_t = kappa c_xx + c1 c, truth c1* = -1, u* = exp(-(kappa pi^2 + 1) t) sin(pi x); guess c1 = -0.2.  Required: the error of
    c1 falls to a third of the guess's, and the misfit ends below that of the twin trained with c1 frozen at the guess.
    Measured on one MI355X (seed fixed, 3 000 epochs): c1 = -0.800; misfit 4.43e-4, twin 8.19e-3."""
    u_star = lambda x, t: np.exp(-(KAPPA * pi ** 2 + 1.0) * t) * np.sin(pi * x)
    guess, truth = -0.2, -1.0
    coef, misfit, err = _train(dict(reaction=(1.0, [guess, 0.0, 0.0])), u_star, tmp_path / 'learn', learnCoef={'reaction': [1, 0, 0]})
    _, misfit_twin, err_twin = _train(dict(reaction=(1.0, [guess, 0.0, 0.0])), u_star, tmp_path / 'twin')
    c1 = coef['reaction'][0]
    RECORD['end_to_end/decay_rate'] = {'c1': c1, 'misfit': misfit, 'misfit_twin': misfit_twin, 'l2_error': float(err),
                                       'l2_error_twin': float(err_twin), 'epochs': EPOCHS}
    print('decay rate: c1 %.4f (truth %.1f, guess %.1f); misfit %.4e, frozen twin %.4e; l2 error %.4f, twin %.4f'
          % (c1, truth, guess, misfit, misfit_twin, err, err_twin))
    assert coef['reaction'][1:] == [0.0, 0.0]
    assert abs(c1 - truth) <= abs(guess - truth) / 3.0
    assert misfit < misfit_twin


def test_recovers_a_diffusivity(tmp_path):
    """c_t = div(kappa d0 grad c), truth d0* = 1, u* = exp(-kappa pi^2 t) sin(pi x); guess d0 = 3, bounded below by 0.05.
    Measured on one MI355X (seed fixed, 3 000 epochs): d0 = 0.775; misfit 1.33e-3, twin 4.18e-2."""
    u_star = lambda x, t: np.exp(-KAPPA * pi ** 2 * t) * np.sin(pi * x)
    guess, truth = 3.0, 1.0
    coef, misfit, err = _train(dict(nldiff=[guess, 0.0, 0.0]), u_star, tmp_path / 'learn', learnCoef={'nldiff': [1, 0, 0]},
                               coefBounds={'nldiff': [(0.05, None), None, None]})
    _, misfit_twin, err_twin = _train(dict(nldiff=[guess, 0.0, 0.0]), u_star, tmp_path / 'twin')
    d0 = coef['nldiff'][0]
    RECORD['end_to_end/diffusivity'] = {'d0': d0, 'misfit': misfit, 'misfit_twin': misfit_twin, 'l2_error': float(err),
                                        'l2_error_twin': float(err_twin), 'epochs': EPOCHS}
    print('diffusivity: d0 %.4f (truth %.1f, guess %.1f); misfit %.4e, frozen twin %.4e; l2 error %.4f, twin %.4f'
          % (d0, truth, guess, misfit, misfit_twin, err, err_twin))
    assert coef['nldiff'][1:] == [0.0, 0.0]
    assert abs(d0 - truth) <= abs(guess - truth) / 3.0
    assert misfit < misfit_twin


def test_loss_lag_blocks_end_in_the_same_coefficients(tmp_path):
    """train(lossLag=8) ends in the coefficients (and the epoch) of lossLag=1 when the tolerance is met inside a block: the
    rollback carries the coefficient state."""
    u_star = lambda x, t: np.exp(-(KAPPA * pi ** 2 + 1.0) * t) * np.sin(pi * x)

    def run(folder, lag, tol, epochs):
        np.random.seed(0)
        pde = ADPDE(Domain1D(np.array([0.0, 1.0])), diff=KAPPA, vel=0.0, tInterval=[0, T_END], IC=lambda x: np.sin(pi * x),
                    reaction=(1.0, [-0.2, 0.0, 0.0]))
        vn = VarNet(pde, layerWidth=[20], activationFun='tanh', discNum=40, bDiscNum=None, tDiscNum=20, learning_rate=0.01,
                    observations=sensors(u_star), learnCoef={'reaction': [1, 0, 0]})
        res = vn.train(str(folder), weight=[10.0, 10.0, 1.0], epochNum=epochs, tol=tol, saveFreq=1, verbose=False, lossLag=lag)
        out = vn.coefficients()['reaction'][0], vn.engine.step, vn.engine.get_params(), list(res.loss)
        vn.engine.close()
        return out

    _, _, _, losses = run(tmp_path / 'probe', 1, 0.0, 30)
    tol = float(losses[20]) * (1.0 + 1e-9)
    c_1, step_1, th_1, _ = run(tmp_path / 'lag1', 1, tol, 60)
    c_8, step_8, th_8, _ = run(tmp_path / 'lag8', 8, tol, 60)
    print('lossLag: stopped after %d / %d steps, c1 %.9g / %.9g' % (step_1, step_8, c_1, c_8))
    assert 1 < step_1 < 60 and step_1 == step_8
    assert c_1 == c_8 and c_1 != -0.2 and np.array_equal(th_1, th_8)
