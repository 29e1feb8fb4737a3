"""
GPU tier of the per-test-function loss weights (vn_set_tf_weights) and the causal time-slab mode (vn_set_causal,
vn_causal_weights, `VarNet(causal=eps)`):

    var = sum_k omega_k l_k,  l_k = detJ_k R_k^2 = lossVec[k] (unweighted everywhere),  omega constant for the gradient;
    causal: omega_k = exp(-eps C_{s_k}),  C_s = sum_{s' < s} mean of l over slab s'.

Static weights: loss components, the unweighted loss field and the gradient against the fp64 restatement (tests/causal_ref.py) on
the automatic and generic routes for all cases, with all three polynomial terms on the automatic route (the order "terms'
seeds, then scale"), and the fp64 objective at the bars of tests/test_obj64_gpu.py.
Causal weights, three separate assertions (the weights are constant for the gradient and a function of the loss field, so no
looser bar is needed): (a) the engine's weights against causal_ref.causal_weights evaluated in fp64 on the engine's OWN loss
field, relative 1e-6 (fp64 accumulation, one exp of an argument in [-1.39, 0], one rounding to fp32; fp64 objective: 1e-12);
(b) against the reference's weights at ln 4 * LVEC_RTOL * (S - 1) * max_k l_k / C_{S-1} + 1e-6, the lossVec bar propagated
through d omega / omega = eps dC; (c) loss and gradient against the reference evaluated with the engine's weights as static
weights, at the unchanged project bars, row-wise and on the de-duplicated step.
Then bitwise repeatability and composition, the registration contract and refusals, the `VarNet` layer, and one training pair.

Bars are the project's own (tests/parity_cases.py: LOSS_RTOL, GRAD_RTOL through tests/gradcheck.assert_grad_close with its fp32
conditioning callback, LVEC_RTOL).  Every parity test first asserts, in the reference, that removing the weights moves varLoss
and the gradient norm by more than 1e-2 relative.

The figures are written to causal_parity.json in the directory VN_RECORD_DIR names (default: profile_out/ beside tests/; the
committed copy: profiles/causal_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import causal_ref, nldiff_cases, nlflux_cases
from tests.causal_cases import (CASES, IDS, LN4, eps_of, inputs, n_slabs, reference, reference64, slabs, static_weights, theta,
                                weights_are_real)
from tests.gradcheck import assert_grad_close, assert_pair_close, block_errors, fp32_deviation
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import VN_KERNEL_AUTO, VN_KERNEL_FUSED, VN_KERNEL_GENERIC, VNEngine, VNError
from varnet_amd.utility import UF
from varnet_amd.varnet import VarNet

pytestmark = pytest.mark.gpu

uf = UF()
pi = np.pi
KEYS = ['loss', 'BCloss', 'ICloss', 'varLoss']
RECORD = {}
KNAME = {VN_KERNEL_AUTO: 'auto', VN_KERNEL_GENERIC: 'generic'}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'causal_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def register_interior(eng, i, batch=0):
    d = inputs(i)[0]
    eng.set_interior(batch, d['Input'], d['gcoef'], d['source'], n_k=CASES[i][4], detJ=d['detJ'], N_rows=d['N_rows'],
                     dNt_rows=d['dNt_rows'])


def register_terms(eng, i, batch=0, which=('react', 'nlflux', 'nldiff')):
    (phi, fcoef), (rate, coef) = nlflux_cases.terms_of(i, 'both')
    for name in which:
        if name == 'react':
            eng.set_reaction(batch, rate, coef)
        elif name == 'nlflux':
            eng.set_nlflux(batch, phi, fcoef)
        else:
            eng.set_nldiff(batch, nldiff_cases.psi(i), nldiff_cases.DIFF)


def register_weights(eng, i, mode, variant='plain', batch=0, eps=None):
    if mode == 'static':
        eng.set_tf_weights(batch, static_weights(i))
    elif mode == 'causal':
        eng.set_causal(batch, slabs(i), n_slabs(i), eps_of(i, variant) if eps is None else eps)


def make_engine(i, kernel=VN_KERNEL_AUTO, mode='none', variant='plain', xcheck=False, optimizer='adam'):
    d_in, dim, widths, q, n_k, nB, bDof, td, act, source, integW, detJvec, rows = CASES[i]
    d, _ = inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW, kernel=kernel, activationFun=act, xcheck=xcheck,
                   optimizer_name=optimizer)
    eng.set_params(theta(i))
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    register_interior(eng, i)
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
    eng.set_weights(d['w'])
    if variant == 'terms':
        register_terms(eng, i)
    register_weights(eng, i, mode, variant)
    return eng


def grad_of(eng, batch=0):
    gb = eng.bind_grad_buffer()
    eng.grad(batch)
    torch.cuda.synchronize()
    return gb.cpu().numpy().astype(np.float64)


def outside_generic(i, kernel):
    """The 128-wide case lies outside the generic kernels: the engine refuses the request (as it does without weights)."""
    if max(CASES[i][2]) > 64 and kernel == VN_KERNEL_GENERIC:
        with pytest.raises(VNError, match='error 5'):
            make_engine(i, kernel)
        return True
    return False


def check_parity(i, eng, ref, tag, g32):
    """eval_loss (with the unweighted lossVec) and grad of batch 0 against ref = (result, gradient); prints and records every
    figure, then asserts."""
    d_in, dim, widths, td = CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][7]
    ref, gref = ref
    out, lv = eng.eval_loss(0, lossVec=True)
    g = grad_of(eng)
    P = eng.P
    rel = lambda got, want: abs(got - want) / max(abs(want), 1e-300) if want != 0.0 else abs(got)
    rec = {'eval_' + k: rel(got, ref[k]) for got, k in zip(out, KEYS)}
    rec.update({'grad_' + k: rel(got, ref[k]) for got, k in zip(g[P:], KEYS)})
    lref = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1)
    rec['lossVec'] = float(np.max(np.abs(lv.cpu().numpy() - lref)) / np.max(np.abs(lref)))
    errs = block_errors(g, gref, d_in, widths, dim, td)
    rec['worst_block'] = max(errs, key=errs.get)
    rec['worst_block_err'] = errs[rec['worst_block']]
    rec['kernel_path'] = list(eng.kernel_path())
    RECORD[tag] = rec
    print('causal %s: %s' % (tag, json.dumps(rec, sort_keys=True)))
    for got, key in zip(out, KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'eval', key, got, ref[key])
    for got, key in zip(g[P:], KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'grad', key, got, ref[key])
    assert rec['lossVec'] <= LVEC_RTOL, (tag, rec['lossVec'])
    assert_grad_close(g[:P], gref, d_in, widths, GRAD_RTOL, dim=dim, td=td, what=tag, g32=g32)
    return g


# ---- static weights -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_static_parity(i, kernel):
    weights_are_real(i, 'static')
    if outside_generic(i, kernel):
        return
    eng = make_engine(i, kernel, 'static')
    try:
        check_parity(i, eng, reference64(i, 'static'), '%s/static/%s' % (IDS[i], KNAME[kernel]),
                     lambda: reference(i, 'static', dtype=torch.float32)[1])
    finally:
        eng.close()


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_static_parity_with_all_three_terms(i):
    """Flux + reaction ('both' of tests/nlflux_cases.py) + D(u): the terms' seed kernels run first, then the scale."""
    weights_are_real(i, 'static', 'terms')
    eng = make_engine(i, mode='static', variant='terms')
    try:
        check_parity(i, eng, reference64(i, 'static', 'terms'), '%s/static/auto/terms' % IDS[i],
                     lambda: reference(i, 'static', 'terms', dtype=torch.float32)[1])
    finally:
        eng.close()


def _objective64_record(i, out, g, lv, ref, gref):
    d_in, dim, widths, td = CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][7]
    rec = {}
    for got, key in zip(out, KEYS):
        rec[key] = abs(got - ref[key]) / max(abs(ref[key]), 1e-300) if ref[key] != 0.0 else abs(got)
    lref = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1)
    rec['lossVec'] = float(np.max(np.abs(lv.cpu().numpy() - lref)) / np.max(np.abs(lref)))
    errs = block_errors(g.cpu().numpy(), gref, d_in, widths, dim, td)
    rec['worst_block'] = max(errs, key=errs.get)
    rec['worst_block_err'] = errs[rec['worst_block']]
    return rec


def _assert_objective64(rec):
    for key in KEYS:
        assert rec[key] <= 1e-12, (key, rec[key])
    assert rec['lossVec'] <= 1e-11, rec['lossVec']
    assert rec['worst_block_err'] <= 1e-11, (rec['worst_block'], rec['worst_block_err'])


OBJ64_CASES = (0, 1, 2, 3, 4, 6)


@pytest.mark.parametrize('i', OBJ64_CASES, ids=[IDS[k] for k in OBJ64_CASES])
def test_static_objective64_parity(i):
    """vn_objective_f64 with static weights at the bars of tests/test_obj64_gpu.py: loss components 1e-12, gradient blocks 1e-11,
    lossVec (unweighted) 1e-11 of its maximum.  Parameters in fp64 (not fp32-representable)."""
    th = theta(i).astype(np.float64) + 1e-3 * np.random.default_rng(6).standard_normal(theta(i).size)
    ref, gref = reference(i, 'static', flat=th)
    ref0, g0 = reference(i, 'none', flat=th)
    assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss'])
    assert np.linalg.norm(gref - g0) > 1e-2 * np.linalg.norm(gref)
    eng = make_engine(i, mode='static')
    try:
        out, g, lv = eng.objective64(0, theta=th, grad=True, lossVec=True)
        rec = _objective64_record(i, out, g, lv, ref, gref)
        RECORD['%s/static/objective64' % IDS[i]] = rec
        print('causal static objective64 %s: %s' % (IDS[i], json.dumps(rec, sort_keys=True)))
        _assert_objective64(rec)
        out2, _, _ = eng.objective64(0, theta=th, grad=False)            # loss-only form, no caller lossVec: same bits
        assert out2 == out
    finally:
        eng.close()


# ---- causal weights -------------------------------------------------------------------------------------------------
def weights_bar(i, variant='plain'):
    """(b): ln 4 * LVEC_RTOL * (S - 1) * max_k l_k / C_{S-1} + 1e-6, from the reference."""
    lv = reference64(i, 'none', variant)[0]['lossVec'].reshape(-1)
    C = LN4 / eps_of(i, variant)
    return LN4 * LVEC_RTOL * (n_slabs(i) - 1) * float(np.max(lv)) / C + 1e-6


def check_causal(i, eng, tag, variant='plain'):
    """The three assertions on a causal engine; returns its gradient."""
    S, sl, eps = n_slabs(i), slabs(i), eps_of(i, variant)
    om = eng.causal_weights(0)
    _, lv = eng.eval_loss(0, lossVec=True)
    own = causal_ref.causal_weights(lv.cpu().numpy().astype(np.float64), sl, S, eps)[1]
    ref_om = reference64(i, 'causal', variant)[0]['omega_slab']
    rec = {'weights_vs_own_lossVec': float(np.max(np.abs(om - own) / own)), 'weights_vs_reference': float(np.max(np.abs(om - ref_om) / ref_om)),
           'weights_bar_b': weights_bar(i, variant), 'min_omega': float(om.min())}
    RECORD[tag + '/weights'] = rec
    print('causal %s weights: %s' % (tag, json.dumps(rec, sort_keys=True)))
    assert om.shape == (S,) and om[0] == 1.0                              # omega = 1 on slab 0
    assert rec['weights_vs_own_lossVec'] <= 1e-6, rec                     # (a)
    assert rec['weights_vs_reference'] <= rec['weights_bar_b'], rec       # (b)
    # (c): the reference with the engine's weights as static weights, at the project bars
    om_k = om[sl]
    return check_parity(i, eng, reference(i, 'static', variant, omega=om_k), tag,
                        lambda: reference(i, 'static', variant, dtype=torch.float32, omega=om_k)[1])


@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_causal_parity(i, kernel):
    weights_are_real(i, 'causal')
    if outside_generic(i, kernel):
        return
    eng = make_engine(i, kernel, 'causal')
    try:
        g1 = check_causal(i, eng, '%s/causal/%s' % (IDS[i], KNAME[kernel]))
        assert np.array_equal(g1, grad_of(eng))                           # two calls: the same bits
    finally:
        eng.close()


def test_causal_parity_with_all_three_terms():
    i = 3
    weights_are_real(i, 'causal', 'terms')
    eng = make_engine(i, mode='causal', variant='terms')
    try:
        check_causal(i, eng, '%s/causal/auto/terms' % IDS[i], 'terms')
    finally:
        eng.close()


@pytest.mark.parametrize('i', OBJ64_CASES, ids=[IDS[k] for k in OBJ64_CASES])
def test_causal_objective64_parity(i):
    """The fp64 objective computes its weights in double from its own loss field: the reference evaluated with the weights of
    the returned (unweighted) lossVec reproduces loss components (1e-12: (a) for this entry point, since var = sum omega_k l_k
    exposes the weights), lossVec and gradient blocks (1e-11); against the reference's own weights: (b) with 1e-11 for LVEC_RTOL."""
    S, sl, eps = n_slabs(i), slabs(i), eps_of(i)
    th = theta(i).astype(np.float64) + 1e-3 * np.random.default_rng(6).standard_normal(theta(i).size)
    ref_c, _ = reference(i, 'causal', flat=th)
    ref0, g0 = reference(i, 'none', flat=th)
    eng = make_engine(i, mode='causal')
    try:
        out, g, lv = eng.objective64(0, theta=th, grad=True, lossVec=True)
        om_k, om_s = causal_ref.causal_weights(lv.cpu().numpy(), sl, S, eps)
        ref, gref = reference(i, 'static', flat=th, omega=om_k)
        assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss'])
        assert np.linalg.norm(gref - g0) > 1e-2 * np.linalg.norm(gref)
        rec = _objective64_record(i, out, g, lv, ref, gref)
        rec['weights_vs_reference'] = float(np.max(np.abs(om_s - ref_c['omega_slab']) / ref_c['omega_slab']))
        RECORD['%s/causal/objective64' % IDS[i]] = rec
        print('causal objective64 %s: %s' % (IDS[i], json.dumps(rec, sort_keys=True)))
        _assert_objective64(rec)
        assert rec['weights_vs_reference'] <= weights_bar(i) * 1e-11 / LVEC_RTOL + 1e-12
        out2, _, _ = eng.objective64(0, theta=th, grad=False)            # engine-owned loss field: same bits
        assert out2 == out
    finally:
        eng.close()


# ---- de-duplicated step ---------------------------------------------------------------------------------------------
def test_causal_dedup_identity_map():
    """Identity point map on the bench network: the three assertions, against the row-wise gradient of the same engine, two
    calls give the same bits, and the row-wise loss-only form agrees."""
    i = 3
    weights_are_real(i, 'causal')
    d_in, dim, widths = CASES[i][0], CASES[i][1], CASES[i][2]
    eng = make_engine(i, mode='causal')
    try:
        g_row = grad_of(eng)
        nT = inputs(i)[0]['Input'].shape[0]
        idx = torch.arange(nT, dtype=torch.int32)
        eng.set_dedup(0, inputs(i)[0]['Input'], idx, torch.arange(nT + 1, dtype=torch.int32), idx)     # keeps the registration
        g1 = check_causal(i, eng, '%s/causal/dedup_identity' % IDS[i])
        assert np.array_equal(g1, grad_of(eng))
        assert not np.array_equal(g1, g_row)                              # another formulation ran
        dev32 = lambda: fp32_deviation(reference(i, 'causal', dtype=torch.float32)[1], reference64(i, 'causal')[1], d_in, widths, dim)
        RECORD['%s/causal/dedup_identity/vs_rowwise' % IDS[i]] = assert_pair_close(
            g1, g_row, d_in, widths, GRAD_RTOL, dim=dim, dev32=dev32, what='dedup vs row-wise')
        out_dd, _ = eng.eval_loss(0)
        eng.debug_point_route(8)
        out_rw, _ = eng.eval_loss(0)
        eng.debug_point_route(0)
        for a, b in zip(out_dd, out_rw):
            assert abs(a - b) <= LOSS_RTOL * abs(b) + 1e-7
        # static weights on the same map
        eng.set_tf_weights(0, static_weights(i))
        check_parity(i, eng, reference64(i, 'static'), '%s/static/dedup_identity' % IDS[i],
                     lambda: reference(i, 'static', dtype=torch.float32)[1])
    finally:
        eng.close()


# ---- bitwise --------------------------------------------------------------------------------------------------------
def _theta_after(eng, state, fn):
    eng.import_state(state)
    fn()
    torch.cuda.synchronize()
    return eng.get_params()


def test_train_epoch_over_two_batches_one_with_causal_weights():
    i = 3
    eng = make_engine(i, mode='causal')                                   # batch 0 carries the registration
    plain = make_engine(i)
    try:
        register_interior(eng, i, batch=1)                                # batch 1: the same rows, unweighted
        g1 = grad_of(eng, 1)
        assert np.array_equal(g1, grad_of(plain))                         # ... bit for bit the step of a plain engine
        assert not np.array_equal(g1, grad_of(eng, 0))
        s0 = eng.export_state()
        acc = torch.zeros(1, device='cuda')
        a = _theta_after(eng, s0, lambda: eng.train_epoch((0, 1, 0), acc))
        losses = [torch.zeros(1, device='cuda') for _ in range(3)]
        b = _theta_after(eng, s0, lambda: [eng.train_step(k, l) for k, l in zip((0, 1, 0), losses)])
        assert np.array_equal(a, b)
        assert eng.step == 3
        total = sum(float(l.item()) for l in losses)
        assert abs(acc.item() - total) <= 1e-5 * abs(total)
    finally:
        eng.close()
        plain.close()


def _snapshot(eng):
    out, lv = eng.eval_loss(0, lossVec=True)
    g = grad_of(eng).copy()
    for _ in range(3):
        eng.train_step(0)
    torch.cuda.synchronize()
    return np.array(out), lv.cpu().numpy(), g, eng.get_params()


@pytest.mark.parametrize('mode', ['static', 'causal'])
@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('i', [2, 3], ids=[IDS[2], IDS[3]])
def test_register_then_clear_is_bitwise_untouched(i, kernel, mode):
    runs = []
    for how in ('never', 'cleared', 'reregistered'):
        eng = make_engine(i, kernel, 'none' if how == 'never' else mode)
        try:
            if how == 'cleared':
                eng.grad(0)                                               # a step with the weights ...
                if mode == 'static':
                    eng.set_tf_weights(0)                                 # ... then cleared
                else:
                    eng.set_causal(0)
            elif how == 'reregistered':
                eng.grad(0)
                register_interior(eng, i)                                 # a new vn_set_interior clears the registration
            runs.append(_snapshot(eng))
        finally:
            eng.close()
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert np.array_equal(x, y)


def test_static_and_causal_registrations_replace_each_other():
    i = 3
    eng = make_engine(i, mode='static')
    ref_s, ref_c = make_engine(i, mode='static'), make_engine(i, mode='causal')
    try:
        g_s, g_c = grad_of(ref_s).copy(), grad_of(ref_c).copy()
        assert not np.array_equal(g_s, g_c)
        assert np.array_equal(grad_of(eng), g_s)
        register_weights(eng, i, 'causal')                                # replaces the static registration
        assert np.array_equal(grad_of(eng), g_c)
        assert np.array_equal(eng.causal_weights(0), ref_c.causal_weights(0))
        register_weights(eng, i, 'static')                                # ... and back
        assert np.array_equal(grad_of(eng), g_s)
        with pytest.raises(VNError, match='error 3: batch 0 has no causal registration'):
            eng.causal_weights(0)
    finally:
        for e in (eng, ref_s, ref_c):
            e.close()


def test_map_terms_and_weights_in_any_order():
    """The de-duplication map, the three terms and the causal registration, registered in several orders: the same bits."""
    i = 3
    nT = inputs(i)[0]['Input'].shape[0]
    idx = torch.arange(nT, dtype=torch.int32)
    ptr = torch.arange(nT + 1, dtype=torch.int32)
    steps = {'map': lambda e: e.set_dedup(0, inputs(i)[0]['Input'], idx, ptr, idx),
             'react': lambda e: register_terms(e, i, which=('react',)),
             'nlflux': lambda e: register_terms(e, i, which=('nlflux',)),
             'nldiff': lambda e: register_terms(e, i, which=('nldiff',)),
             'weights': lambda e: register_weights(e, i, 'causal', 'terms')}
    orders = (('map', 'react', 'nlflux', 'nldiff', 'weights'), ('weights', 'nldiff', 'nlflux', 'react', 'map'),
              ('react', 'weights', 'map', 'nldiff', 'nlflux'))
    grads, oms = [], []
    for order in orders:
        eng = make_engine(i)
        try:
            for name in order:
                steps[name](eng)
            grads.append(grad_of(eng).copy())
            oms.append(eng.causal_weights(0))
        finally:
            eng.close()
    ref = reference64(i, 'causal', 'terms')[0]
    assert abs(grads[0][-4] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7          # map, terms and weights are all there
    for g, om in zip(grads[1:], oms[1:]):
        assert np.array_equal(g, grads[0]) and np.array_equal(om, oms[0])


# ---- slab selection, alignment ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
def test_zero_eps_is_unit_weights(kernel):
    i = 2
    eng = make_engine(i, kernel)
    try:
        register_weights(eng, i, 'causal', eps=0.0)
        np.testing.assert_array_equal(eng.causal_weights(0), np.ones(n_slabs(i)))
        check_parity(i, eng, reference64(i, 'none'), '%s/causal_eps0/%s' % (IDS[i], KNAME[kernel]),
                     lambda: reference(i, 'none', dtype=torch.float32)[1])
    finally:
        eng.close()


def test_omega_view_off_the_16_byte_grid():
    """Case 1 cut to 39 test functions, omega_dev one float off the 16-byte grid: the one-row form of the row-wise apply kernel."""
    i, n_k = 1, 39
    d_in, dim, widths, q, _, nB, bDof, td, act, source, integW, detJvec, rows = CASES[i]
    d = {k: (v[:n_k * q] if k in ('Input', 'gcoef') else v) for k, v in inputs(i)[0].items()}
    om = static_weights(i)[:n_k]
    eng = VNEngine(dim, d_in, widths, td, q, activationFun=act)
    try:
        eng.set_params(theta(i))
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=n_k, detJ=d['detJ'])
        eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
        eng.set_weights(d['w'])
        buf = torch.zeros(n_k + 5, dtype=torch.float32, device='cuda')
        view = buf[1:1 + n_k]
        view.copy_(torch.as_tensor(om))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
        eng.set_tf_weights(0, view)
        kw = dict(Input=d['Input'], gcoef=d['gcoef'], source=None, N=d['N'][:n_k * q], dNt=d['dNt'][:n_k * q], integW=None,
                  intShape=[n_k, q], detJ=float(d['detJ']), detJvec=False, biInput=d['biInput'][:nB], biLabel=d['biLabel'][:nB],
                  bDof=bDof, biDimVal=2.0, w=d['w'], dim=dim, time_dependent=td, is_source=False, integWflag=False, activation=act)
        ev = lambda dt, f, o: causal_ref.loss_and_grad(theta(i).astype(f), d_in, widths, o, None, dtype=dt, **{
            k: (v.astype(f) if isinstance(v, np.ndarray) and v.dtype.kind == 'f' else v) for k, v in kw.items()})
        ref, gref = ev(torch.float64, np.float64, om)
        ref0, g0 = ev(torch.float64, np.float64, None)
        assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss'])
        assert np.linalg.norm(gref - g0) > 1e-2 * np.linalg.norm(gref)
        check_parity(i, eng, (ref, gref), '%s/static/misaligned_39' % IDS[i], lambda: ev(torch.float32, np.float32, om)[1])
    finally:
        eng.close()


# ---- contract and refusals ------------------------------------------------------------------------------------------
def test_refusals():
    i = 2
    sl, S = slabs(i), n_slabs(i)
    eng = make_engine(i, VN_KERNEL_FUSED)                                 # the 4-wave cross-check geometry
    try:
        with pytest.raises(VNError, match='error 5: vn_set_tf_weights is not built for VN_KERNEL_FUSED'):
            eng.set_tf_weights(0, static_weights(i))
        with pytest.raises(VNError, match='error 5: vn_set_causal is not built for VN_KERNEL_FUSED'):
            eng.set_causal(0, sl, S, 1.0)
        eng.set_tf_weights(0)                                             # clearing is always accepted
        eng.set_causal(0)
    finally:
        eng.close()
    eng = make_engine(i)
    try:
        for eps in (float('nan'), float('inf'), -1.0):
            with pytest.raises(VNError, match='error 1: causal eps'):
                eng.set_causal(0, sl, S, eps)
        for n in (0, 4097):
            with pytest.raises(VNError, match='error 1: n_slabs'):
                eng.set_causal(0, sl, n, 1.0)
        bad = sl.copy()
        bad[1] = S
        with pytest.raises(VNError, match=r'error 1: 1 slab id\(s\) outside'):
            eng.set_causal(0, bad, S, 1.0)
        bad[1] = -1
        with pytest.raises(VNError, match=r'error 1: 1 slab id\(s\) outside'):
            eng.set_causal(0, bad, S, 1.0)
        with pytest.raises(VNError, match='error 3'):
            eng.set_causal(5, sl, S, 1.0)                                 # an unregistered batch
        with pytest.raises(VNError, match='error 3'):
            eng.set_tf_weights(5, static_weights(i))
        with pytest.raises(VNError, match='error 3'):
            eng.causal_weights(0)                                         # no causal registration
        d_in, dim = CASES[i][0], CASES[i][1]
        eng.set_interior(1, torch.zeros(0, d_in, device='cuda'), torch.zeros(0, dim, device='cuda'), None, n_k=0, detJ=0.1)
        some = torch.zeros(4, dtype=torch.int32, device='cuda')           # (an empty tensor has no address: through the C ABI)
        with pytest.raises(VNError, match='error 1: batch 1 has no interior rows'):
            eng._ck(eng.lib.vn_set_tf_weights(eng.h, 1, some.data_ptr()))
        with pytest.raises(VNError, match='error 1: batch 1 has no interior rows'):
            eng._ck(eng.lib.vn_set_causal(eng.h, 1, some.data_ptr(), 1, 1.0))
        with pytest.raises(AssertionError, match='one entry per test function'):
            eng.set_tf_weights(0, static_weights(i)[:-1])
        with pytest.raises(AssertionError, match='one entry per test function'):
            eng.set_causal(0, sl[:-1], S, 1.0)
        # none of the refused calls left a registration behind
        plain = make_engine(i)
        try:
            assert np.array_equal(grad_of(eng), grad_of(plain))
        finally:
            plain.close()
    finally:
        eng.close()


def test_lbfgs_takes_static_weights_and_refuses_causal_ones():
    i = 2
    eng = make_engine(i, mode='static', optimizer='lbfgs')
    try:
        ref = reference64(i, 'static')[0]
        info = eng.lbfgs_step(0)
        assert abs(info['f_k'] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7       # the objective has the weights
        assert info['status'] == 0 and info['f_next'] < info['f_k'], info
        register_weights(eng, i, 'causal')
        with pytest.raises(VNError, match='error 5: vn_lbfgs_step on batch 0, which has a causal registration'):
            eng.lbfgs_step(0)
        eng.set_causal(0)                                                 # cleared: the plain objective, evaluated afresh
        out0, _ = eng.eval_loss(0)
        info = eng.lbfgs_step(0)
        assert abs(info['f_k'] - out0[0]) <= LOSS_RTOL * abs(out0[0]) + 1e-7 and info['pairs'] == 0, info
    finally:
        eng.close()


# ---- through VarNet -------------------------------------------------------------------------------------------------
def _pde(vel=0.5, **kw):
    return ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, vel=vel, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x), **kw)


# loss weights of the VarNet test: an untrained network misses its IC by O(1) while its weak-form residuals are O(1e-2), so at unit
# weights the variational term (and with it the weights under test) would be under 1 % of the gradient; 100 puts it beside BC / IC
VN_W = np.array([1.0, 1.0, 100.0])


def _varnet_reference(vn, td, omega=None, causal=None, dtype=torch.float64):
    fd, d = vn.fixData, td.mor[0]
    f = np.float64 if dtype == torch.float64 else np.float32
    Nr, dNxr, dNtr = fd.rows()                                   # (rounded to fp32 below: the engine's tables are fp32)
    cpu = lambda t: t.cpu().numpy().astype(f)
    kw = dict(Input=cpu(d['Input']), gcoef=cpu(d['gcoef']), source=None if d['source'] is None else cpu(d['source']).reshape(-1, 1),
              N=Nr.astype(np.float32).astype(f), dNt=dNtr.astype(np.float32).astype(f), integW=None, intShape=[fd.nt, fd.integNum],
              detJ=float(fd.detJ), detJvec=False, biInput=cpu(d['biInput']), biLabel=cpu(d['biLabel']).reshape(-1, 1), bDof=fd.bDofsum,
              biDimVal=float(fd.biDimVal), w=VN_W, dim=vn.dim, time_dependent=True, is_source=vn.lossOpt['isSource'],
              integWflag=False)
    return causal_ref.loss_and_grad(vn.engine.get_params().astype(f), vn.inpDim, vn.layerWidth, omega, causal, dtype=dtype, **kw)


def test_through_varnet_rowwise_shuffled_and_dedup():
    """`VarNet(pde, causal=eps)` on a 12 x 10 1D+t grid: slab ids k % 10, splitLoss in fp32 and fp64 reports the weighted var,
    precisionReport within its bars, causalWeights against the reference, a shuffle moves the ids with the test functions, and
    enable_dedup (a real shared-point map) keeps the registration: the three assertions there too, and against row-wise."""
    vn = VarNet(_pde(), causal=1.0, tDiscNum=10, discNum=12, bDiscNum=None, layerWidth=[20, 20])
    eng = vn.engine
    try:
        eng.set_params(eng.get_params() + 0.05 * np.random.default_rng(5).standard_normal(eng.P).astype(np.float32))
        nt = vn.fixData.nt
        td = vn._build_tdata()
        np.testing.assert_array_equal(td.mor[0]['slab'].cpu().numpy(), np.arange(nt) % 10)
        td.select_mor(0)
        eng.set_weights(VN_W)
        sl = np.arange(nt) % 10
        # eps from the untrained network's own loss field: min omega = 1/4 in the reference
        lv0 = _varnet_reference(vn, td)[0]['lossVec'].reshape(-1)
        C = float(np.sum([lv0[sl == s].mean() for s in range(9)]))
        vn.tData = td
        vn.setCausal(LN4 / C)
        causal = (sl, 10, LN4 / C)
        ref, gref = _varnet_reference(vn, td, causal=causal)
        ref0, g0 = _varnet_reference(vn, td)
        assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss'])
        assert np.linalg.norm(gref - g0) > 1e-2 * np.linalg.norm(gref)
        bar_b = LN4 * LVEC_RTOL * 9 * float(np.max(lv0)) / C + 1e-6
        P = eng.P

        def three(tag):
            om = vn.causalWeights(td)
            out, lv = eng.eval_loss(0, lossVec=True)
            lv = lv.cpu().numpy().astype(np.float64)
            own = causal_ref.causal_weights(lv, sl, 10, LN4 / C)[1]
            rec = {'weights_vs_own_lossVec': float(np.max(np.abs(om - own) / own)),
                   'weights_vs_reference': float(np.max(np.abs(om - ref['omega_slab']) / ref['omega_slab'])), 'weights_bar_b': bar_b}
            assert om[0] == 1.0 and rec['weights_vs_own_lossVec'] <= 1e-6 and rec['weights_vs_reference'] <= bar_b, rec
            # lossVec is unweighted: the same bits under other weights (the seed kernel that writes it never sees them)
            vn.setCausal(2.0 * LN4 / C)
            assert not np.array_equal(vn.causalWeights(td), om)
            assert np.array_equal(eng.eval_loss(0, lossVec=True)[1].cpu().numpy().astype(np.float64), lv)
            vn.setCausal(LN4 / C)
            td.select_mor(0)
            rs, gs = _varnet_reference(vn, td, omega=om[sl])
            g = grad_of(eng)
            for k in range(4):
                assert abs(g[P + k] - rs[KEYS[k]]) <= LOSS_RTOL * abs(rs[KEYS[k]]) + 1e-7, (tag, KEYS[k], g[P + k], rs[KEYS[k]])
                assert abs(out[k] - rs[KEYS[k]]) <= LOSS_RTOL * abs(rs[KEYS[k]]) + 1e-7, (tag, KEYS[k], out[k], rs[KEYS[k]])
            assert_grad_close(g[:P], gs, vn.inpDim, vn.layerWidth, GRAD_RTOL, dim=1, what=tag,
                              g32=lambda: _varnet_reference(vn, td, omega=om[sl], dtype=torch.float32)[1], rec=rec)
            RECORD[tag] = rec
            return g

        g_row = three('varnet_1dt/rowwise')
        comp, _, _ = vn.splitLoss(td)
        assert abs(comp[2, 0] - ref['varLoss']) <= LOSS_RTOL * abs(ref['varLoss']) + 1e-7
        comp64, _, _ = vn.splitLoss(td, fp64=True)
        assert abs(comp64[2, 0] - ref['varLoss']) <= 1e-9 * abs(ref['varLoss'])
        rep = vn.precisionReport(td)
        assert not rep['dedup'] and rep['loss']['varLoss'] <= LOSS_RTOL and rep['grad_global'] <= GRAD_RTOL, rep
        # a shuffle permutes the test functions: the ids move with them, so the full-batch var is unchanged (the BC / IC rows
        # are permuted across their split by the same call, as in the reference: those two components move)
        loss_before = eng.eval_loss(0)[0][3:]
        np.random.seed(3)
        td.shuffleTrainData()
        td.select_mor(0)
        assert not np.array_equal(td.batchInd, np.arange(nt))
        loss_after = eng.eval_loss(0)[0][3:]
        for a, b in zip(loss_after, loss_before):
            assert abs(a - b) <= LOSS_RTOL * abs(b) + 1e-7, (loss_after, loss_before)
        # the de-duplicated step on a fresh (unshuffled) set
        td = vn.tData = vn._build_tdata()
        td.select_mor(0)
        U = td.enable_dedup()
        assert td.dedup_reason is None and 0 < U < vn.fixData.nT / 2, (td.dedup_reason, U)
        g1 = three('varnet_1dt/dedup')
        assert np.array_equal(g1, grad_of(eng)) and not np.array_equal(g1, g_row)
        dev32 = lambda: fp32_deviation(_varnet_reference(vn, td, causal=causal, dtype=torch.float32)[1], gref, vn.inpDim, vn.layerWidth, 1)
        RECORD['varnet_1dt/dedup_vs_rowwise'] = assert_pair_close(g1, g_row, vn.inpDim, vn.layerWidth, GRAD_RTOL, dim=1, dev32=dev32,
                                                                    what='varnet dedup vs row-wise')
        rep = vn.precisionReport(td)
        assert rep['dedup'] and rep['loss']['varLoss'] <= LOSS_RTOL and rep['grad_global'] <= GRAD_RTOL, rep
    finally:
        eng.close()


# ---- training: one pair of runs -----------------------------------------------------------------------------------------
E2E = dict(layerWidth=[20], discNum=20, bDiscNum=None, activationFun='tanh', learning_rate=0.01)     # tests/test_nlflux_gpu.py
EPOCHS = 10000
KAPPA, T_END, VEL = 0.1, 0.5, 0.5


def test_causal_run_against_the_plain_run(tmp_path):
    """The advection-diffusion travelling wave of tests/test_nlflux_gpu.py::test_linear_flux_against_the_velocity_run in its
    plain vel = 0.5 form, u = exp(-kappa pi^2 t) sin(pi (x - vel t)) with its Dirichlet data, trained plainly (the twin, which
    that test requires to reach 0.05) and with causal = ln 4 / C_{S-1} of the untrained network's loss field (smallest initial
    weight 1/4).  Bars: err <= 2 err_twin + 0.01, cap 0.2, twin <= 0.05; the final min omega is finite and above the initial
    one: the early slabs converged and released the late ones.  No claim that the causal run beats the twin on this easy problem."""
    cEx = lambda x, t=0: np.exp(-KAPPA * pi ** 2 * t) * np.sin(pi * (x - VEL * t))
    mk = lambda: ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=KAPPA, vel=VEL, tInterval=[0, T_END], IC=lambda x: cEx(x, 0.0),
                       cEx=cEx, BCs=[[0.0, 1.0, cEx], [0.0, 1.0, cEx]])
    np.random.seed(0)
    twin_vn = VarNet(mk(), tDiscNum=10, **E2E)
    twin_vn.train(str(tmp_path / 'twin'), epochNum=EPOCHS, tol=0.0, saveFreq=EPOCHS, verbose=False)
    twin = float(twin_vn.residual()[2])
    twin_vn.engine.close()

    np.random.seed(0)
    vn = VarNet(mk(), tDiscNum=10, causal=0.0, **E2E)
    td = vn._build_tdata()
    td.select_mor(0)
    _, lv = vn.engine.eval_loss(0, lossVec=True)
    lv = lv.cpu().numpy().astype(np.float64)
    sl = td.mor[0]['slab'].cpu().numpy()
    C = float(np.sum([lv[sl == s].mean() for s in range(9)]))
    vn.tData = td
    vn.setCausal(LN4 / C)                                                 # re-registers td; train() registers its own set with it
    om0 = vn.causalWeights(td)
    np.random.seed(0)
    vn.train(str(tmp_path / 'causal'), epochNum=EPOCHS, tol=0.0, saveFreq=EPOCHS, verbose=False)
    err = float(vn.residual()[2])
    om1 = vn.causalWeights()
    vn.engine.close()
    rec = {'causal': err, 'twin': twin, 'bar': min(2.0 * twin + 0.01, 0.2), 'eps': LN4 / C, 'min_omega_initial': float(om0.min()),
           'min_omega_final': float(om1.min())}
    RECORD['twin/travelling_wave'] = rec
    print('causal travelling wave: %s' % json.dumps(rec, sort_keys=True))
    assert abs(om0.min() - 0.25) <= 1e-3
    assert twin <= 0.05, twin
    assert err <= 2.0 * twin + 0.01 and err <= 0.2, (err, twin)
    assert np.isfinite(om1.min()) and om1.min() > om0.min(), (om0, om1)
