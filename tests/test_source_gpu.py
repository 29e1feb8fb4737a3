"""
GPU tier of source identification (vn_set_source_basis, vn_set_source_learn, vn_get_source_amps, vn_set_source_amps;
`VarNet(learnSource=...)`): the amplitude gradient of vn_learnt.hip against the fp64 restatement tests/source_ref.py on the cases of
tests/source_cases.py -- row-wise on the automatic route (the two-pass sequence; for integ_num > 128 the two-pass route itself), on
the generic kernels and on one layer-by-layer engine, de-duplicated on the case's shared-point map (for the EMPTY cases also the
map with row-less points) -- loss pieces, lossVec and the theta-gradient at the mixed source, that a = 0 and learning off give back
the bits of an engine without a basis, the Adam step of the amplitudes, snapshot / rollback, vn_eval_loss and the fp64 objective at
the device amplitudes, every refusal, and one recovery end to end.

Bar per component (tests/source_cases.py): |g - g64| <= GRAD_RTOL * max(|g64|, 0.01 S_j).  The worst errors are written to
source_parity.json in the directory VN_RECORD_DIR names (default: profile_out/ beside tests/; committed copy:
profiles/source_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import source_cases as sc
from tests.dedup_term_cases import BIDIMVAL, DETJ, empty_map
from tests.test_dedup_terms_gpu import check_parity
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import VN_COMM_ID_BYTES, VN_KERNEL_AUTO, VN_KERNEL_GENERIC, VN_KERNEL_LAYERED, VNEngine, VNError
from varnet_amd.varnet import VarNet

pytestmark = pytest.mark.gpu

pi = np.pi
RECORD = {}
KERNEL = {'generic': VN_KERNEL_GENERIC, 'layered': VN_KERNEL_LAYERED}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'source_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


# ---- engine-level helpers -------------------------------------------------------------------------------------------
def make_engine(i, route='auto', J=3, empty=False, optimizer='adam', lr=0.001, source=None, basis=True):
    """An engine of case i with has_source, the case's s0 (zeros when it has none; `source`: another stream), the three polynomial
    terms and, with `basis`, the J basis streams; route 'dedup' adds the case's shared-point map."""
    d_in, dim, widths, q, n_k, U, nB, bDof, _, integW, td, act = sc.case(i)[:12]
    d = sc.inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=True, integWflag=integW, activationFun=act, optimizer_name=optimizer,
                   learning_rate=lr, kernel=KERNEL.get(route, VN_KERNEL_AUTO))
    eng.set_params(sc.theta(i))
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, BIDIMVAL)
    eng.set_weights(d['w'])
    eng.set_interior(0, d['Input'], d['gcoef'], sc.s0_of(i) if source is None else source, n_k=n_k, detJ=DETJ)
    nldiff, nlflux, reaction = sc.terms_of(i)
    eng.set_reaction(0, *reaction)
    eng.set_nlflux(0, *nlflux)
    eng.set_nldiff(0, *nldiff)
    if basis:
        eng.set_source_basis(0, sc.basis(i, J)[0])
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


def check_amp_grad(tag, ga, i, J, mask=None):
    """ga against the fp64 reference within the bar, printed and recorded before the assertion."""
    _, _, g64, S = sc.reference64(i, J)
    on = np.ones(J, dtype=bool) if mask is None else np.array(mask, dtype=bool)
    bar = sc.bars(g64, S)
    err = np.abs(ga - g64)
    rel = np.where(on, err / bar, 0.0)
    RECORD[tag] = {'worst_err_over_bar': float(rel.max()), 'worst_component': int(rel.argmax()),
                   'worst_rel_of_g': float(np.max(np.where(on, err / np.abs(g64), 0.0))),
                   'worst_rel_of_S': float(np.max(np.where(on, err / S, 0.0)))}
    print('source %s: %s' % (tag, json.dumps(RECORD[tag], sort_keys=True)))
    assert np.all(np.isfinite(ga))
    assert np.all(ga[~on] == 0.0), (tag, ga)
    assert np.all(err[on] <= bar[on]), (tag, ga, g64, bar)


def gradient_checks(i, J, route, empty=False, mask=None):
    tag = '%s/J%d/%s%s' % (sc.IDS[i], J, route, '/empty_points' if empty else '')
    Phi, amp = sc.basis(i, J)
    m = [1] * J if mask is None else mask
    net = (sc.case(i)[0], sc.case(i)[1], sc.case(i)[2], sc.case(i)[10])
    eng = make_engine(i, route, J, empty)
    try:
        # learning off: a registered basis changes nothing (the bits of an engine that has none)
        g_off, (l_off, lv_off) = grad_of(eng), loss_field(eng)
        if J == 3 and route in ('generic', 'dedup'):
            bare = make_engine(i, route, J, empty, basis=False)
            try:
                assert np.array_equal(grad_of(bare), g_off), tag
                lb, lvb = loss_field(bare)
                assert np.array_equal(lb, l_off) and np.array_equal(lvb, lv_off), tag
            finally:
                bare.close()
            # a = 0: loss pieces, lossVec and theta-gradient are bitwise those of the engine without a basis
            eng.set_source_learn(m, np.zeros(J), lr=0.01)
            assert np.array_equal(grad_of(eng), g_off), tag
            l0, lv0 = loss_field(eng)
            assert np.array_equal(l0, l_off) and np.array_equal(lv0, lv_off), tag
        eng.set_source_learn(m, amp, lr=0.01)
        ref = sc.reference64(i, J)
        g32 = lambda: sc.evaluate(i, J, dtype=torch.float32)[1]
        g_on = check_parity(i, eng, tag, ref[:2], g32, net=net, record=RECORD)
        assert not np.array_equal(g_on, g_off), tag                           # the amplitudes count
        a, ga = eng.get_source_amps(grad=True)
        assert np.array_equal(a, amp)
        check_amp_grad(tag + '/amp', ga, i, J, mask)
        grad_of(eng)
        assert np.array_equal(eng.get_source_amps(grad=True)[1], ga), tag     # two evaluations: the same J doubles
        eng.set_source_learn(None)
        assert np.array_equal(grad_of(eng), g_off), tag                       # learning off again: the parent's bits
        with pytest.raises(VNError, match='error 3: no learnt source amplitudes'):
            eng.get_source_amps(J=J)
    finally:
        eng.close()


# ---- 1. the amplitude gradient ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['auto', 'generic', 'dedup'])
@pytest.mark.parametrize('i', range(sc.N_CASES), ids=sc.IDS)
def test_amplitude_gradient(i, route):
    gradient_checks(i, 3, route)


@pytest.mark.parametrize('i', sc.EMPTY, ids=[sc.IDS[k] for k in sc.EMPTY])
def test_amplitude_gradient_with_rowless_points(i):
    gradient_checks(i, 3, 'dedup', empty=True)


@pytest.mark.parametrize('route', ['auto', 'dedup'])
@pytest.mark.parametrize('J', [1, 64])
@pytest.mark.parametrize('i', sc.WIDE, ids=[sc.IDS[k] for k in sc.WIDE])
def test_one_and_sixty_four_streams(i, J, route):
    gradient_checks(i, J, route)


@pytest.mark.parametrize('route', ['auto', 'generic', 'dedup'])
@pytest.mark.parametrize('i', sc.WIDE, ids=[sc.IDS[k] for k in sc.WIDE])
def test_masked_amplitudes(i, route):
    """Mask [1, 0, 1, 0, 0]: the unmasked gradients read 0 (gradient_checks), the unmasked amplitudes take part in the source at
    their initial values and keep their bits through a step."""
    gradient_checks(i, 5, route, mask=sc.MASK5)
    amp = sc.basis(i, 5)[1]
    eng = make_engine(i, route, 5)
    try:
        eng.set_source_learn(sc.MASK5, amp, lr=0.05)
        eng.train_epoch([0, 0])
        torch.cuda.synchronize()
        got = eng.get_source_amps()
        on = np.array(sc.MASK5, dtype=bool)
        assert np.array_equal(got[~on], amp[~on]) and np.all(got[on] != amp[on]), (got, amp)
    finally:
        eng.close()


def test_layer_by_layer_route():
    i = 7
    eng = make_engine(i, 'layered')
    try:
        assert eng.kernel_path()[0] == VN_KERNEL_LAYERED
    finally:
        eng.close()
    gradient_checks(i, 3, 'layered')


def test_routes_taken():
    """The automatic route of the cases with integ_num > 128 is the two-pass route; GENERIC is the generic kernels."""
    for i in (2, 4):
        eng = make_engine(i)
        try:
            assert eng.kernel_path()[1] == 1, sc.IDS[i]
        finally:
            eng.close()
    eng = make_engine(0, route='generic')
    try:
        assert eng.kernel_path()[0] == VN_KERNEL_GENERIC
    finally:
        eng.close()


def test_single_launch_route_takes_the_two_pass_sequence():
    """A batch without any polynomial term runs the single-launch 8-wave kernel; with a basis and learning on it takes the two-pass
    sequence (udbar exists there only) and the amplitude gradient is the reference's of that problem."""
    i, J = 0, 3
    d_in, dim, widths, q, n_k, U, nB, bDof, _, integW, td, act = sc.case(i)[:12]
    d = sc.inputs(i)
    Phi, amp = sc.basis(i, J)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=True, integWflag=integW, activationFun=act)
    try:
        eng.set_params(sc.theta(i))
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        eng.set_bic(d['biInput'], d['biLabel'], bDof, BIDIMVAL)
        eng.set_weights(d['w'])
        eng.set_interior(0, d['Input'], d['gcoef'], sc.s0_of(i), n_k=n_k, detJ=DETJ)
        eng.set_source_basis(0, Phi)
        assert eng.kernel_path()[1] == 0
        eng.set_source_learn([1] * J, amp, lr=0.01)
        grad_of(eng)
        ga = eng.get_source_amps(grad=True)[1]
        from tests import source_ref
        from tests.inverse_ref import OFF
        _, _, g64, S = source_ref.evaluate(sc.theta(i), d_in, widths, sc.s0_of(i), Phi.T, amp, np.array(OFF), **sc.ref_kw(i))
        err, bar = np.abs(ga - g64), sc.bars(g64, S)
        print('no terms, fused8 -> two-pass: err/bar', err / bar)
        assert np.all(g64 != 0.0) and np.all(err <= bar), (ga, g64, bar)
    finally:
        eng.close()


def test_next_to_coefficient_learning():
    """Both modes on: each gradient keeps the value it has with the other mode off -- the nine coefficient gradients bitwise, the
    amplitude gradient at its bar (and here bitwise too); one step moves both vectors on the one step counter."""
    i, J = 0, 3
    amp, c0 = sc.basis(i, J)[1], sc.coefs_of(i)
    for route in ('auto', 'dedup'):
        eng = make_engine(i, route, J)
        try:
            eng.set_source_learn([1] * J, amp, lr=0.01)
            grad_of(eng)
            ga_alone = eng.get_source_amps(grad=True)[1]
        finally:
            eng.close()
        # the coefficients alone, on an engine whose plain source is the mixed stream the other one forms
        mix = fma_mix(i, J, amp)
        eng = make_engine(i, route, J, source=mix, basis=False)
        try:
            eng.set_coef_learn([1] * 9, c0, lr=0.01)
            grad_of(eng)
            gc_alone = eng.get_coefs(grad=True)[1]
        finally:
            eng.close()
        eng = make_engine(i, route, J)
        try:
            eng.set_coef_learn([1] * 9, c0, lr=0.01)
            eng.set_source_learn([1] * J, amp, lr=0.01)
            grad_of(eng)
            gc, ga = eng.get_coefs(grad=True)[1], eng.get_source_amps(grad=True)[1]
            assert np.array_equal(gc, gc_alone), (route, gc, gc_alone)
            check_amp_grad('%s/J%d/%s/with_coef_learn' % (sc.IDS[i], J, route), ga, i, J)
            assert np.array_equal(ga, ga_alone)
            eng.train_step(0)
            torch.cuda.synchronize()
            assert eng.step == 1
            assert np.all(eng.get_coefs() != c0.astype(np.float32).astype(np.float64)) and np.all(eng.get_source_amps() != amp)
        finally:
            eng.close()


def test_next_to_flux_rows_periodic_pairs_and_observations():
    """The boundary passes do not contain the source: with all three registered the amplitude gradient is what it was."""
    i, J = 0, 3
    d_in, dim = sc.case(i)[0], sc.case(i)[1]
    rng = np.random.default_rng(31)
    for route in ('auto', 'dedup'):
        eng = make_engine(i, route, J)
        try:
            eng.set_source_learn([1] * J, sc.basis(i, J)[1], lr=0.01)
            grad_of(eng)
            before = eng.get_source_amps(grad=True)[1]
            nrm = rng.standard_normal((17, dim)).astype(np.float32)
            eng.set_flux_bc(rng.uniform(-1, 1, (17, d_in)).astype(np.float32), nrm, rng.uniform(0, 1, 17).astype(np.float32),
                            rng.standard_normal(17).astype(np.float32), BIDIMVAL)
            eng.set_periodic(rng.uniform(-1, 1, (22, d_in)).astype(np.float32), rng.standard_normal((22, dim)).astype(np.float32), 1.0,
                             BIDIMVAL)
            eng.set_observations(rng.uniform(-1, 1, (33, d_in)).astype(np.float32), rng.standard_normal(33).astype(np.float32), weight=2.0)
            grad_of(eng)
            ga = eng.get_source_amps(grad=True)[1]
            check_amp_grad('%s/J%d/%s/edge_passes' % (sc.IDS[i], J, route), ga, i, J)
            assert np.array_equal(ga, before)
        finally:
            eng.close()


# ---- 2. the step ----------------------------------------------------------------------------------------------------------
STEP_LR = 0.1     # 1e-6 of lr = 1e-7: above the half-ulp of an fp32 amplitude of magnitude <= 2 (1.2e-7 / 2) plus the fp32 step arithmetic


@pytest.mark.parametrize('route', ['auto', 'dedup'])
@pytest.mark.parametrize('i', sc.WIDE, ids=[sc.IDS[k] for k in sc.WIDE])
def test_train_step_is_adam_on_the_masked_amplitudes(i, route):
    """One vn_train_step from zero slots moves each masked amplitude as Adam in fp64 says (the engine's beta1, beta2, eps and lr_t
    as the kernel receives them, in fp32; step 1), within 1e-6 of lr; unmasked ones keep their bits; a bound that is hit is held
    exactly; grad + apply takes the same step."""
    J = 5
    mask = [1, 1, 0, 1, 1]
    amp = sc.basis(i, J)[1]
    lo, hi = np.full(J, -np.inf), np.full(J, np.inf)
    lo[3], hi[3] = amp[3] - 0.004, amp[3] + 0.004                       # the first Adam step is lr in size: a_3 hits one of them
    eng = make_engine(i, route, J)
    try:
        eng.set_source_learn(mask, amp, lo, hi, lr=STEP_LR)
        grad_of(eng)
        ga = eng.get_source_amps(grad=True)[1]
        eng.train_step(0)
        torch.cuda.synchronize()
        got, ga2 = eng.get_source_amps(grad=True)
        assert np.array_equal(ga, ga2) and eng.step == 1
        b1, b2, eps = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8))
        gi = ga.astype(np.float32).astype(np.float64)
        lr_t = float(np.float32(STEP_LR * np.sqrt(1 - 0.999) / (1 - 0.9)))
        want = amp - lr_t * ((1 - b1) * gi) / (np.sqrt((1 - b2) * gi * gi) + eps)
        for j in range(J):
            print('step %s/%s a%d: %.9g -> %.9g (Adam %.9g)' % (sc.IDS[i], route, j, amp[j], got[j], want[j]))
            if not mask[j]:
                assert got[j] == amp[j]
            elif j == 3:
                bound = lo[3] if gi[3] > 0 else hi[3]
                assert got[j] == float(np.float32(bound))
            else:
                assert gi[j] != 0.0 and abs(got[j] - want[j]) <= 1e-6 * STEP_LR, (j, got[j], want[j])
        eng.set_source_learn(mask, amp, lo, hi, lr=STEP_LR)
        eng.set_params(sc.theta(i))
        eng.grad(0)
        eng.apply()
        torch.cuda.synchronize()
        # (the step counter went on: lr_t of step 2 with fresh slots differs, so compare against the formula, not the bits)
        t = 2.0
        lr2 = float(np.float32(STEP_LR * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)))
        got2 = eng.get_source_amps()
        want2 = amp - lr2 * ((1 - b1) * gi) / (np.sqrt((1 - b2) * gi * gi) + eps)
        for j in (0, 1, 4):
            assert abs(got2[j] - want2[j]) <= 1e-6 * STEP_LR, (j, got2[j], want2[j])
    finally:
        eng.close()


def _state(eng):
    torch.cuda.synchronize()
    return np.asarray(eng.export_state()).copy(), eng.get_source_amps()


@pytest.mark.parametrize('route', ['auto', 'dedup'])
def test_train_epoch_snapshot_and_rollback(route):
    """vn_train_epoch over [0, 0, 0, 0] is bitwise four single steps, parameters, slots and amplitudes; snapshot -> three steps ->
    rollback restores amplitudes, their slots and the step counter bitwise (the replayed steps end in the same bits);
    vn_set_source_amps invalidates the snapshot."""
    i, J = 6, 3
    amp = sc.basis(i, J)[1]
    a, b = make_engine(i, route, J, lr=0.01), make_engine(i, route, J, lr=0.01)
    try:
        for e in (a, b):
            e.set_source_learn([1] * J, amp, lr=0.02)
        a.train_epoch([0, 0, 0, 0])
        for _ in range(4):
            b.train_step(0)
        sa, ca = _state(a)
        sb, cb = _state(b)
        assert np.array_equal(sa, sb) and np.array_equal(ca, cb)
        assert np.all(ca != amp)
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
        a.set_source_amps(amp)
        with pytest.raises(VNError, match='error 3: no snapshot to roll back to'):
            a.state_rollback()
    finally:
        a.close()
        b.close()


# ---- 3. evaluations at the device amplitudes ----------------------------------------------------------------------------
def fma_mix(i, J, amp):
    """The stream vn_learnt_mix_kernel forms, restated: fp32, from s0, j ascending, one fused multiply-add per stream (the product
    of two fp32 numbers is exact in fp64, so each step is one fp64 addition rounded to fp32)."""
    Phi = sc.basis(i, J)[0]
    s = sc.s0_of(i).astype(np.float32)
    for j in range(J):
        s = (np.float64(np.float32(amp[j])) * Phi[j].astype(np.float64) + s.astype(np.float64)).astype(np.float32)
    return s


@pytest.mark.parametrize('route', ['auto', 'dedup'])
def test_evaluations_at_the_device_amplitudes(route):
    """After vn_set_source_amps(a') vn_eval_loss, vn_grad and vn_objective_f64 equal those of an engine given the pre-mixed stream
    as its plain source: the fp32 results bitwise (the same kernels read the same bits), the fp64 objective at the bars of
    tests/test_obj64_gpu.py (loss pieces 1e-12, gradient 1e-11 of its maximum)."""
    i, J = 1, 3
    amp = sc.basis(i, J)[1]
    a1 = (amp * np.array([1.5, -0.5, 2.0])).astype(np.float32).astype(np.float64)
    a, b = make_engine(i, route, J), make_engine(i, route, J, source=fma_mix(i, J, a1), basis=False)
    try:
        a.set_source_learn([1] * J, amp, lr=0.01)
        out0 = a.objective64(0)[0]
        a.set_source_amps(a1)
        assert np.array_equal(a.get_source_amps(), a1)
        la, lva = loss_field(a)
        lb, lvb = loss_field(b)
        assert np.array_equal(la, lb) and np.array_equal(lva, lvb)
        assert np.array_equal(grad_of(a), grad_of(b))
        out_a, g_a = a.objective64(0)[:2]
        out_b, g_b = b.objective64(0)[:2]
        g_a, g_b = g_a.cpu().numpy(), g_b.cpu().numpy()
        assert not np.allclose(out0[0], out_a[0], rtol=1e-6)               # the amplitudes count
        for k in range(4):
            assert abs(out_a[k] - out_b[k]) <= 1e-12 * abs(out_b[k]), (k, out_a[k], out_b[k])
        assert np.max(np.abs(g_a - g_b)) <= 1e-11 * np.max(np.abs(g_b))
    finally:
        a.close()
        b.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals():
    i, J = 6, 3
    Phi, amp = sc.basis(i, J)
    n_k = sc.case(i)[4]
    ones = [1] * J
    for opt, word in (('rmsprop', 'an RMSProp'), ('lbfgs', 'an L-BFGS')):
        eng = make_engine(i, optimizer=opt)
        try:
            with pytest.raises(VNError, match='error 5: vn_set_source_learn on %s engine' % word):
                eng.set_source_learn(ones, amp, lr=0.01)
        finally:
            eng.close()
    eng = make_engine(i)
    try:
        bad = amp.copy()
        bad[1] = np.nan
        with pytest.raises(VNError, match='error 1: initial amplitude 1'):
            eng.set_source_learn(ones, bad, lr=0.01)
        lo, hi = np.full(J, -np.inf), np.full(J, np.inf)
        lo[2], hi[2] = 1.0, 0.5
        with pytest.raises(VNError, match='error 1: bounds of amplitude 2'):
            eng.set_source_learn(ones, amp, lo, hi, lr=0.01)
        for lr in (0.0, -1.0, float('nan')):
            with pytest.raises(VNError, match='error 1: amplitude learning rate'):
                eng.set_source_learn(ones, amp, lr=lr)
        with pytest.raises(VNError, match='error 1: 1 to 64 source amplitudes can be learnt, got 65'):
            eng.set_source_learn([1] * 65, np.zeros(65), lr=0.01)
        with pytest.raises(VNError, match='error 3: no learnt source amplitudes'):
            eng.set_source_amps(amp)
        with pytest.raises(VNError, match='error 1: a source basis has 1 to 64 streams, got 65'):
            eng.set_source_basis(0, np.zeros((65, Phi.shape[1]), dtype=np.float32))
        # (a failed call leaves the batch without a basis: learning on, the step runs with nothing to reduce)
        eng.set_source_learn(ones, amp, lr=0.01)
        grad_of(eng)
        assert np.all(eng.get_source_amps(grad=True)[1] == 0.0)
        # a basis of another J than the learnt vector's
        eng.set_source_basis(0, sc.basis(i, 5)[0])
        with pytest.raises(VNError, match='error 1: batch 0 has a source basis of 5 streams, the learnt amplitudes .* are 3'):
            eng.grad(0)
        with pytest.raises(VNError, match='error 1: batch 0 has a source basis of 5 streams'):
            eng.eval_loss(0)
        eng.set_source_basis(0, Phi)
        with pytest.raises(VNError, match='error 1: the engine holds 3 source amplitudes'):
            eng.get_source_amps(J=5)
        with pytest.raises(VNError, match='error 1: the engine holds 3 source amplitudes'):
            eng.set_source_amps(np.zeros(5))
        with pytest.raises(VNError, match='error 1: amplitude 0'):
            eng.set_source_amps([np.inf, 0.0, 0.0])
        # per-test-function weights and learning, in either order
        with pytest.raises(VNError, match='error 5: learnt source amplitudes .* next to per-test-function loss weights'):
            eng.set_tf_weights(0, np.ones(n_k, dtype=np.float32))
        eng.set_source_learn(None)
        eng.set_tf_weights(0, np.ones(n_k, dtype=np.float32))
        with pytest.raises(VNError, match=r'error 5: learnt source amplitudes \(vn_set_source_learn\) next to per-test-function loss weights'):
            eng.set_source_learn(ones, amp, lr=0.01)
        eng.set_tf_weights(0, None)
        eng.set_source_learn(ones, amp, lr=0.01)
        with pytest.raises(VNError, match='error 5: vn_comm_init while source amplitudes are learnt'):
            eng.comm_init(0, 1, bytes(VN_COMM_ID_BYTES))
        # vn_set_interior clears the basis of its batch
        d = sc.inputs(i)
        eng.set_interior(0, d['Input'], d['gcoef'], sc.s0_of(i), n_k=n_k, detJ=DETJ)
        grad_of(eng)
        assert np.all(eng.get_source_amps(grad=True)[1] == 0.0)
    finally:
        eng.close()
    # an engine without has_source carries no basis
    d_in, dim, widths, q, n_k, U, nB, bDof, _, integW, td, act = sc.case(i)[:12]
    d = sc.inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=False, integWflag=integW, activationFun=act)
    try:
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=n_k, detJ=DETJ)
        with pytest.raises(VNError, match='error 3: vn_set_source_basis needs an engine created with has_source = 1'):
            eng.set_source_basis(0, Phi)
    finally:
        eng.close()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
KAPPA, T_END = 0.1, 0.5
EPOCHS = 80000      # 3 000, the count of tests/test_inverse_gpu.py, leaves a_3 at 0.002: see test_recovers_the_source_amplitudes
A_STAR = np.array([2.0, -1.0, 4.0])
MODES = (1, 2, 3)


def u_star(x, t):
    """The solution of c_t = kappa c_xx + sum_j a*_j sin(j pi x) with zero initial and boundary values."""
    return sum(a * np.sin(j * pi * x) * (1.0 - np.exp(-KAPPA * j * j * pi * pi * t)) / (KAPPA * j * j * pi * pi)
               for a, j in zip(A_STAR, MODES))


def sensors(seed=0):
    rng = np.random.default_rng(seed)
    x, t = rng.uniform(0, 1, 64), rng.uniform(0, T_END, 64)
    return np.column_stack([x, t]), u_star(x, t)


def problem():
    return ADPDE(Domain1D(np.array([0.0, 1.0])), diff=KAPPA, vel=0.0, tInterval=[0, T_END], IC=lambda x: 0.0 * x, cEx=u_star,
                 sourceBasis=[lambda x, t, j=j: np.sin(j * pi * x) for j in MODES], sourceAmp=[0.0, 0.0, 0.0])


def _train(folder, **vn_kw):
    np.random.seed(0)
    vn = VarNet(problem(), layerWidth=[20], activationFun='tanh', discNum=40, bDiscNum=None, tDiscNum=20, learning_rate=0.01,
                observations=sensors(), **vn_kw)
    vn.train(str(folder), weight=[10.0, 10.0, 1.0], epochNum=EPOCHS, tol=0.0, saveFreq=EPOCHS, verbose=False)
    out = vn.sourceAmplitudes(), vn.obsMisfit(), vn.residual()[2]
    text = open(os.path.join(str(folder), 'caseData.txt')).read()
    vn.engine.close()
    return out + (text,)


def test_recovers_the_source_amplitudes(tmp_path):
    """c_t = kappa c_xx + sum_j a_j sin(j pi x) on [0, 1] x [0, 0.5], truth a* = (2, -1, 4), guess a = 0, 64 point sensors.
    Required: ||a - a*|| falls to a third of the guess's (1.5275), and the misfit ends below that of the twin trained with the
    amplitudes frozen at the guess.  The amplitudes follow the network, and a [20] tanh network takes up sin(3 pi x) from 64 sensors
    slowly: measured on one MI355X (seed fixed, sourceLr at its default 0.01), ||a - a*|| is 4.022 after 3 000 epochs (a_3 = 0.002),
    3.705 after 10 000, 2.498 after 20 000, 1.747 after 40 000, 1.624 after 60 000 and 1.471 after 80 000 (a = (2.026, -0.897,
    2.533)); sourceLr of 0.03, 0.1 and 0.5 change the third digit only.  Hence 80 000 epochs."""
    a, misfit, err, text = _train(tmp_path / 'learn', learnSource=True)
    a_twin, misfit_twin, err_twin, _ = _train(tmp_path / 'twin')
    dist, dist0 = float(np.linalg.norm(a - A_STAR)), float(np.linalg.norm(A_STAR))
    RECORD['end_to_end/source_amplitudes'] = {'a': [float(x) for x in a], 'distance': dist, 'distance_guess': dist0, 'misfit': misfit,
                                              'misfit_twin': misfit_twin, 'l2_error': float(err), 'l2_error_twin': float(err_twin),
                                              'epochs': EPOCHS}
    print('source amplitudes: a %s (truth %s); |a - a*| %.4f of %.4f; misfit %.4e, frozen twin %.4e; l2 error %.4f, twin %.4f'
          % (a, A_STAR, dist, dist0, misfit, misfit_twin, err, err_twin))
    assert np.array_equal(a_twin, np.zeros(3))
    assert 'Learnt source amplitudes: mask [1, 1, 1], initial [0.0, 0.0, 0.0], final' in text
    assert dist <= dist0 / 3.0
    assert misfit < misfit_twin


def test_loss_lag_blocks_end_in_the_same_amplitudes(tmp_path):
    """train(lossLag=8) ends in the amplitudes (and the epoch) of lossLag=1 when the tolerance is met inside a block: the rollback
    carries the amplitude state."""
    def run(folder, lag, tol, epochs):
        np.random.seed(0)
        vn = VarNet(problem(), layerWidth=[20], activationFun='tanh', discNum=40, bDiscNum=None, tDiscNum=20, learning_rate=0.01,
                    observations=sensors(), learnSource=True)
        res = vn.train(str(folder), weight=[10.0, 10.0, 1.0], epochNum=epochs, tol=tol, saveFreq=1, verbose=False, lossLag=lag)
        out = vn.sourceAmplitudes(), vn.engine.step, vn.engine.get_params(), list(res.loss)
        vn.engine.close()
        return out

    _, _, _, losses = run(tmp_path / 'probe', 1, 0.0, 30)
    tol = float(losses[20]) * (1.0 + 1e-9)
    a_1, step_1, th_1, _ = run(tmp_path / 'lag1', 1, tol, 60)
    a_8, step_8, th_8, _ = run(tmp_path / 'lag8', 8, tol, 60)
    print('lossLag: stopped after %d / %d steps, a %s / %s' % (step_1, step_8, a_1, a_8))
    assert 1 < step_1 < 60 and step_1 == step_8
    assert np.array_equal(a_1, a_8) and np.all(a_1 != 0.0) and np.array_equal(th_1, th_8)
