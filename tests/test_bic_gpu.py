"""
GPU tier of boundary data identification (vn_set_bic_basis, vn_set_bic_learn, vn_get_bic_amps, vn_set_bic_amps;
`VarNet(learnBic=...)`): the amplitude gradient of vn_bicgrad_kernel (vn_learnt.hip) against the fp64 restatement tests/bic_ref.py on
the cases of tests/bic_cases.py -- on the automatic route (with the three polynomial terms the two-pass sequence; without them, on
case 0, the single launch), on the generic kernels, de-duplicated on the case's shared-point map and on one layer-by-layer engine --
loss pieces, lossVec and the theta-gradient at the mixed labels, that a = 0 and learning off give back the bits of an engine without a
basis, the Adam step of the amplitudes over eight steps against tests/learnt_adam_ref.Adam64 with each step's gradient against the
reference at the engine's pre-step parameters (the check that catches a forward of the BC/IC rows enqueued behind the parameters'
update), snapshot / rollback, vn_eval_loss and the fp64 objective at the device amplitudes, every refusal, and one recovery end to end.

Bar per component (tests/bic_cases.py): |g - g64| <= GRAD_RTOL * max(|g64|, 0.01 S_j).  The worst errors are written to
bic_parity.json in the directory VN_RECORD_DIR names (default: profile_out/ beside tests/; committed copy: profiles/bic_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import bic_cases as bc
from tests import learnt_adam_ref as ar
from tests import learnt_cases as lc
from tests.dedup_term_cases import BIDIMVAL, DETJ
from tests.test_dedup_terms_gpu import check_parity
from tests.test_learnt_adam_gpu import build as build_three
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import (VN_COMM_ID_BYTES, VN_KERNEL_AUTO, VN_KERNEL_FUSED, VN_KERNEL_FUSED16, VN_KERNEL_GENERIC, VN_KERNEL_LAYERED,
                               VNEngine, VNError)
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
        with open(os.path.join(out, 'bic_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


# ---- engine-level helpers -------------------------------------------------------------------------------------------
def make_engine(i, route='auto', J=3, optimizer='adam', lr=0.001, label=None, basis=True, terms=True, bic=None, kernel=None):
    """An engine of case i with the case's BC/IC rows (`label`: other labels; `bic`: (biInput, biLabel, B) in place of the case's
    rows and streams), with `terms` the three polynomial terms and with `basis` the J basis streams on the shared set; route
    'dedup' adds the case's shared-point map."""
    d_in, dim, widths, q, n_k, U, nB, bDof, source, integW, td, act = bc.case(i)[:12]
    d = bc.inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW, activationFun=act, optimizer_name=optimizer,
                   learning_rate=lr, kernel=KERNEL.get(route, VN_KERNEL_AUTO) if kernel is None else kernel)
    try:
        eng.set_params(bc.theta(i))
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        biInput, biLabel, B = (d['biInput'], bc.label0_of(i) if label is None else label, bc.basis(i, J)[0]) if bic is None else bic
        eng.set_bic(biInput, biLabel, bDof, BIDIMVAL)
        eng.set_weights(d['w'])
        eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=DETJ)
        if terms:
            nldiff, nlflux, reaction = bc.terms_of(i)
            eng.set_reaction(0, *reaction)
            eng.set_nlflux(0, *nlflux)
            eng.set_nldiff(0, *nldiff)
        if basis:
            eng.set_bic_basis(-1, B)
        if route == 'dedup':
            eng.set_dedup(0, d['Xu'], d['uid'], d['rowptr'], d['rowidx'])
    except Exception:
        eng.close()
        raise
    return eng


def grad_of(eng):
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    return gb.cpu().numpy().copy()


def loss_field(eng):
    out, lv = eng.eval_loss(0, lossVec=True)
    return np.asarray(out, dtype=np.float64), lv.cpu().numpy().copy()


def check_amp_grad(tag, ga, ref, mask=None):
    """ga against the fp64 reference (.., .., g64, S) within the bar, printed and recorded before the assertion."""
    g64, S = ref[2], ref[3]
    J = g64.size
    on = np.ones(J, dtype=bool) if mask is None else np.array(mask, dtype=bool)
    bar = bc.bars(g64, S)
    err = np.abs(ga - g64)
    rel = np.where(on, err / bar, 0.0)
    RECORD[tag] = {'worst_err_over_bar': float(rel.max()), 'worst_component': int(rel.argmax()),
                   'worst_rel_of_g': float(np.max(np.where(on, err / np.abs(g64), 0.0))),
                   'worst_rel_of_S': float(np.max(np.where(on, err / S, 0.0)))}
    print('bic %s: %s' % (tag, json.dumps(RECORD[tag], sort_keys=True)))
    assert np.all(np.isfinite(ga))
    assert np.all(ga[~on] == 0.0), (tag, ga)
    assert np.all(err[on] <= bar[on]), (tag, ga, g64, bar)


def gradient_checks(i, J, route, mask=None):
    tag = '%s/J%d/%s' % (bc.IDS[i], J, route)
    B, amp = bc.basis(i, J)
    m = [1] * J if mask is None else mask
    net = (bc.case(i)[0], bc.case(i)[1], bc.case(i)[2], bc.case(i)[10])
    eng = make_engine(i, route, J)
    try:
        # learning off: a registered basis is not read (the bits of an engine that has none)
        g_off, (l_off, lv_off) = grad_of(eng), loss_field(eng)
        if J == 3:
            bare = make_engine(i, route, J, basis=False)
            try:
                assert np.array_equal(grad_of(bare), g_off), tag
                lb, lvb = loss_field(bare)
                assert np.array_equal(lb, l_off) and np.array_equal(lvb, lv_off), tag
            finally:
                bare.close()
            # a = 0: loss pieces, lossVec and theta-gradient are bitwise those of the engine without a basis
            eng.set_bic_learn(m, np.zeros(J), lr=0.01)
            assert np.array_equal(grad_of(eng), g_off), tag
            l0, lv0 = loss_field(eng)
            assert np.array_equal(l0, l_off) and np.array_equal(lv0, lv_off), tag
        eng.set_bic_learn(m, amp, lr=0.01)
        ref = bc.reference64(i, J)
        g32 = lambda: bc.evaluate(i, J, dtype=torch.float32)[1]
        g_on = check_parity(i, eng, tag, ref[:2], g32, net=net, record=RECORD)
        assert not np.array_equal(g_on, g_off), tag                           # the amplitudes count
        a, ga = eng.get_bic_amps(grad=True)
        assert np.array_equal(a, amp)
        check_amp_grad(tag + '/amp', ga, ref, mask)
        grad_of(eng)
        assert np.array_equal(eng.get_bic_amps(grad=True)[1], ga), tag        # two evaluations: the same J doubles
        eng.set_bic_learn(None)
        assert np.array_equal(grad_of(eng), g_off), tag                       # learning off again: the parent's bits
        with pytest.raises(VNError, match='error 3: no learnt boundary and initial amplitudes'):
            eng.get_bic_amps(J=J)
    finally:
        eng.close()


# ---- 1. the amplitude gradient ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['auto', 'generic', 'dedup'])
@pytest.mark.parametrize('i', range(bc.N_CASES), ids=bc.IDS)
def test_amplitude_gradient(i, route):
    gradient_checks(i, 3, route)


@pytest.mark.parametrize('route', ['auto', 'generic', 'dedup'])
@pytest.mark.parametrize('J', [1, 64])
@pytest.mark.parametrize('i', bc.WIDE, ids=[bc.IDS[k] for k in bc.WIDE])
def test_one_and_sixty_four_streams(i, J, route):
    gradient_checks(i, J, route)


@pytest.mark.parametrize('route', ['auto', 'generic', 'dedup'])
@pytest.mark.parametrize('i', bc.WIDE, ids=[bc.IDS[k] for k in bc.WIDE])
def test_masked_amplitudes(i, route):
    """Mask [1, 0, 1, 0, 0]: the unmasked gradients read 0 (gradient_checks), the unmasked amplitudes take part in the labels at
    their initial values and keep their bits through two steps."""
    gradient_checks(i, 5, route, mask=bc.MASK5)
    amp = bc.basis(i, 5)[1]
    eng = make_engine(i, route, 5)
    try:
        eng.set_bic_learn(bc.MASK5, amp, lr=0.05)
        eng.train_epoch([0, 0])
        torch.cuda.synchronize()
        got = eng.get_bic_amps()
        on = np.array(bc.MASK5, dtype=bool)
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


def test_single_launch_route_is_kept():
    """A batch without any polynomial term runs the single-launch 8-wave kernel, and keeps it with learning on: vn_kernel_path
    reports it, the theta-gradient and the loss pieces are bitwise those of an engine given the pre-mixed labels (which has no
    reason to leave the single launch), and the amplitude gradient is the reference's of that problem."""
    i, J = 0, 3
    B, amp = bc.basis(i, J)
    eng, plain = make_engine(i, J=J, terms=False), make_engine(i, J=J, terms=False, label=bc.fma_mix(i, J, amp), basis=False)
    try:
        assert eng.kernel_path() == plain.kernel_path() and eng.kernel_path()[0] == VN_KERNEL_FUSED16 and eng.kernel_path()[1] == 0
        eng.set_bic_learn([1] * J, amp, lr=0.01)
        assert eng.kernel_path()[0] == VN_KERNEL_FUSED16 and eng.kernel_path()[1] == 0
        g = grad_of(eng)
        assert np.array_equal(g, grad_of(plain))
        ga = eng.get_bic_amps(grad=True)[1]
        ref = bc.evaluate(i, J, terms=False)
        assert np.all(ref[2] != 0.0)
        check_amp_grad('%s/J%d/single_launch/amp' % (bc.IDS[i], J), ga, ref)
        grad_of(eng)
        assert np.array_equal(eng.get_bic_amps(grad=True)[1], ga)
    finally:
        eng.close()
        plain.close()


@pytest.mark.parametrize('k', range(len(bc.BIG)), ids=bc.BIG_IDS)
def test_amplitude_gradient_on_a_capped_grid(k):
    """More BC/IC rows than the capped reduction grid has threads: every thread of a partial takes several rows.  The learnt
    components are well conditioned in the reference (asserted before the device is looked at)."""
    i, J, mask = bc.N_CASES + k, bc.BIG_J, bc.BIG_MASK
    ref = bc.reference64(i, J)
    on = np.array(mask, dtype=bool)
    assert np.all(np.abs(ref[2][on]) >= bc.COND_FLOOR * ref[3][on]), (ref[2], ref[3])
    amp = bc.basis(i, J)[1]
    for route in ('auto', 'generic', 'dedup'):
        eng = make_engine(i, route, J)
        try:
            eng.set_bic_learn(mask, amp, lr=0.01)
            grad_of(eng)
            ga = eng.get_bic_amps(grad=True)[1]
            check_amp_grad('%s/J%d/%s/amp' % (bc.BIG_IDS[k], J, route), ga, ref, mask)
            grad_of(eng)
            assert np.array_equal(eng.get_bic_amps(grad=True)[1], ga)
        finally:
            eng.close()


def test_steady_case_ignores_the_rows_behind_bDof():
    """A steady engine evaluates the first bDof rows: garbage in the labels, the inputs and the streams behind them changes no bit."""
    i, J = 5, 3
    B, amp = bc.basis(i, J)
    d = bc.inputs(i)
    nB, extra = B.shape[1], 7
    rng = np.random.default_rng(77)
    junk = np.array([1e30, -1e30, np.nan, np.inf, 3.0, -np.inf, 1e-30], dtype=np.float32)
    bic = (np.concatenate([d['biInput'], rng.uniform(-50, 50, (extra, d['biInput'].shape[1])).astype(np.float32)]),
           np.concatenate([bc.label0_of(i), junk]), np.concatenate([B, np.tile(junk[::-1], (J, 1))], axis=1))
    assert not bc.case(i)[10] and bic[0].shape[0] == nB + extra
    for route in ('auto', 'generic', 'dedup'):
        a, b = make_engine(i, route, J), make_engine(i, route, J, bic=bic)
        try:
            out = []
            for e in (a, b):
                e.set_bic_learn([1] * J, amp, lr=0.01)
                g = grad_of(e)
                out.append((g, e.get_bic_amps(grad=True)[1], loss_field(e)))
            assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), route
            assert np.array_equal(out[0][2][0], out[1][2][0]) and np.array_equal(out[0][2][1], out[1][2][1]), route
            assert np.all(out[0][1] != 0.0)
        finally:
            a.close()
            b.close()


def test_batch_with_its_own_permuted_copy():
    """A batch with its own BC/IC copy (vn_set_batch_bic) and that copy's basis, rows permuted within the boundary and within
    the initial block: the amplitude gradient of the unpermuted set within the bar.  Without a copy the registration is refused;
    a new copy and vn_set_interior clear it."""
    i, J = 0, 3
    B, amp = bc.basis(i, J)
    d = bc.inputs(i)
    nB, bDof = bc.case(i)[6], bc.case(i)[7]
    rng = np.random.default_rng(5)
    perm = np.concatenate([rng.permutation(bDof), bDof + rng.permutation(nB - bDof)])
    ref = bc.reference64(i, J)
    for route in ('auto', 'generic', 'dedup'):
        eng = make_engine(i, route, J, basis=False)
        try:
            with pytest.raises(VNError, match='error 3: batch 0 has no BC/IC rows of its own'):
                eng.set_bic_basis(0, B[:, perm])
            eng.set_batch_bic(0, d['biInput'][perm], bc.label0_of(i)[perm])
            eng.set_bic_basis(0, B[:, perm])
            eng.set_bic_learn([1] * J, amp, lr=0.01)
            grad_of(eng)
            ga = eng.get_bic_amps(grad=True)[1]
            check_amp_grad('%s/J%d/%s/permuted_copy/amp' % (bc.IDS[i], J, route), ga, ref)
            # a new copy drops the basis: nothing to reduce, the labels are the copy's own
            eng.set_batch_bic(0, d['biInput'][perm], bc.label0_of(i)[perm])
            grad_of(eng)
            assert np.all(eng.get_bic_amps(grad=True)[1] == 0.0)
            # the shared set's basis does not serve a batch that reads its own copy
            eng.set_bic_basis(-1, B)
            grad_of(eng)
            assert np.all(eng.get_bic_amps(grad=True)[1] == 0.0)
            eng.set_batch_bic(0)
            grad_of(eng)
            check_amp_grad('%s/J%d/%s/back_on_the_shared_set/amp' % (bc.IDS[i], J, route), eng.get_bic_amps(grad=True)[1], ref)
        finally:
            eng.close()


@pytest.mark.parametrize('route', ['auto', 'dedup'])
@pytest.mark.parametrize('i', lc.CASES, ids=lc.IDS)
def test_next_to_the_other_three_vectors(i, route):
    """All four vectors learning on one engine: the three others' gradients are bitwise those of an engine given the pre-mixed
    labels, the BC/IC amplitude gradient is bitwise that of an engine that learns nothing else (it reads the parameters and the
    labels only); one step moves all four on one counter."""
    J = 3
    B, amp = bc.basis(i, J)
    three = build_three(i, route, [lc.whole(i)])
    try:
        three.set_bic(lc.whole(i)['biInput'], bc.fma_mix(i, J, amp), bc.case(i)[7], BIDIMVAL)
        grad_of(three)
        alone3 = {k: getattr(three, 'get_' + n)(grad=True)[1] for k, n in (('coef', 'coefs'), ('source', 'source_amps'), ('field', 'field_amps'))}
    finally:
        three.close()
    alone = make_engine(i, route, J)
    try:
        alone.set_bic_learn([1] * J, amp, lr=0.01)
        grad_of(alone)
        ga_alone = alone.get_bic_amps(grad=True)[1]
    finally:
        alone.close()
    eng = build_three(i, route, [lc.whole(i)])
    try:
        eng.set_bic_basis(-1, B)
        eng.set_bic_learn([1] * J, amp, lr=0.01)
        grad_of(eng)
        got = {k: getattr(eng, 'get_' + n)(grad=True) for k, n in (('coef', 'coefs'), ('source', 'source_amps'), ('field', 'field_amps'),
                                                                    ('bic', 'bic_amps'))}
        for k in alone3:
            assert np.array_equal(got[k][1], alone3[k]) and np.all(alone3[k] != 0.0), (k, got[k][1], alone3[k])
        assert np.array_equal(got['bic'][1], ga_alone) and np.all(ga_alone != 0.0), (got['bic'][1], ga_alone)
        eng.train_step(0)
        torch.cuda.synchronize()
        assert eng.step == 1
        for k, n in (('coef', 'coefs'), ('source', 'source_amps'), ('field', 'field_amps'), ('bic', 'bic_amps')):
            assert np.all(getattr(eng, 'get_' + n)() != got[k][0]), k
    finally:
        eng.close()


def test_next_to_flux_rows_periodic_pairs_and_observations():
    """The edge passes do not read the labels: with all three registered the amplitude gradient is what it was."""
    i, J = 0, 3
    d_in, dim = bc.case(i)[0], bc.case(i)[1]
    rng = np.random.default_rng(31)
    for route in ('auto', 'dedup'):
        eng = make_engine(i, route, J)
        try:
            eng.set_bic_learn([1] * J, bc.basis(i, J)[1], lr=0.01)
            grad_of(eng)
            before = eng.get_bic_amps(grad=True)[1]
            nrm = rng.standard_normal((17, dim)).astype(np.float32)
            eng.set_flux_bc(rng.uniform(-1, 1, (17, d_in)).astype(np.float32), nrm, rng.uniform(0, 1, 17).astype(np.float32),
                            rng.standard_normal(17).astype(np.float32), BIDIMVAL)
            eng.set_periodic(rng.uniform(-1, 1, (22, d_in)).astype(np.float32), rng.standard_normal((22, dim)).astype(np.float32), 1.0,
                             BIDIMVAL)
            eng.set_observations(rng.uniform(-1, 1, (33, d_in)).astype(np.float32), rng.standard_normal(33).astype(np.float32), weight=2.0)
            grad_of(eng)
            assert np.array_equal(eng.get_bic_amps(grad=True)[1], before)
        finally:
            eng.close()


# ---- 2. the step ----------------------------------------------------------------------------------------------------------
STEP_LR, STEP_ENGINE_LR, STEPS = 0.02, 0.01, 8
STEP_RUNS = [(0, 'auto', False), (0, 'dedup', True), (6, 'auto', True), (6, 'dedup', True)]
STEP_IDS = ['%s-%s' % (bc.IDS[i], 'single_launch' if not terms else route) for i, route, terms in STEP_RUNS]


@pytest.mark.parametrize('i,route,terms', STEP_RUNS, ids=STEP_IDS)
def test_eight_steps_follow_adam_on_the_reference_gradient(i, route, terms):
    """Eight steps, odd ones through vn_train_step and even ones through vn_grad + vn_apply.  Before each step parameters and
    amplitudes are read back; after it the engine's amplitude gradient has to be within the gradient bar of the fp64 reference AT
    THOSE parameters (a forward of the BC/IC rows enqueued behind the reduction that folds the parameters' update in would show
    the next step's), and the amplitudes within the per-step bar of tests/learnt_adam_ref (half an ulp plus C lr_t) of Adam64
    started from the values before the step, on the engine's gradient; unmasked entries keep their bits."""
    J, mask = 5, [1, 1, 0, 1, 1]
    tag = 'steps/%s' % STEP_IDS[STEP_RUNS.index((i, route, terms))]
    amp = bc.basis(i, J)[1]
    on = np.array(mask, dtype=bool)
    eng = make_engine(i, route, J, lr=STEP_ENGINE_LR, terms=terms)
    try:
        if not terms:
            assert eng.kernel_path()[0] == VN_KERNEL_FUSED16 and eng.kernel_path()[1] == 0
        eng.set_bic_learn(mask, amp, lr=STEP_LR)
        adam = ar.Adam64(J, mask, STEP_LR)
        worst_g = worst_a = 0.0
        th0 = None
        for t in range(1, STEPS + 1):
            torch.cuda.synchronize()
            theta, before = eng.get_params(), eng.get_bic_amps()
            if th0 is None:
                th0 = theta.copy()
            if t % 2:
                eng.train_step(0)
            else:
                eng.grad(0)
                eng.apply()
            torch.cuda.synchronize()
            after, g = eng.get_bic_amps(grad=True)
            assert eng.step == t
            ref = bc.evaluate(i, J, amp=before, flat=theta, terms=terms)
            bar_g = bc.bars(ref[2], ref[3])
            rel_g = float(np.max(np.where(on, np.abs(g - ref[2]) / bar_g, 0.0)))
            want = adam.step(before, g, t)
            bar_a = ar.bar(before, want, adam.lr_t(t))
            rel_a = float(np.max(np.where(on, np.abs(after - want) / bar_a, 0.0)))
            worst_g, worst_a = max(worst_g, rel_g), max(worst_a, rel_a)
            print('%s step %d: gradient err/bar %.3f, amplitude err/bar %.3f' % (tag, t, rel_g, rel_a))
            assert np.all(g[~on] == 0.0) and np.array_equal(after[~on], before[~on]), (tag, t)
            assert rel_g <= 1.0, (tag, t, g, ref[2], bar_g)
            assert rel_a <= 1.0, (tag, t, after, want, bar_a)
        # the check has teeth: the reference at the parameters one step on leaves the gradient bar of the first step
        ref0, ref1 = bc.evaluate(i, J, amp=amp, flat=th0, terms=terms), None
        eng2 = make_engine(i, route, J, lr=STEP_ENGINE_LR, terms=terms)
        try:
            eng2.set_bic_learn(mask, amp, lr=STEP_LR)
            eng2.train_step(0)
            torch.cuda.synchronize()
            ref1 = bc.evaluate(i, J, amp=amp, flat=eng2.get_params(), terms=terms)
        finally:
            eng2.close()
        late = float(np.max(np.where(on, np.abs(ref1[2] - ref0[2]) / bc.bars(ref0[2], ref0[3]), 0.0)))
        print('%s: the gradient at the next step\'s parameters is %.1f bars away' % (tag, late))
        assert late > 2.0, (tag, late)
        RECORD[tag] = {'worst_gradient_err_over_bar': worst_g, 'worst_amplitude_err_over_bar': worst_a,
                       'next_step_parameters_bars_away': late}
        assert np.all(eng.get_bic_amps()[on] != amp[on])
    finally:
        eng.close()


def _state(eng):
    torch.cuda.synchronize()
    return np.asarray(eng.export_state()).copy(), eng.get_bic_amps()


@pytest.mark.parametrize('route', ['auto', 'dedup'])
def test_train_epoch_snapshot_and_rollback(route):
    """vn_train_epoch over [0, 0, 0, 0] is bitwise four single steps, parameters, slots and amplitudes; snapshot -> three steps ->
    rollback restores amplitudes, their slots and the step counter bitwise (the replayed steps end in the same bits);
    vn_set_bic_amps and vn_set_bic_basis invalidate the snapshot."""
    i, J = 6, 3
    B, amp = bc.basis(i, J)
    a, b = make_engine(i, route, J, lr=0.01), make_engine(i, route, J, lr=0.01)
    try:
        for e in (a, b):
            e.set_bic_learn([1] * J, amp, lr=0.02)
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
        a.set_bic_amps(amp)
        with pytest.raises(VNError, match='error 3: no snapshot to roll back to'):
            a.state_rollback()
        a.state_snapshot()
        a.set_bic_basis(-1, B)
        with pytest.raises(VNError, match='error 3: no snapshot to roll back to'):
            a.state_rollback()
    finally:
        a.close()
        b.close()


# ---- 3. evaluations at the device amplitudes ----------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['auto', 'generic', 'dedup'])
def test_evaluations_at_the_device_amplitudes(route):
    """After vn_set_bic_amps(a') vn_eval_loss, vn_grad and vn_objective_f64 equal those of an engine given the pre-mixed labels:
    the fp32 results bitwise (the same kernels read the same bits), the fp64 objective at the bars of tests/test_obj64_gpu.py
    (loss pieces 1e-12, gradient 1e-11 of its maximum)."""
    i, J = 1, 3
    amp = bc.basis(i, J)[1]
    a1 = (amp * np.array([1.5, -0.5, 2.0])).astype(np.float32).astype(np.float64)
    a, b = make_engine(i, route, J), make_engine(i, route, J, label=bc.fma_mix(i, J, a1), basis=False)
    try:
        a.set_bic_learn([1] * J, amp, lr=0.01)
        out0 = a.objective64(0)[0]
        a.set_bic_amps(a1)
        assert np.array_equal(a.get_bic_amps(), a1)
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
    B, amp = bc.basis(i, J)
    n_k = bc.case(i)[4]
    ones = [1] * J
    for opt, word in (('rmsprop', 'an RMSProp'), ('lbfgs', 'an L-BFGS')):
        eng = make_engine(i, optimizer=opt)
        try:
            with pytest.raises(VNError, match='error 5: vn_set_bic_learn on %s engine' % word):
                eng.set_bic_learn(ones, amp, lr=0.01)
        finally:
            eng.close()
    eng = make_engine(i)
    try:
        bad = amp.copy()
        bad[1] = np.nan
        with pytest.raises(VNError, match='error 1: initial amplitude 1'):
            eng.set_bic_learn(ones, bad, lr=0.01)
        lo, hi = np.full(J, -np.inf), np.full(J, np.inf)
        lo[2], hi[2] = 1.0, 0.5
        with pytest.raises(VNError, match='error 1: bounds of amplitude 2'):
            eng.set_bic_learn(ones, amp, lo, hi, lr=0.01)
        for lr in (0.0, -1.0, float('nan')):
            with pytest.raises(VNError, match='error 1: amplitude learning rate'):
                eng.set_bic_learn(ones, amp, lr=lr)
        with pytest.raises(VNError, match='error 1: 1 to 64 boundary and initial amplitudes can be learnt, got 65'):
            eng.set_bic_learn([1] * 65, np.zeros(65), lr=0.01)
        with pytest.raises(VNError, match='error 3: no learnt boundary and initial amplitudes'):
            eng.set_bic_amps(amp)
        with pytest.raises(VNError, match='error 1: a BC/IC basis has 1 to 64 streams, got 65'):
            eng.set_bic_basis(-1, np.zeros((65, B.shape[1]), dtype=np.float32))
        with pytest.raises(VNError, match='error 3: batch 3 has no interior data'):
            eng.set_bic_basis(3, B)
        # (a failed call leaves the set without a basis: learning on, the step runs with nothing to reduce)
        eng.set_bic_learn(ones, amp, lr=0.01)
        grad_of(eng)
        assert np.all(eng.get_bic_amps(grad=True)[1] == 0.0)
        # a basis of another J than the learnt vector's: the step, the loss-only evaluation and the fp64 objective
        eng.set_bic_basis(-1, bc.basis(i, 5)[0])
        for call in (lambda: eng.grad(0), lambda: eng.train_step(0), lambda: eng.eval_loss(0), lambda: eng.objective64(0)):
            with pytest.raises(VNError, match='error 1: the BC/IC rows of batch 0 have a basis of 5 streams, the learnt amplitudes .* are 3'):
                call()
        assert eng.step == 0
        eng.set_bic_basis(-1, B)
        with pytest.raises(VNError, match='error 1: the engine holds 3 boundary and initial amplitudes'):
            eng.get_bic_amps(J=5)
        with pytest.raises(VNError, match='error 1: the engine holds 3 boundary and initial amplitudes'):
            eng.set_bic_amps(np.zeros(5))
        with pytest.raises(VNError, match='error 1: amplitude 0'):
            eng.set_bic_amps([np.inf, 0.0, 0.0])
        # per-test-function weights and learning, in either order
        with pytest.raises(VNError, match='error 5: learnt boundary and initial amplitudes .* next to per-test-function loss weights'):
            eng.set_tf_weights(0, np.ones(n_k, dtype=np.float32))
        eng.set_bic_learn(None)
        eng.set_tf_weights(0, np.ones(n_k, dtype=np.float32))
        with pytest.raises(VNError, match=r'error 5: learnt boundary and initial amplitudes \(vn_set_bic_learn\) next to per-test-function loss weights'):
            eng.set_bic_learn(ones, amp, lr=0.01)
        eng.set_tf_weights(0, None)
        eng.set_bic_learn(ones, amp, lr=0.01)
        with pytest.raises(VNError, match='error 5: vn_comm_init while boundary and initial amplitudes are learnt'):
            eng.comm_init(0, 1, bytes(VN_COMM_ID_BYTES))
        # vn_set_bic clears the shared set's basis
        d = bc.inputs(i)
        grad_of(eng)
        assert np.all(eng.get_bic_amps(grad=True)[1] != 0.0)
        eng.set_bic(d['biInput'], bc.label0_of(i), bc.case(i)[7], BIDIMVAL)
        grad_of(eng)
        assert np.all(eng.get_bic_amps(grad=True)[1] == 0.0)
    finally:
        eng.close()
    # the 4-wave cross-check geometry carries no values of the BC/IC rows
    eng = make_engine(0, kernel=VN_KERNEL_FUSED, terms=False)
    try:
        with pytest.raises(VNError, match='error 5: learnt boundary and initial amplitudes are not built for VN_KERNEL_FUSED'):
            eng.set_bic_learn(ones, bc.basis(0, J)[1], lr=0.01)
    finally:
        eng.close()
    # an engine without BC/IC rows has no label to mix
    d_in, dim, widths, q, n_k, U, nB, bDof, source, integW, td, act = bc.case(i)[:12]
    d = bc.inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW, activationFun=act)
    try:
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=DETJ)
        with pytest.raises(VNError, match='error 1: no BC/IC rows are registered'):
            eng.set_bic_basis(-1, B)
    finally:
        eng.close()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
KAPPA, T_END = 0.1, 0.5
A_STAR = np.array([1.0, -0.5])
MODES = (1, 2)
EPOCHS, BIC_LR, WEIGHT = 30000, 0.01, [10.0, 10.0, 1.0]     # see test_recovers_the_initial_amplitudes


def u_star(x, t):
    """The solution of c_t = kappa c_xx with zero boundary values from c(x, 0) = sum_j a*_j sin(j pi x)."""
    return sum(a * np.sin(j * pi * x) * np.exp(-KAPPA * j * j * pi * pi * t) for a, j in zip(A_STAR, MODES))


def sensors(seed=0):
    rng = np.random.default_rng(seed)
    x, t = rng.uniform(0, 1, 64), rng.uniform(0, T_END, 64)
    return np.column_stack([x, t]), u_star(x, t)


def problem():
    return ADPDE(Domain1D(np.array([0.0, 1.0])), diff=KAPPA, vel=0.0, tInterval=[0, T_END], IC=lambda x: 0.0 * x, cEx=u_star,
                 icBasis=[lambda x, j=j: np.sin(j * pi * x) for j in MODES], icAmp=[0.0, 0.0])


def train(folder, epochs=None, checkpoints=(), **vn_kw):
    """One training of the end-to-end problem; `checkpoints`: epoch counts at which the amplitudes are noted (further train() calls)."""
    np.random.seed(0)
    vn = VarNet(problem(), layerWidth=[20], activationFun='tanh', discNum=40, bDiscNum=None, tDiscNum=20, learning_rate=0.01,
                observations=sensors(), **vn_kw)
    epochs = EPOCHS if epochs is None else epochs
    vn.train(str(folder), weight=WEIGHT, epochNum=epochs, tol=0.0, saveFreq=epochs, verbose=False)
    a = vn.bicAmplitudes()['ic']
    out = a, vn.obsMisfit(), vn.residual()[2]
    text = open(os.path.join(str(folder), 'caseData.txt')).read()
    vn.engine.close()
    return out + (text,)


def test_recovers_the_initial_amplitudes(tmp_path):
    """c_t = kappa c_xx on [0, 1] x [0, 0.5] with zero Dirichlet ends, c(x, 0) = sum_j a_j sin(j pi x), truth a* = (1, -0.5), guess
    a = 0, 64 point sensors over the whole space-time rectangle.  Required: ||a - a*|| falls to a third of the guess's (1.118), and
    the misfit ends below that of the twin trained with the amplitudes frozen at the guess.  The first mode is found at once, the
    second follows the network, which takes up sin(2 pi x) e^{-4 kappa pi^2 t} slowly: measured on one MI355X (seed fixed, bicLr at
    its default 0.01, weight (10, 10, 1)), ||a - a*|| is 0.493 after 2 000 epochs, 0.471 after 4 000, 0.440 after 6 000, 0.433 after
    8 000, 0.427 after 10 000, 0.387 after 15 000, 0.361 after 20 000 (the first count below the bar 0.3727) and 0.339 after 30 000
    (a = (1.025, -0.162)); bicLr of 0.03 and 0.1 change the second digit only, an IC weight of 100 slows the second mode down (0.473
    after 30 000).  Hence 30 000 epochs: the first count that meets the bar, plus one checkpoint."""
    a, misfit, err, text = train(tmp_path / 'learn', learnBic={'ic': True}, bicLr=BIC_LR)
    a_twin, misfit_twin, err_twin, _ = train(tmp_path / 'twin')
    dist, dist0 = float(np.linalg.norm(a - A_STAR)), float(np.linalg.norm(A_STAR))
    RECORD['end_to_end/initial_amplitudes'] = {'a': [float(x) for x in a], 'distance': dist, 'distance_guess': dist0, 'misfit': misfit,
                                               'misfit_twin': misfit_twin, 'l2_error': float(err), 'l2_error_twin': float(err_twin),
                                               'epochs': EPOCHS, 'bicLr': BIC_LR}
    print('initial amplitudes: a %s (truth %s); |a - a*| %.4f of %.4f; misfit %.4e, frozen twin %.4e; l2 error %.4f, twin %.4f'
          % (a, A_STAR, dist, dist0, misfit, misfit_twin, err, err_twin))
    assert np.array_equal(a_twin, np.zeros(2))
    assert 'Learnt boundary and initial amplitudes (bc, then ic): mask [1, 1], initial [0.0, 0.0], final' in text
    assert dist <= dist0 / 3.0
    assert misfit < misfit_twin
