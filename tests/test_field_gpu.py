"""
GPU tier of field identification (vn_set_field_basis, vn_set_field_learn, vn_get_field_amps, vn_set_field_amps;
`VarNet(learnField=...)`): the amplitude gradient of vn_learnt.hip against the fp64 restatement tests/field_ref.py on the cases of
tests/field_cases.py -- row-wise on the automatic route (the two-pass sequence; for integ_num > 128 the two-pass route itself) and
on the generic kernels, de-duplicated on the case's shared-point map (for the EMPTY cases also the map with row-less points) --
loss pieces, lossVec and the theta-gradient at the mixed gcoef, that b = 0 and learning off give back the bits of an engine without
a basis, that gcoef follows the amplitudes every step, the Adam step of the amplitudes, snapshot / rollback, the fp64 objective at
the device amplitudes, the three learnt vectors together, every refusal, and one recovery end to end.

Bar per component (tests/field_cases.py): |g - g64| <= GRAD_RTOL * max(|g64|, 0.01 S_j).  The worst errors are written to
field_parity.json in the directory VN_RECORD_DIR names (default: profile_out/ beside tests/; committed copy:
profiles/field_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import field_cases as fc
from tests import source_cases as sc
from tests.dedup_term_cases import BIDIMVAL, CASES, DETJ, DIFF, PERIODIC, empty_map
from tests.test_dedup_terms_gpu import check_parity
from tests.test_source_gpu import fma_mix as source_fma_mix
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import (VN_COMM_ID_BYTES, VN_KERNEL_AUTO, VN_KERNEL_FUSED, VN_KERNEL_GENERIC, VN_KERNEL_LAYERED, VNEngine,
                               VNError)
from varnet_amd.varnet import VarNet

pytestmark = pytest.mark.gpu

pi = np.pi
RECORD = {}
KERNEL = {'generic': VN_KERNEL_GENERIC, 'layered': VN_KERNEL_LAYERED}
DEGENERATE = (0.0, 0.0, 1.0)


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'field_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


# ---- engine-level helpers -------------------------------------------------------------------------------------------
def make_engine(i, route='auto', J=3, empty=False, optimizer='adam', lr=0.001, gcoef=None, source=None, basis=True, dcoef=None,
                dedup_first=False):
    """An engine of case i with has_source, the case's gcoef (`gcoef`: another direction) and s0 (`source`: another stream), the
    three polynomial terms (`dcoef`: other coefficients of D(u)) and, with `basis`, the J basis streams; route 'dedup' adds the
    case's shared-point map, before the basis with `dedup_first`."""
    d_in, dim, widths, q, n_k, U, nB, bDof, _, integW, td, act = fc.case(i)[:12]
    d = fc.inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=True, integWflag=integW, activationFun=act, optimizer_name=optimizer,
                   learning_rate=lr, kernel=KERNEL.get(route, VN_KERNEL_AUTO))
    eng.set_params(fc.theta(i))
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, BIDIMVAL)
    eng.set_weights(d['w'])
    eng.set_interior(0, d['Input'], d['gcoef'] if gcoef is None else gcoef, fc.s0_of(i) if source is None else source, n_k=n_k,
                     detJ=DETJ)
    nldiff, nlflux, reaction = fc.terms_of(i)
    eng.set_reaction(0, *reaction)
    eng.set_nlflux(0, *nlflux)
    eng.set_nldiff(0, nldiff[0], nldiff[1] if dcoef is None else dcoef)

    def dedup():
        if route == 'dedup':
            Xu, rowptr = empty_map(sc.base(i)) if empty else (d['Xu'], d['rowptr'])
            eng.set_dedup(0, Xu, d['uid'], rowptr, d['rowidx'])
    if dedup_first:
        dedup()
    if basis:
        eng.set_field_basis(0, fc.basis(i, J)[0])
    if not dedup_first:
        dedup()
    return eng


def grad_of(eng):
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    return gb.cpu().numpy().copy()


def loss_field(eng):
    out, lv = eng.eval_loss(0, lossVec=True)
    return np.asarray(out, dtype=np.float64), lv.cpu().numpy().copy()


def check_amp_grad(tag, gb, g64, S, mask=None):
    """gb against the fp64 reference within the bar, printed and recorded before the assertion.  Returns the bar."""
    J = g64.size
    on = np.ones(J, dtype=bool) if mask is None else np.array(mask, dtype=bool)
    bar = fc.bars(g64, S)
    err = np.abs(gb - g64)
    rel = np.where(on, err / bar, 0.0)
    RECORD[tag] = {'worst_err_over_bar': float(rel.max()), 'worst_component': int(rel.argmax()),
                   'worst_rel_of_g': float(np.max(np.where(on, err / np.abs(g64), 0.0))),
                   'worst_rel_of_S': float(np.max(np.where(on, err / S, 0.0)))}
    print('field %s: %s' % (tag, json.dumps(RECORD[tag], sort_keys=True)))
    assert np.all(np.isfinite(gb))
    assert np.all(gb[~on] == 0.0), (tag, gb)
    assert np.all(err[on] <= bar[on]), (tag, gb, g64, bar)
    return bar


def reads_csr(i, route):
    """The parent's de-duplicated step of case i reads the CSR-ordered copy of gcoef (not the periodic table)."""
    return route == 'dedup' and sc.base(i) not in PERIODIC


def gradient_checks(i, J, route, empty=False, mask=None):
    tag = '%s/J%d/%s%s' % (fc.IDS[i], J, route, '/empty_points' if empty else '')
    G, amp = fc.basis(i, J)
    m = [1] * J if mask is None else mask
    net = (fc.case(i)[0], fc.case(i)[1], fc.case(i)[2], fc.case(i)[10])
    eng = make_engine(i, route, J, empty)
    try:
        # learning off: a registered basis is not read (the bits of an engine that has none, a gper batch included)
        g_off, (l_off, lv_off) = grad_of(eng), loss_field(eng)
        if J == 3:
            bare = make_engine(i, route, J, empty, basis=False)
            try:
                assert np.array_equal(grad_of(bare), g_off), tag
                lb, lvb = loss_field(bare)
                assert np.array_equal(lb, l_off) and np.array_equal(lvb, lv_off), tag
            finally:
                bare.close()
            if route != 'dedup' or reads_csr(i, route):
                # b = 0: loss pieces, lossVec and theta-gradient are bitwise those of the engine without a basis on the same route
                eng.set_field_learn(m, np.zeros(J), lr=0.01)
                assert np.array_equal(grad_of(eng), g_off), tag
                l0, lv0 = loss_field(eng)
                assert np.array_equal(l0, l_off) and np.array_equal(lv0, lv_off), tag
        eng.set_field_learn(m, amp, lr=0.01)
        ref = fc.reference64(i, J)
        g32 = lambda: fc.evaluate(i, J, dtype=torch.float32)[1]
        g_on = check_parity(sc.base(i), eng, tag, ref[:2], g32, net=net, record=RECORD)
        assert not np.array_equal(g_on, g_off), tag                           # the amplitudes count
        a, gb = eng.get_field_amps(grad=True)
        assert np.array_equal(a, amp)
        check_amp_grad(tag + '/amp', gb, ref[2], ref[3], mask)
        grad_of(eng)
        assert np.array_equal(eng.get_field_amps(grad=True)[1], gb), tag      # two evaluations: the same J doubles
        eng.set_field_learn(None)
        assert np.array_equal(grad_of(eng), g_off), tag                       # learning off again: the parent's bits
        with pytest.raises(VNError, match='error 3: no learnt field amplitudes'):
            eng.get_field_amps(J=J)
        return gb
    finally:
        eng.close()


# ---- 1. the amplitude gradient ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['auto', 'generic', 'dedup'])
@pytest.mark.parametrize('i', range(fc.N_CASES), ids=fc.IDS)
def test_amplitude_gradient(i, route):
    gradient_checks(i, 3, route)


@pytest.mark.parametrize('i', fc.EMPTY, ids=[fc.IDS[k] for k in fc.EMPTY])
def test_amplitude_gradient_with_rowless_points(i):
    gradient_checks(i, 3, 'dedup', empty=True)


@pytest.mark.parametrize('i', range(fc.N_CASES), ids=fc.IDS)
def test_deduplicated_against_row_wise(i):
    """The two formulations sum the same rows in another order and take grad u from another point pass: inside the sum of their
    bars."""
    J = 3
    G, amp = fc.basis(i, J)
    got = {}
    for route in ('auto', 'dedup'):
        eng = make_engine(i, route, J, dedup_first=True)
        try:
            eng.set_field_learn([1] * J, amp, lr=0.01)
            grad_of(eng)
            got[route] = eng.get_field_amps(grad=True)[1]
        finally:
            eng.close()
    _, _, g64, S = fc.reference64(i, J)
    bar = fc.bars(g64, S)
    print('field %s dedup - rowwise over 2 bar: %s' % (fc.IDS[i], np.abs(got['auto'] - got['dedup']) / (2 * bar)))
    assert np.all(np.abs(got['auto'] - got['dedup']) <= 2 * bar), (got, bar)


@pytest.mark.parametrize('route', ['auto', 'dedup'])
@pytest.mark.parametrize('J', [1, fc.JMAX])
@pytest.mark.parametrize('i', fc.WIDE, ids=[fc.IDS[k] for k in fc.WIDE])
def test_one_and_thirty_two_streams(i, J, route):
    gradient_checks(i, J, route)


@pytest.mark.parametrize('route', ['auto', 'generic', 'dedup'])
@pytest.mark.parametrize('i', fc.WIDE, ids=[fc.IDS[k] for k in fc.WIDE])
def test_masked_amplitudes(i, route):
    """Mask [1, 0, 1, 0, 0]: the unmasked gradients read 0 (gradient_checks), the unmasked amplitudes take part in gcoef at their
    initial values and keep their bits through two steps."""
    gradient_checks(i, 5, route, mask=fc.MASK5)
    amp = fc.basis(i, 5)[1]
    eng = make_engine(i, route, 5)
    try:
        eng.set_field_learn(fc.MASK5, amp, lr=0.05)
        eng.train_epoch([0, 0])
        torch.cuda.synchronize()
        got = eng.get_field_amps()
        on = np.array(fc.MASK5, dtype=bool)
        assert np.array_equal(got[~on], amp[~on]) and np.all(got[on] != amp[on]), (got, amp)
    finally:
        eng.close()


def test_routes_taken():
    """The automatic route of the cases with integ_num > 128 is the two-pass route; GENERIC is the generic kernels."""
    for i in (2, 4):
        eng = make_engine(i)
        try:
            assert eng.kernel_path()[1] == 1, fc.IDS[i]
        finally:
            eng.close()
    eng = make_engine(0, route='generic')
    try:
        assert eng.kernel_path()[0] == VN_KERNEL_GENERIC
    finally:
        eng.close()


def test_single_launch_route_takes_the_two_pass_sequence():
    """A batch without any polynomial term runs the single-launch 8-wave kernel; with a basis and learning on it takes the two-pass
    sequence (udbar exists there only) and the amplitude gradient is the reference's of that problem (D = 1)."""
    i, J = 0, 3
    d_in, dim, widths, q, n_k, U, nB, bDof, _, integW, td, act = fc.case(i)[:12]
    d = fc.inputs(i)
    G, amp = fc.basis(i, J)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=True, integWflag=integW, activationFun=act)
    try:
        eng.set_params(fc.theta(i))
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        eng.set_bic(d['biInput'], d['biLabel'], bDof, BIDIMVAL)
        eng.set_weights(d['w'])
        eng.set_interior(0, d['Input'], d['gcoef'], fc.s0_of(i), n_k=n_k, detJ=DETJ)
        eng.set_field_basis(0, G)
        assert eng.kernel_path()[1] == 0
        g_off = grad_of(eng)
        eng.set_field_learn([1] * J, np.zeros(J), lr=0.01)
        g_zero = grad_of(eng)                                      # another kernel sequence than the single launch: not its bits
        assert np.allclose(g_zero, g_off, rtol=1e-3, atol=1e-3 * np.max(np.abs(g_off)))
        eng.set_field_learn([1] * J, amp, lr=0.01)
        grad_of(eng)
        gb = eng.get_field_amps(grad=True)[1]
        from tests import field_ref
        from tests.inverse_ref import OFF
        _, _, g64, S = field_ref.evaluate(fc.theta(i), d_in, widths, d['gcoef'], G, amp, np.array(OFF), **fc.ref_kw(i))
        assert np.all(g64 != 0.0)
        check_amp_grad('%s/J%d/no_terms_fused8_to_twopass/amp' % (fc.IDS[i], J), gb, g64, S)
        eng.set_field_learn(None)
        assert np.array_equal(grad_of(eng), g_off)
    finally:
        eng.close()


@pytest.mark.parametrize('route', ['auto', 'dedup'])
@pytest.mark.parametrize('name', ['D', 'degenerate'])
def test_with_a_solution_dependent_diffusivity(name, route):
    """D = (0.7, 0.4, 0.3) and the degenerate D = (0, 0, 1) on both formulations: the seed the reduction reads carries D(u)."""
    i, J = 1, 3
    dc = DIFF if name == 'D' else DEGENERATE
    G, amp = fc.basis(i, J)
    eng = make_engine(i, route, J, dcoef=dc)
    try:
        eng.set_field_learn([1] * J, amp, lr=0.01)
        grad_of(eng)
        gb = eng.get_field_amps(grad=True)[1]
        _, _, g64, S = fc.evaluate(i, J, nldiff_coef=dc)
        _, _, g64_one, _ = fc.evaluate(i, J, nldiff_coef=(1.0, 0.0, 0.0))
        bar = check_amp_grad('%s/J%d/%s/nldiff_%s/amp' % (fc.IDS[i], J, route, name), gb, g64, S)
        assert np.all(np.abs(g64 - g64_one) >= 100 * bar)          # (a condition on the inputs) D(u) counts in every component
    finally:
        eng.close()


def test_next_to_the_other_learnt_vectors():
    """vn_set_coef_learn, vn_set_source_learn and vn_set_field_learn on together: each of the three gradients is bitwise what it is
    alone at the same mixed streams; one step moves all three vectors on the one step counter."""
    i, J = 0, 3
    G, amp = fc.basis(i, J)
    Phi, samp = sc.basis(i, J)
    c0 = fc.coefs_of(i)
    smix, gmix = source_fma_mix(i, J, samp), fc.fma_mix(i, J, amp)
    for route in ('auto', 'dedup'):
        def engine(field, source):
            eng = make_engine(i, route, J, gcoef=None if field else gmix, source=None if source else smix, basis=field)
            if source:
                eng.set_source_basis(0, Phi)
            return eng
        alone = {}
        eng = engine(True, False)
        try:
            eng.set_field_learn([1] * J, amp, lr=0.01)
            grad_of(eng)
            alone['field'] = eng.get_field_amps(grad=True)[1]
        finally:
            eng.close()
        eng = engine(False, True)
        try:
            eng.set_source_learn([1] * J, samp, lr=0.01)
            grad_of(eng)
            alone['source'] = eng.get_source_amps(grad=True)[1]
        finally:
            eng.close()
        eng = engine(False, False)
        try:
            eng.set_coef_learn([1] * 9, c0, lr=0.01)
            grad_of(eng)
            alone['coef'] = eng.get_coefs(grad=True)[1]
        finally:
            eng.close()
        eng = engine(True, True)
        try:
            eng.set_coef_learn([1] * 9, c0, lr=0.01)
            eng.set_source_learn([1] * J, samp, lr=0.01)
            eng.set_field_learn([1] * J, amp, lr=0.01)
            grad_of(eng)
            gc, gs, gf = eng.get_coefs(grad=True)[1], eng.get_source_amps(grad=True)[1], eng.get_field_amps(grad=True)[1]
            assert np.array_equal(gc, alone['coef']), (route, gc, alone['coef'])
            assert np.array_equal(gs, alone['source']), (route, gs, alone['source'])
            assert np.array_equal(gf, alone['field']), (route, gf, alone['field'])
            assert np.all(gf != 0.0) and np.all(gs != 0.0)
            eng.train_step(0)
            torch.cuda.synchronize()
            assert eng.step == 1
            assert np.all(eng.get_coefs() != c0.astype(np.float32).astype(np.float64))
            assert np.all(eng.get_source_amps() != samp) and np.all(eng.get_field_amps() != amp)
        finally:
            eng.close()


def test_next_to_flux_rows_periodic_pairs_and_observations():
    """The boundary passes do not read gcoef: with all three registered the amplitude gradient is what it was."""
    i, J = 0, 3
    d_in, dim = fc.case(i)[0], fc.case(i)[1]
    rng = np.random.default_rng(31)
    _, _, g64, S = fc.reference64(i, J)
    for route in ('auto', 'dedup'):
        eng = make_engine(i, route, J)
        try:
            eng.set_field_learn([1] * J, fc.basis(i, J)[1], lr=0.01)
            grad_of(eng)
            before = eng.get_field_amps(grad=True)[1]
            nrm = rng.standard_normal((17, dim)).astype(np.float32)
            eng.set_flux_bc(rng.uniform(-1, 1, (17, d_in)).astype(np.float32), nrm, rng.uniform(0, 1, 17).astype(np.float32),
                            rng.standard_normal(17).astype(np.float32), BIDIMVAL)
            eng.set_periodic(rng.uniform(-1, 1, (22, d_in)).astype(np.float32), rng.standard_normal((22, dim)).astype(np.float32), 1.0,
                             BIDIMVAL)
            eng.set_observations(rng.uniform(-1, 1, (33, d_in)).astype(np.float32), rng.standard_normal(33).astype(np.float32), weight=2.0)
            grad_of(eng)
            gb = eng.get_field_amps(grad=True)[1]
            check_amp_grad('%s/J%d/%s/edge_passes' % (fc.IDS[i], J, route), gb, g64, S)
            assert np.array_equal(gb, before)
        finally:
            eng.close()


# ---- 2. the step ----------------------------------------------------------------------------------------------------------
STEP_LR = 0.1     # 1e-6 of lr = 1e-7: above the half-ulp of an fp32 amplitude of magnitude <= 2 (1.2e-7 / 2) plus the fp32 step arithmetic


@pytest.mark.parametrize('route', ['auto', 'dedup'])
@pytest.mark.parametrize('i', fc.WIDE, ids=[fc.IDS[k] for k in fc.WIDE])
def test_train_step_is_adam_on_the_masked_amplitudes(i, route):
    """One vn_train_step from zero slots moves each masked amplitude as Adam in fp64 says (the engine's beta1, beta2, eps and lr_t
    as the kernel receives them, in fp32; step 1), within 1e-6 of lr; unmasked ones keep their bits; a bound that is hit is held
    exactly; grad + apply takes the same step."""
    J = 5
    mask = [1, 1, 0, 1, 1]
    amp = fc.basis(i, J)[1]
    lo, hi = np.full(J, -np.inf), np.full(J, np.inf)
    lo[3], hi[3] = amp[3] - 0.004, amp[3] + 0.004                       # the first Adam step is lr in size: b_3 hits one of them
    eng = make_engine(i, route, J)
    try:
        eng.set_field_learn(mask, amp, lo, hi, lr=STEP_LR)
        grad_of(eng)
        gb = eng.get_field_amps(grad=True)[1]
        eng.train_step(0)
        torch.cuda.synchronize()
        got, gb2 = eng.get_field_amps(grad=True)
        assert np.array_equal(gb, gb2) and eng.step == 1
        b1, b2, eps = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8))
        gi = gb.astype(np.float32).astype(np.float64)
        lr_t = float(np.float32(STEP_LR * np.sqrt(1 - 0.999) / (1 - 0.9)))
        want = amp - lr_t * ((1 - b1) * gi) / (np.sqrt((1 - b2) * gi * gi) + eps)
        for j in range(J):
            print('step %s/%s b%d: %.9g -> %.9g (Adam %.9g)' % (fc.IDS[i], route, j, amp[j], got[j], want[j]))
            if not mask[j]:
                assert got[j] == amp[j]
            elif j == 3:
                bound = lo[3] if gi[3] > 0 else hi[3]
                assert got[j] == float(np.float32(bound))
            else:
                assert gi[j] != 0.0 and abs(got[j] - want[j]) <= 1e-6 * STEP_LR, (j, got[j], want[j])
        eng.set_field_learn(mask, amp, lo, hi, lr=STEP_LR)
        eng.set_params(fc.theta(i))
        eng.grad(0)
        eng.apply()
        torch.cuda.synchronize()
        # (the step counter went on: lr_t of step 2 with fresh slots differs, so compare against the formula, not the bits)
        t = 2.0
        lr2 = float(np.float32(STEP_LR * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)))
        got2 = eng.get_field_amps()
        want2 = amp - lr2 * ((1 - b1) * gi) / (np.sqrt((1 - b2) * gi * gi) + eps)
        for j in (0, 1, 4):
            assert abs(got2[j] - want2[j]) <= 1e-6 * STEP_LR, (j, got2[j], want2[j])
    finally:
        eng.close()


def _state(eng):
    torch.cuda.synchronize()
    return np.asarray(eng.export_state()).copy(), eng.get_field_amps()


@pytest.mark.parametrize('route', ['auto', 'dedup'])
def test_train_epoch_snapshot_and_rollback(route):
    """vn_train_epoch over [0, 0, 0, 0] is bitwise four single steps, parameters, slots and amplitudes; snapshot -> three steps ->
    rollback restores amplitudes, their slots and the step counter bitwise (the replayed steps end in the same bits);
    vn_set_field_amps invalidates the snapshot."""
    i, J = 6, 3
    amp = fc.basis(i, J)[1]
    a, b = make_engine(i, route, J, lr=0.01), make_engine(i, route, J, lr=0.01)
    try:
        for e in (a, b):
            e.set_field_learn([1] * J, amp, lr=0.02)
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
        a.set_field_amps(amp)
        with pytest.raises(VNError, match='error 3: no snapshot to roll back to'):
            a.state_rollback()
    finally:
        a.close()
        b.close()


# ---- 3. gcoef is per step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['auto', 'generic', 'dedup'])
def test_gcoef_follows_the_device_amplitudes(route):
    """After vn_set_field_amps(b') vn_eval_loss, vn_grad and vn_objective_f64 equal those of an engine registered with the
    pre-mixed gcoef: the fp32 results bitwise (the same kernels read the same bits; case 1 has a non-periodic g0, so the
    de-duplicated step of both reads a CSR-ordered copy), the fp64 objective at the bars of tests/test_obj64_gpu.py (loss pieces
    1e-12, gradient 1e-11 of its maximum).  Then one training step: the next evaluation reads the moved amplitudes."""
    i, J = 1, 3
    amp = fc.basis(i, J)[1]
    b1 = (amp * np.array([1.5, -0.5, 2.0])).astype(np.float32).astype(np.float64)
    a, b = make_engine(i, route, J), make_engine(i, route, J, gcoef=fc.fma_mix(i, J, b1), basis=False)
    try:
        a.set_field_learn([1] * J, amp, lr=0.01)
        out0 = a.objective64(0)[0]
        l_first = loss_field(a)[0]
        a.set_field_amps(b1)
        assert np.array_equal(a.get_field_amps(), b1)
        la, lva = loss_field(a)
        lb, lvb = loss_field(b)
        assert np.array_equal(la, lb) and np.array_equal(lva, lvb)
        assert not np.array_equal(la, l_first)
        assert np.array_equal(grad_of(a), grad_of(b))
        out_a, g_a = a.objective64(0)[:2]
        out_b, g_b = b.objective64(0)[:2]
        g_a, g_b = g_a.cpu().numpy(), g_b.cpu().numpy()
        assert not np.allclose(out0[0], out_a[0], rtol=1e-6)               # the amplitudes count
        for k in range(4):
            assert abs(out_a[k] - out_b[k]) <= 1e-12 * abs(out_b[k]), (k, out_a[k], out_b[k])
        assert np.max(np.abs(g_a - g_b)) <= 1e-11 * np.max(np.abs(g_b))
        # a step moves the amplitudes, and the evaluation after it is that of the gcoef mixed at the moved ones
        a.set_field_learn([1] * J, b1, lr=0.05)
        a.train_step(0)
        torch.cuda.synchronize()
        b2 = a.get_field_amps()
        assert np.all(b2 != b1)
        c = make_engine(i, route, J, gcoef=fc.fma_mix(i, J, b2), basis=False)
        try:
            c.set_params(a.get_params())
            lc, lvc = loss_field(c)
            la2, lva2 = loss_field(a)
            assert np.array_equal(la2, lc) and np.array_equal(lva2, lvc)
        finally:
            c.close()
    finally:
        a.close()
        b.close()


def test_periodic_table_batch_with_learning_on_and_off():
    """A batch whose g0 repeats with period integ_num (the de-duplicated step reads it as a table): with learning on the step reads
    the mixed direction instead (the reference's numbers, test_amplitude_gradient), in either order of vn_set_dedup and
    vn_set_field_basis the same bits; mask = NULL gives back the table's bits."""
    i, J = 2, 3
    assert sc.base(i) in PERIODIC
    amp = fc.basis(i, J)[1]
    a, b = make_engine(i, 'dedup', J), make_engine(i, 'dedup', J, dedup_first=True)
    try:
        g_off = grad_of(a)
        assert np.array_equal(grad_of(b), g_off)
        res = []
        for e in (a, b):
            e.set_field_learn([1] * J, amp, lr=0.01)
            g = grad_of(e)
            res.append((g, e.get_field_amps(grad=True)[1]))
            e.set_field_learn(None)
            assert np.array_equal(grad_of(e), g_off)
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        assert not np.array_equal(res[0][0], g_off)
    finally:
        a.close()
        b.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals():
    i, J = 6, 3
    G, amp = fc.basis(i, J)
    n_k = fc.case(i)[4]
    nT, dim = G.shape[1], G.shape[2]
    ones = [1] * J
    for opt, word in (('rmsprop', 'an RMSProp'), ('lbfgs', 'an L-BFGS')):
        eng = make_engine(i, optimizer=opt)
        try:
            with pytest.raises(VNError, match='error 5: vn_set_field_learn on %s engine' % word):
                eng.set_field_learn(ones, amp, lr=0.01)
        finally:
            eng.close()
    eng = make_engine(i)
    try:
        bad = amp.copy()
        bad[1] = np.nan
        with pytest.raises(VNError, match='error 1: initial amplitude 1'):
            eng.set_field_learn(ones, bad, lr=0.01)
        lo, hi = np.full(J, -np.inf), np.full(J, np.inf)
        lo[2], hi[2] = 1.0, 0.5
        with pytest.raises(VNError, match='error 1: bounds of amplitude 2'):
            eng.set_field_learn(ones, amp, lo, hi, lr=0.01)
        for lr in (0.0, -1.0, float('nan')):
            with pytest.raises(VNError, match='error 1: amplitude learning rate'):
                eng.set_field_learn(ones, amp, lr=lr)
        with pytest.raises(VNError, match='error 1: 1 to 32 field amplitudes can be learnt, got 33'):
            eng.set_field_learn([1] * 33, np.zeros(33), lr=0.01)
        with pytest.raises(VNError, match='error 3: no learnt field amplitudes'):
            eng.set_field_amps(amp)
        with pytest.raises(VNError, match='error 1: a field basis has 1 to 32 streams, got 33'):
            eng.set_field_basis(0, np.zeros((33, nT, dim), dtype=np.float32))
        # (a failed call leaves the batch without a basis: learning on, the step runs with nothing to reduce)
        eng.set_field_learn(ones, amp, lr=0.01)
        grad_of(eng)
        assert np.all(eng.get_field_amps(grad=True)[1] == 0.0)
        # a basis of another J than the learnt vector's
        eng.set_field_basis(0, fc.basis(i, 5)[0])
        with pytest.raises(VNError, match='error 1: batch 0 has a field basis of 5 streams, the learnt amplitudes .* are 3'):
            eng.grad(0)
        with pytest.raises(VNError, match='error 1: batch 0 has a field basis of 5 streams'):
            eng.eval_loss(0)
        with pytest.raises(VNError, match='error 1: batch 0 has a field basis of 5 streams'):
            eng.objective64(0)
        eng.set_field_basis(0, G)
        with pytest.raises(VNError, match='error 1: the engine holds 3 field amplitudes'):
            eng.get_field_amps(J=5)
        with pytest.raises(VNError, match='error 1: the engine holds 3 field amplitudes'):
            eng.set_field_amps(np.zeros(5))
        with pytest.raises(VNError, match='error 1: amplitude 0'):
            eng.set_field_amps([np.inf, 0.0, 0.0])
        # per-test-function weights and learning, in either order
        with pytest.raises(VNError, match='error 5: learnt field amplitudes .* next to per-test-function loss weights'):
            eng.set_tf_weights(0, np.ones(n_k, dtype=np.float32))
        eng.set_field_learn(None)
        eng.set_tf_weights(0, np.ones(n_k, dtype=np.float32))
        with pytest.raises(VNError, match=r'error 5: learnt field amplitudes \(vn_set_field_learn\) next to per-test-function loss weights'):
            eng.set_field_learn(ones, amp, lr=0.01)
        eng.set_tf_weights(0, None)
        eng.set_field_learn(ones, amp, lr=0.01)
        with pytest.raises(VNError, match='error 5: vn_comm_init while field amplitudes are learnt'):
            eng.comm_init(0, 1, bytes(VN_COMM_ID_BYTES))
        # vn_set_interior clears the basis of its batch
        d = fc.inputs(i)
        eng.set_interior(0, d['Input'], d['gcoef'], fc.s0_of(i), n_k=n_k, detJ=DETJ)
        grad_of(eng)
        assert np.all(eng.get_field_amps(grad=True)[1] == 0.0)
    finally:
        eng.close()
    # the layer-by-layer route has no point pass for the rows' grad u
    eng = make_engine(i, 'layered', basis=False)
    try:
        assert eng.kernel_path()[0] == VN_KERNEL_LAYERED
        with pytest.raises(VNError, match='error 5: learnt field amplitudes are not built for the layer-by-layer route'):
            eng.set_field_learn(ones, amp, lr=0.01)
    finally:
        eng.close()
    # the 4-wave cross-check geometry leaves no row seeds
    d_in, dim, widths, q, n_k, U, nB, bDof, source, integW, td, act = CASES[0][:12]
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW, activationFun=act, kernel=VN_KERNEL_FUSED)
    try:
        with pytest.raises(VNError, match='error 5: learnt field amplitudes are not built for VN_KERNEL_FUSED'):
            eng.set_field_learn(ones, amp, lr=0.01)
    finally:
        eng.close()
    # more than three space dimensions: the point pass carries three gradient components
    eng = VNEngine(4, 5, [20, 20], True, 16)
    try:
        with pytest.raises(VNError, match='error 5: learnt field amplitudes need dim <= 3, got 4'):
            eng.set_field_learn(ones, amp, lr=0.01)
    finally:
        eng.close()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
KAPPA_STAR, V_STAR, T_END = 0.1, 0.5, 0.5
KAPPA_GUESS, V_GUESS = 0.3, 0.0
B_STAR = np.array([KAPPA_STAR - KAPPA_GUESS, V_STAR - V_GUESS])
EPOCHS = 650       # the smallest probed count (steps of 50) that ends within 0.8 of the bar: see test_recovers_diffusivity_and_velocity
FIELD_LR = 0.01    # the network's rate, which is also the default


def u_star(x, t):
    """The solution of u_t + v u_x = kappa u_xx with kappa* = 0.1, v* = 0.5 that starts as sin(pi x)."""
    return np.exp(-KAPPA_STAR * pi * pi * t) * np.sin(pi * (x - V_STAR * t))


def sensors(seed=0):
    rng = np.random.default_rng(seed)
    x, t = rng.uniform(0, 1, 64), rng.uniform(0, T_END, 64)
    return np.column_stack([x, t]), u_star(x, t)


def problem():
    edge = [0.0, 1.0, lambda x, t: u_star(x, t)]
    return ADPDE(Domain1D(np.array([0.0, 1.0])), diff=KAPPA_GUESS, vel=V_GUESS, tInterval=[0, T_END], BCs=[list(edge), list(edge)],
                 IC=lambda x: np.sin(pi * x), cEx=u_star, diffBasis=[1], velBasis=[1])


LEARN = dict(learnField={'diff': True, 'vel': True}, fieldBounds={'diff': (0.01 - KAPPA_GUESS, None)})      # kappa >= 0.01


def _train(folder, epochs=None, **vn_kw):
    epochs = EPOCHS if epochs is None else epochs
    np.random.seed(0)
    vn = VarNet(problem(), layerWidth=[20], activationFun='tanh', discNum=40, bDiscNum=None, tDiscNum=20, learning_rate=0.01,
                observations=sensors(), **vn_kw)
    vn.train(str(folder), weight=[10.0, 10.0, 1.0], epochNum=epochs, tol=0.0, saveFreq=epochs, verbose=False)
    amps = vn.fieldAmplitudes()
    out = np.concatenate([amps['diff'], amps['vel']]), vn.obsMisfit(), vn.residual()[2]
    text = open(os.path.join(str(folder), 'caseData.txt')).read()
    vn.engine.close()
    return out + (text,)


def test_recovers_diffusivity_and_velocity(tmp_path):
    """u_t + v u_x = kappa u_xx on [0, 1] x [0, 0.5] with u = exp(-kappa pi^2 t) sin(pi (x - v t)), truth kappa* = 0.1, v* = 0.5;
    the PDE is given kappa = 0.3 + b_1, v = 0 + b_2, so b* = (-0.2, 0.5), guess b = 0; Dirichlet ends and the initial condition from
    u, 64 point sensors.  Required: ||b - b*|| <= ||b*|| / 3 = 0.1795, and the misfit ends below that of the twin trained with the
    amplitudes frozen at the guess (same seed, same epochs).  Measured on one MI355X (seed fixed, fieldLr 0.01), ||b - b*|| is
    0.187 after 500 epochs, 0.150 after 600, 0.134 after 650 (b = (-0.265, 0.383); misfit 1.36e-2, twin 2.79e-2), 0.118 after 700,
    0.088 after 800, 0.052 after 1 000, 0.017 after 2 000, 0.016 after 3 000 and 0.019 after 10 000 (b = (-0.205, 0.518)); fieldLr
    of 0.003 and 0.03 give 0.061 and 0.052 after 1 000.  650 is the smallest probed count that ends within 0.8 of the bar (0.1436);
    the two trainings take under a second."""
    b, misfit, err, text = _train(tmp_path / 'learn', fieldLr=FIELD_LR, **LEARN)
    b_twin, misfit_twin, err_twin, _ = _train(tmp_path / 'twin')
    dist, dist0 = float(np.linalg.norm(b - B_STAR)), float(np.linalg.norm(B_STAR))
    RECORD['end_to_end/field_amplitudes'] = {'b': [float(x) for x in b], 'distance': dist, 'distance_guess': dist0, 'misfit': misfit,
                                             'misfit_twin': misfit_twin, 'l2_error': float(err), 'l2_error_twin': float(err_twin),
                                             'epochs': EPOCHS, 'fieldLr': FIELD_LR}
    print('field amplitudes: b %s (truth %s); |b - b*| %.4f of %.4f; misfit %.4e, frozen twin %.4e; l2 error %.4f, twin %.4f'
          % (b, B_STAR, dist, dist0, misfit, misfit_twin, err, err_twin))
    assert np.array_equal(b_twin, np.zeros(2))
    assert 'Learnt field amplitudes (diff, then vel): mask [1, 1], initial [0.0, 0.0], final' in text
    assert dist <= dist0 / 3.0
    assert misfit < misfit_twin


def test_loss_lag_blocks_end_in_the_same_amplitudes(tmp_path):
    """train(lossLag=8) ends in the amplitudes (and the epoch) of lossLag=1 when the tolerance is met inside a block: the rollback
    carries the amplitude state."""
    def run(folder, lag, tol, epochs):
        np.random.seed(0)
        vn = VarNet(problem(), layerWidth=[20], activationFun='tanh', discNum=40, bDiscNum=None, tDiscNum=20, learning_rate=0.01,
                    observations=sensors(), fieldLr=FIELD_LR, **LEARN)
        res = vn.train(str(folder), weight=[10.0, 10.0, 1.0], epochNum=epochs, tol=tol, saveFreq=1, verbose=False, lossLag=lag)
        amps = vn.fieldAmplitudes()
        out = np.concatenate([amps['diff'], amps['vel']]), vn.engine.step, vn.engine.get_params(), list(res.loss)
        vn.engine.close()
        return out

    _, _, _, losses = run(tmp_path / 'probe', 1, 0.0, 30)
    tol = float(losses[20]) * (1.0 + 1e-9)
    b_1, step_1, th_1, _ = run(tmp_path / 'lag1', 1, tol, 60)
    b_8, step_8, th_8, _ = run(tmp_path / 'lag8', 8, tol, 60)
    print('lossLag: stopped after %d / %d steps, b %s / %s' % (step_1, step_8, b_1, b_8))
    assert 1 < step_1 < 60 and step_1 == step_8
    assert np.array_equal(b_1, b_8) and np.all(b_1 != 0.0) and np.array_equal(th_1, th_8)
