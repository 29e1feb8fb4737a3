"""
GPU tier of the polynomial reaction term (vn_set_reaction, `ADPDE(reaction=(rate, [c1, c2, c3]))`):

    c_t = div(kappa grad c) - v . grad c + s + rate p(c),      p(c) = c1 c + c2 c^2 + c3 c^3.

Parity of the loss components, the loss field and the gradient against the fp64 restatement (tests/reaction_ref.py) on every
route (generic, single-launch 8-wave -> two-pass sequence, two-pass, layer by layer, de-duplicated), the fp64 objective at the
bars of tests/test_obj64_gpu.py, the composition of the step's entry points, the registration contract, the strong residual, and
two small training problems judged against a twin run whose reaction is folded into the source through the exact solution.

Bars are the project's own (tests/parity_cases.py: LOSS_RTOL, GRAD_RTOL through tests/gradcheck.assert_grad_close with its fp32
conditioning callback, LVEC_RTOL).  Every parity test also asserts, in the reference, that removing the reaction moves varLoss and
the gradient norm by more than 1e-2 relative: the term is a real part of what is compared.

The worst errors per case and route and both twins' errors are written to reaction_parity.json in the directory VN_RECORD_DIR
names (default: profile_out/ beside tests/; the committed copy: profiles/reaction_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import flux_ref, reaction_ref
from tests.gradcheck import assert_grad_close, assert_pair_close, block_errors, fp32_deviation
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL
from tests.reaction_cases import CASES, COEF, IDS, inputs, reaction_of, reference, reference64, theta
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import (VN_KERNEL_AUTO, VN_KERNEL_FUSED, VN_KERNEL_FUSED16, VN_KERNEL_GENERIC, VN_KERNEL_LAYERED, VNEngine,
                               VNError)
from varnet_amd.utility import UF
from varnet_amd.varnet import VarNet

pytestmark = pytest.mark.gpu

uf = UF()
pi = np.pi
KEYS = ['loss', 'BCloss', 'ICloss', 'varLoss']
RECORD = {}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'reaction_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def make_engine(i, kernel=VN_KERNEL_AUTO, variant='rate', xcheck=False, optimizer='adam'):
    d_in, dim, widths, q, n_k, nB, bDof, td, act, source, integW, detJvec, rows = CASES[i]
    d, _ = inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW, kernel=kernel, activationFun=act, xcheck=xcheck,
                   optimizer_name=optimizer)
    eng.set_params(theta(i))
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    register_interior(eng, i)
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
    eng.set_weights(d['w'])
    if variant != 'none':
        eng.set_reaction(0, *reaction_of(i, variant))
    return eng


def register_interior(eng, i, batch=0):
    d = inputs(i)[0]
    eng.set_interior(batch, d['Input'], d['gcoef'], d['source'], n_k=CASES[i][4], detJ=d['detJ'], N_rows=d['N_rows'],
                     dNt_rows=d['dNt_rows'])


def grad_of(eng, batch=0):
    gb = eng.bind_grad_buffer()
    eng.grad(batch)
    torch.cuda.synchronize()
    return gb.cpu().numpy().astype(np.float64)


def term_is_real(i, variant):
    """In the reference: removing the reaction moves varLoss and the gradient norm by more than 1e-2 relative."""
    ref, g = reference64(i, variant)
    ref0, g0 = reference64(i, 'none')
    assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss']), (ref['varLoss'], ref0['varLoss'])
    assert np.linalg.norm(g - g0) > 1e-2 * np.linalg.norm(g)


def check_parity(i, eng, variant, tag, ref=None, g32=None):
    """eval_loss (with lossVec) and grad of batch 0 against the reference; prints and records every figure, then asserts."""
    d_in, dim, widths, td = CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][7]
    ref, gref = reference64(i, variant) if ref is None else ref
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
    print('reaction %s: %s' % (tag, json.dumps(rec, sort_keys=True)))
    for got, key in zip(out, KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'eval', key, got, ref[key])
    for got, key in zip(g[P:], KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'grad', key, got, ref[key])
    assert rec['lossVec'] <= LVEC_RTOL, (tag, rec['lossVec'])
    if g32 is None:
        g32 = lambda: reference(i, reaction_of(i, variant), dtype=torch.float32)[1]
    assert_grad_close(g[:P], gref, d_in, widths, GRAD_RTOL, dim=dim, td=td, what=tag, g32=g32)
    return g


# ---- parity on every route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_parity(i, kernel):
    term_is_real(i, 'rate')
    if max(CASES[i][2]) > 64 and kernel == VN_KERNEL_GENERIC:
        # the 128-wide case lies outside the generic kernels: the engine refuses the request (as it does without a reaction)
        with pytest.raises(VNError, match='error 5'):
            make_engine(i, kernel)
        return
    eng = make_engine(i, kernel)
    try:
        check_parity(i, eng, 'rate', '%s/%s' % (IDS[i], 'auto' if kernel == VN_KERNEL_AUTO else 'generic'))
    finally:
        eng.close()


@pytest.mark.parametrize('variant', ['unit', 'linear'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_parity_unit_rate_and_linear_term(i, variant):
    """rate=None (rate = 1) with the cubic, and coef = (lambda, 0, 0) with the rate stream, on the automatic route."""
    term_is_real(i, variant)
    eng = make_engine(i, variant=variant)
    try:
        check_parity(i, eng, variant, '%s/auto/%s' % (IDS[i], variant))
    finally:
        eng.close()


def test_routes_of_the_cases():
    """What the parity cases run on: integ_num 4, 16 and 64 on the single-launch 8-wave route (whose batches with a reaction
    take the two-pass sequence), 216 on the two-pass route, 128 wide layer by layer."""
    want = {0: (VN_KERNEL_FUSED16, 0), 1: (VN_KERNEL_FUSED16, 0), 3: (VN_KERNEL_FUSED16, 0), 4: (VN_KERNEL_FUSED16, 1),
            5: (VN_KERNEL_LAYERED, 0)}
    for i, kp in want.items():
        eng = make_engine(i, variant='none')
        try:
            assert tuple(eng.kernel_path()) == kp, (IDS[i], eng.kernel_path())
        finally:
            eng.close()


# ---- de-duplicated step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['rate', 'unit'])
def test_dedup_identity_map(variant):
    """Identity point map on the bench network: against the reference, against the row-wise gradient of the same engine, and
    two calls give the same bits."""
    i = 3
    term_is_real(i, variant)
    d_in, dim, widths = CASES[i][0], CASES[i][1], CASES[i][2]
    eng = make_engine(i, variant=variant)
    try:
        g_row = grad_of(eng)
        nT = inputs(i)[0]['Input'].shape[0]
        idx = torch.arange(nT, dtype=torch.int32)
        eng.set_dedup(0, inputs(i)[0]['Input'], idx, torch.arange(nT + 1, dtype=torch.int32), idx)
        g1 = check_parity(i, eng, variant, '%s/dedup_identity/%s' % (IDS[i], variant))
        g2 = grad_of(eng)
        assert np.array_equal(g1, g2)
        assert not np.array_equal(g1, g_row)                       # another formulation ran
        dev32 = lambda: fp32_deviation(reference(i, reaction_of(i, variant), dtype=torch.float32)[1], reference64(i, variant)[1],
                                       d_in, widths, dim)
        RECORD['%s/dedup_identity/%s/vs_rowwise' % (IDS[i], variant)] = assert_pair_close(
            g1, g_row, d_in, widths, GRAD_RTOL, dim=dim, dev32=dev32, what='dedup vs row-wise')
        # row-wise eval_loss of the same batch (debug route 8) agrees with the de-duplicated one
        out_dd, _ = eng.eval_loss(0)
        eng.debug_point_route(8)
        out_rw, _ = eng.eval_loss(0)
        eng.debug_point_route(0)
        for a, b in zip(out_dd, out_rw):
            assert abs(a - b) <= LOSS_RTOL * abs(b) + 1e-7
    finally:
        eng.close()


def rate_fun(x, t=0):
    return 1.0 + 0.5 * x ** 2 + t


def _varnet_reference(vn, td, reaction, dtype=torch.float64):
    fd, d = vn.fixData, td.mor[0]
    f = np.float64 if dtype == torch.float64 else np.float32
    Nr, dNxr, dNtr = fd.rows()                                   # (rounded to fp32 below: the engine's tables are fp32)
    cpu = lambda t: t.cpu().numpy().astype(f)
    kw = dict(Input=cpu(d['Input']), gcoef=cpu(d['gcoef']), source=None if d['source'] is None else cpu(d['source']).reshape(-1, 1),
              N=Nr.astype(np.float32).astype(f), dNt=dNtr.astype(np.float32).astype(f), integW=None, intShape=[fd.nt, fd.integNum], detJ=float(fd.detJ), detJvec=False,
              biInput=cpu(d['biInput']), biLabel=cpu(d['biLabel']).reshape(-1, 1), bDof=fd.bDofsum, biDimVal=float(fd.biDimVal),
              w=np.ones(3), dim=vn.dim, time_dependent=True, is_source=vn.lossOpt['isSource'], integWflag=False)
    if reaction is not None and reaction[0] is not None:
        reaction = (np.asarray(reaction[0]).astype(f), reaction[1])
    return reaction_ref.loss_and_grad(vn.engine.get_params().astype(f), vn.inpDim, vn.layerWidth, reaction, dtype, **kw)


def test_dedup_shared_points_through_varnet():
    """A real shared-point map on a uniform 1D+t grid, built by VarNet: the rate stream is uploaded per row, enable_dedup keeps
    the registration, and the de-duplicated gradient agrees with the reference and with the row-wise one."""
    pde = ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, vel=0.5, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x),
                reaction=(rate_fun, list(COEF)))
    vn = VarNet(pde, layerWidth=[20, 20], discNum=12, bDiscNum=None, tDiscNum=10)
    eng = vn.engine
    try:
        eng.set_params(eng.get_params() + 0.05 * np.random.default_rng(5).standard_normal(eng.P).astype(np.float32))
        td = vn._build_tdata()
        td.select_mor(0)
        eng.set_weights([1.0, 1.0, 1.0])
        rate = td.mor[0]['rate'].cpu().numpy().reshape(-1, 1)
        X = td.mor[0]['Input_host']
        np.testing.assert_allclose(rate, rate_fun(X[:, 0:1], X[:, 1:2]), rtol=1e-6)
        ref, gref = _varnet_reference(vn, td, (rate, COEF))
        ref0, g0 = _varnet_reference(vn, td, None)
        assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss'])
        assert np.linalg.norm(gref - g0) > 1e-2 * np.linalg.norm(gref)
        g32 = lambda: _varnet_reference(vn, td, (rate, COEF), torch.float32)[1]
        g_row = grad_of(eng)
        P = eng.P
        assert abs(g_row[P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7
        rec = {}
        assert_grad_close(g_row[:P], gref, vn.inpDim, vn.layerWidth, GRAD_RTOL, dim=1, what='varnet row-wise', g32=g32, rec=rec)
        RECORD['varnet_1dt/rowwise'] = rec
        U = td.enable_dedup()
        assert td.dedup_reason is None and 0 < U < vn.fixData.nT / 2, (td.dedup_reason, U)
        g1 = grad_of(eng)
        g2 = grad_of(eng)
        assert np.array_equal(g1, g2) and not np.array_equal(g1, g_row)
        for k in range(4):
            assert abs(g1[P + k] - ref[KEYS[k]]) <= LOSS_RTOL * abs(ref[KEYS[k]]) + 1e-7, (KEYS[k], g1[P + k], ref[KEYS[k]])
        rec = {}
        assert_grad_close(g1[:P], gref, vn.inpDim, vn.layerWidth, GRAD_RTOL, dim=1, what='varnet dedup', g32=g32, rec=rec)
        RECORD['varnet_1dt/dedup'] = rec
        dev32 = lambda: fp32_deviation(g32(), gref, vn.inpDim, vn.layerWidth, 1)
        RECORD['varnet_1dt/dedup_vs_rowwise'] = assert_pair_close(g1, g_row, vn.inpDim, vn.layerWidth, GRAD_RTOL, dim=1,
                                                                    dev32=dev32, what='varnet dedup vs row-wise')
        out, lv = eng.eval_loss(0, lossVec=True)                     # the loss-only form of the de-duplicated assembly
        assert abs(out[3] - ref['varLoss']) <= LOSS_RTOL * abs(ref['varLoss']) + 1e-7
        lref = ref['lossVec'].reshape(-1)
        assert np.max(np.abs(lv.cpu().numpy() - lref)) <= LVEC_RTOL * np.max(np.abs(lref))
        # splitLoss (fp32 and fp64) and precisionReport see the term
        comp, _, _ = vn.splitLoss(td)
        assert abs(comp[2, 0] - ref['varLoss']) <= LOSS_RTOL * abs(ref['varLoss']) + 1e-7
        comp64, _, _ = vn.splitLoss(td, fp64=True)
        assert abs(comp64[2, 0] - ref['varLoss']) <= 1e-9 * abs(ref['varLoss'])
        rep = vn.precisionReport(td)
        assert rep['dedup'] and rep['loss']['varLoss'] <= LOSS_RTOL and rep['grad_global'] <= GRAD_RTOL, rep
    finally:
        eng.close()


# ---- fp64 objective -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['rate', 'unit'])
@pytest.mark.parametrize('i', [0, 1, 2, 3, 4, 6], ids=[IDS[k] for k in (0, 1, 2, 3, 4, 6)])
def test_objective64_parity(i, variant):
    """vn_objective_f64 against the reference at the bars of tests/test_obj64_gpu.py: loss components 1e-12, gradient blocks
    1e-11, lossVec 1e-11 of its maximum.  Parameters in fp64 (not fp32-representable)."""
    d_in, dim, widths, td = CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][7]
    th = theta(i).astype(np.float64) + 1e-3 * np.random.default_rng(6).standard_normal(theta(i).size)
    ref, gref = reference(i, reaction_of(i, variant), flat=th)
    ref0, g0 = reference(i, None, flat=th)
    assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss'])
    assert np.linalg.norm(gref - g0) > 1e-2 * np.linalg.norm(gref)
    eng = make_engine(i, variant=variant)
    try:
        out, g, lv = eng.objective64(0, theta=th, grad=True, lossVec=True)
        rec = {}
        for got, key in zip(out, KEYS):
            rec[key] = abs(got - ref[key]) / max(abs(ref[key]), 1e-300) if ref[key] != 0.0 else abs(got)
        lref = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1)
        rec['lossVec'] = float(np.max(np.abs(lv.cpu().numpy() - lref)) / np.max(np.abs(lref)))
        errs = block_errors(g.cpu().numpy(), gref, d_in, widths, dim, td)
        rec['worst_block'] = max(errs, key=errs.get)
        rec['worst_block_err'] = errs[rec['worst_block']]
        RECORD['%s/objective64/%s' % (IDS[i], variant)] = rec
        print('reaction objective64 %s %s: %s' % (IDS[i], variant, json.dumps(rec, sort_keys=True)))
        for key in KEYS:
            assert rec[key] <= 1e-12, (key, rec[key])
        assert rec['lossVec'] <= 1e-11, rec['lossVec']
        assert rec['worst_block_err'] <= 1e-11, (rec['worst_block'], rec['worst_block_err'])
        # loss-only form and a second call: same bits
        out2, _, _ = eng.objective64(0, theta=th, grad=False)
        assert out2 == out
    finally:
        eng.close()


def test_objective64_is_refused_beyond_the_kernels_with_or_without_the_term():
    eng = make_engine(5)
    try:
        with pytest.raises(VNError, match='error 5: vn_objective_f64 serves networks of the hand-written kernels'):
            eng.objective64(0)
    finally:
        eng.close()


# ---- composition ----------------------------------------------------------------------------------------------------
def _theta_after(eng, state, fn):
    eng.import_state(state)
    fn()
    torch.cuda.synchronize()
    return eng.get_params()


@pytest.mark.parametrize('i', [2, 3], ids=[IDS[2], IDS[3]])
def test_train_step_equals_grad_then_apply(i):
    """train_step folds the update into the gradient reduction; grad + apply runs it as its own kernel.  Their relation is
    measured first without a reaction, then required to hold with one (tests/test_flux_bc_gpu.py measures it the same way)."""
    eng = make_engine(i, variant='none')
    try:
        s0 = eng.export_state()
        flat = eng.get_params()
        gap = []
        for with_term in (False, True):
            if with_term:
                eng.set_reaction(0, *reaction_of(i, 'rate'))
            a = _theta_after(eng, s0, lambda: eng.train_step(0))
            b = _theta_after(eng, s0, lambda: (eng.grad(0), eng.apply()))
            assert np.max(np.abs(a - flat)) > 1e-4                       # the step moved theta
            gap.append(float(np.max(np.abs(a - b))))
        assert gap[1] <= max(2.0 * gap[0], 1e-6), gap
    finally:
        eng.close()


def test_train_epoch_over_two_batches_one_with_a_reaction():
    i = 3
    eng = make_engine(i)                                                # batch 0 carries the reaction
    plain = make_engine(i, variant='none')
    try:
        register_interior(eng, i, batch=1)                              # batch 1: the same rows, no reaction
        g1 = grad_of(eng, 1)
        assert np.array_equal(g1, grad_of(plain))                       # ... and bit for bit the step of an engine without any
        assert not np.array_equal(g1, grad_of(eng, 0))
        s0 = eng.export_state()
        acc = torch.zeros(1, device='cuda')
        a = _theta_after(eng, s0, lambda: eng.train_epoch((0, 1, 0), acc))
        losses = [torch.zeros(1, device='cuda') for _ in range(3)]
        b = _theta_after(eng, s0, lambda: [eng.train_step(k, l) for k, l in zip((0, 1, 0), losses)])
        assert np.array_equal(a, b)
        assert eng.step == 3
        total = sum(float(l.item()) for l in losses)
        assert abs(acc.item() - total) <= 1e-5 * abs(total)             # the epoch's loss sum: the three pre-update losses
    finally:
        eng.close()
        plain.close()


def test_lbfgs_step_decreases_the_reaction_objective():
    i = 2
    eng = make_engine(i, optimizer='lbfgs')
    try:
        ref = reference64(i, 'rate')[0]
        info = eng.lbfgs_step(0)
        assert abs(info['f_k'] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7        # the objective has the term
        assert info['status'] == 0 and info['f_next'] < info['f_k'], info
        out, _ = eng.eval_loss(0)
        assert abs(out[0] - info['f_next']) <= LOSS_RTOL * abs(out[0]) + 1e-7
        # a change of the registration invalidates (f_k, g_k): the next call evaluates the new objective first
        eng.set_reaction(0)
        out0, _ = eng.eval_loss(0)
        info = eng.lbfgs_step(0)
        assert abs(info['f_k'] - out0[0]) <= LOSS_RTOL * abs(out0[0]) + 1e-7 and info['pairs'] == 0, info
    finally:
        eng.close()


@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
def test_flux_rows_and_reaction_together(kernel):
    i = 2
    d_in, dim, widths = CASES[i][0], CASES[i][1], CASES[i][2]
    nF = 40
    rng = np.random.default_rng(14)
    nrm = rng.standard_normal((nF, dim))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    coef = rng.uniform(0.5, 2.0, nF)
    coef[:nF // 2] = 0.0
    fx = {k: np.asarray(v).astype(np.float32) for k, v in
          dict(X=rng.uniform(-1, 1, (nF, d_in)), normal=nrm, coef=coef, label=rng.standard_normal(nF)).items()}

    def ref_with_flux(dtype):
        f = np.float64 if dtype == torch.float64 else np.float32
        res, g = reference(i, reaction_of(i, 'rate'), dtype=dtype)
        w = inputs(i)[0]['w']
        F, gF, _ = flux_ref.flux_term(theta(i).astype(f), d_in, widths, dim, fx['X'].astype(f), fx['normal'].astype(f),
                                      fx['coef'].astype(f), fx['label'].astype(f), 2.0, CASES[i][8], dtype)
        res = dict(res)
        res['BCloss'] = res['BCloss'] + F
        res['loss'] = res['loss'] + w[0] * F
        return res, g + w[0] * gF

    term_is_real(i, 'rate')
    ref = ref_with_flux(torch.float64)
    assert abs(ref[0]['BCloss'] - reference64(i, 'rate')[0]['BCloss']) > 1e-2 * abs(ref[0]['BCloss'])
    eng = make_engine(i, kernel)
    try:
        eng.set_flux_bc(fx['X'], fx['normal'], fx['coef'], fx['label'], 2.0)
        check_parity(i, eng, 'rate', '%s/flux/%s' % (IDS[i], 'auto' if kernel == VN_KERNEL_AUTO else 'generic'), ref=ref,
                     g32=lambda: ref_with_flux(torch.float32)[1])
    finally:
        eng.close()


# ---- contract -------------------------------------------------------------------------------------------------------
def _snapshot(eng):
    out, lv = eng.eval_loss(0, lossVec=True)
    g = grad_of(eng).copy()
    for _ in range(3):
        eng.train_step(0)
    torch.cuda.synchronize()
    return np.array(out), lv.cpu().numpy(), g, eng.get_params()


@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('i', [2, 3], ids=[IDS[2], IDS[3]])
def test_register_then_clear_is_bitwise_untouched(i, kernel):
    runs = []
    for how in ('never', 'cleared', 'reregistered'):
        eng = make_engine(i, kernel, variant='none' if how == 'never' else 'rate')
        try:
            if how == 'cleared':
                eng.grad(0)                                             # a step with the term ...
                eng.set_reaction(0, None, (0.0, 0.0, 0.0))             # ... then cleared
            elif how == 'reregistered':
                eng.grad(0)
                register_interior(eng, i)                               # a new vn_set_interior clears the registration
            runs.append(_snapshot(eng))
        finally:
            eng.close()
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert np.array_equal(x, y)


def test_set_dedup_keeps_the_reaction_and_set_reaction_keeps_the_map():
    i = 3
    nT = inputs(i)[0]['Input'].shape[0]
    idx = torch.arange(nT, dtype=torch.int32)
    ptr = torch.arange(nT + 1, dtype=torch.int32)
    ref = reference64(i, 'rate')[0]
    grads = []
    for order in ('reaction_first', 'map_first'):
        eng = make_engine(i, variant='rate' if order == 'reaction_first' else 'none')
        try:
            g_row = grad_of(eng).copy() if order == 'reaction_first' else None
            eng.set_dedup(0, inputs(i)[0]['Input'], idx, ptr, idx)
            if order == 'map_first':
                eng.set_reaction(0, *reaction_of(i, 'rate'))
            g = grad_of(eng)
            assert abs(g[eng.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7      # the term is there
            if g_row is not None:
                assert not np.array_equal(g, g_row)                                       # ... and so is the map
            grads.append(g.copy())
        finally:
            eng.close()
    assert np.array_equal(grads[0], grads[1])


def test_refusals():
    i = 2
    rate = inputs(i)[1]
    eng = make_engine(i, VN_KERNEL_FUSED, variant='none')               # the 4-wave cross-check geometry
    try:
        with pytest.raises(VNError, match='error 5: the reaction term is not built for VN_KERNEL_FUSED'):
            eng.set_reaction(0, rate, COEF)
        eng.set_reaction(0)                                             # clearing is always accepted
    finally:
        eng.close()
    eng = make_engine(i, variant='none')
    try:
        with pytest.raises(VNError, match='error 1: reaction coefficients'):
            eng.set_reaction(0, rate, (1.0, float('nan'), 0.0))
        with pytest.raises(VNError, match='error 1: reaction coefficients'):
            eng.set_reaction(0, None, (float('inf'), 0.0, 0.0))
        with pytest.raises(VNError, match='error 3'):
            eng.set_reaction(5, None, COEF)                             # an unregistered batch
        d_in, dim = CASES[i][0], CASES[i][1]
        eng.set_interior(1, torch.zeros(0, d_in, device='cuda'), torch.zeros(0, dim, device='cuda'), None, n_k=0, detJ=0.1)
        with pytest.raises(VNError, match='error 1: batch 1 has no interior rows'):
            eng.set_reaction(1, None, COEF)
        with pytest.raises(ValueError, match='at most three coefficients'):
            eng.set_reaction(0, None, (1.0, 2.0, 3.0, 4.0))
        # none of the refused calls left a registration behind
        plain = make_engine(i, variant='none')
        try:
            assert np.array_equal(grad_of(eng), grad_of(plain))
        finally:
            plain.close()
    finally:
        eng.close()


# ---- strong residual ------------------------------------------------------------------------------------------------
def test_residual_with_the_term():
    """VNEngine.residual(..., reaction=...) in fp32 and fp64 against the reference, at the bars of
    tests/test_engine_gpu.py::test_forward_and_residual_parity (the same network class)."""
    d_in, dim, widths = 3, 2, [10, 20, 30]
    rng = np.random.default_rng(0)
    n = 1000
    X = rng.uniform(-1, 1, (n, d_in))
    diff = rng.uniform(0.1, 1, (n, 1)); vel = rng.standard_normal((n, dim))
    src = rng.standard_normal((n, 1)); ddx = rng.standard_normal((n, dim))
    rate = rng.uniform(0.5, 2.0, (n, 1))
    eng = VNEngine(dim, d_in, widths, True, 64)
    try:
        eng.init_params(seed=11)
        flat = eng.get_params().astype(np.float64)
        for tag, rx in (('stream', (rate, COEF)), ('unit', (None, COEF)), ('number', (1.5, (-1.0,)))):
            rref = (np.full((n, 1), rx[0]), rx[1]) if np.ndim(rx[0]) == 0 and rx[0] is not None else rx
            uref, ref = reaction_ref.residual(flat, d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, rref, True)
            _, ref0 = reaction_ref.residual(flat, d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, None, True)
            assert np.max(np.abs(ref - ref0)) > 1e-2 * np.max(np.abs(ref))
            scale = max(1, np.max(np.abs(ref)))
            u, r = eng.residual(X, diff, vel, src, ddx, fp64=True, reaction=rx)
            e64 = np.max(np.abs(r.cpu().numpy() - ref[:, 0])) / scale
            assert np.max(np.abs(u.cpu().numpy() - uref[:, 0])) < 1e-13
            u, r = eng.residual(X.astype(np.float32), diff, vel, src, ddx, fp64=False, reaction=rx)
            e32 = np.max(np.abs(r.cpu().numpy() - ref[:, 0])) / scale
            RECORD['residual/' + tag] = {'fp64': float(e64), 'fp32': float(e32)}
            print('reaction residual %s: fp64 %.2e (bar 1e-11), fp32 %.2e (bar 5e-5)' % (tag, e64, e32))
            assert e64 < 1e-11 and e32 < 5e-5
    finally:
        eng.close()


# ---- two training problems, each against its twin -------------------------------------------------------------------------
KAPPA, LAM, T_END = 0.1, 1.0, 0.5
E2E = dict(layerWidth=[20], discNum=20, bDiscNum=None, activationFun='tanh', learning_rate=0.01)
EPOCHS = 10000                     # Adam epochs of every run, twin included (well under a second each on the device)


def _train(pde, path, epochs, **kw):
    np.random.seed(0)
    vn = VarNet(pde, **dict(E2E, **kw))
    vn.train(str(path), epochNum=epochs, tol=0.0, saveFreq=epochs, verbose=False)
    err = vn.residual()[2]
    vn.engine.close()
    return float(err)


def _judge(name, err, twin):
    RECORD['twin/' + name] = {'reaction': err, 'twin': twin, 'bar': min(2.0 * twin + 0.01, 0.2)}
    print('reaction %s: l2 error %.4f with the term, %.4f for the twin (bar %.4f, cap 0.2)' % (name, err, twin, 2.0 * twin + 0.01))
    assert err <= 2.0 * twin + 0.01 and err <= 0.2, (name, err, twin)


def test_decay_1dt_against_its_twin(tmp_path):
    """u_t = kappa u_xx - lambda u on [-1,1] x [0,0.5], IC sin(pi x), Dirichlet 0: u = exp(-(kappa pi^2 + lambda) t) sin(pi x).
    The twin folds the reaction into the source through the exact solution, s' = -lambda u*, and is what the engine could already
    train; same seed, network and epochs.  Bar: err <= 2 err_twin + 0.01 (two optimisation paths to the same weak solution), cap 0.2."""
    dom = lambda: Domain1D(np.array([-1.0, 1.0]))
    cEx = lambda x, t: np.exp(-(KAPPA * pi ** 2 + LAM) * t) * np.sin(pi * x)
    # a run that ignored the term would approach the reaction-free solution, which is far from the exact one at t = T
    x = np.linspace(-1, 1, 201).reshape(-1, 1)
    free = np.exp(-KAPPA * pi ** 2 * T_END) * np.sin(pi * x)
    assert uf.l2Err(cEx(x, T_END), free) > 0.3
    common = dict(diff=KAPPA, vel=0.0, tInterval=[0, T_END], IC=lambda x: np.sin(pi * x), cEx=cEx)
    err = _train(ADPDE(dom(), reaction=(LAM, [-1.0]), **common), tmp_path / 'reaction', EPOCHS, tDiscNum=10)
    twin = _train(ADPDE(dom(), source=lambda x, t=0: -LAM * cEx(x, t), **common), tmp_path / 'twin', EPOCHS, tDiscNum=10)
    _judge('decay_1dt', err, twin)


def test_steady_nonlinear_against_its_twin(tmp_path):
    """0 = u'' + s - 2 (u + u^3) on [-1,1], Dirichlet 0, manufactured u* = 0.8 sin(pi x) (the reaction is monotone: the solution is
    unique).  Twin: s' = s - 2 (u* + u*^3) = 0.8 pi^2 sin(pi x), no reaction."""
    dom = lambda: Domain1D(np.array([-1.0, 1.0]))
    uex = lambda x: 0.8 * np.sin(pi * x)
    s_twin = lambda x, t=0: 0.8 * pi ** 2 * np.sin(pi * x)
    s_full = lambda x, t=0: s_twin(x) + 2.0 * (uex(x) + uex(x) ** 3)
    err = _train(ADPDE(dom(), diff=1.0, vel=0.0, source=s_full, cEx=uex, reaction=(2.0, [-1.0, 0.0, -1.0])),
                 tmp_path / 'reaction', EPOCHS, discNum=40)
    twin = _train(ADPDE(dom(), diff=1.0, vel=0.0, source=s_twin, cEx=uex), tmp_path / 'twin', EPOCHS, discNum=40)
    _judge('steady_nonlinear', err, twin)
