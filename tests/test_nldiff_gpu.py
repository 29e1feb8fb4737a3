"""
GPU tier of the solution-dependent diffusivity (vn_set_nldiff, `ADPDE(nldiff=[d0, d1, d2])`):

    c_t = div(kappa D(c) grad c) - v . grad c - div(w F(c)) + s + rate p(c),      D(c) = d0 + d1 c + d2 c^2.

Parity of the loss components, the loss field and the gradient against the fp64 restatement (tests/nldiff_ref.py) on every route
(generic, single-launch 8-wave -> two-pass sequence, two-pass, layer by layer, de-duplicated), with and without the psi stream,
together with a reaction and a flux term, at a degenerate D = u^2, the fp64 objective at the bars of tests/test_nlflux_gpu.py, the
composition of the step's entry points, the registration contract, the strong residual, and two trained problems judged against a
twin run the engine could train before.  Every test here needs vn_set_nldiff: without the entry point they fail.

Bars are the project's own (tests/parity_cases.py: LOSS_RTOL, GRAD_RTOL through tests/gradcheck.assert_grad_close with its fp32
conditioning callback, LVEC_RTOL).  That the inputs make a missing term fail is a condition asserted on the CPU
(tests/test_nldiff_host.py::test_inputs_make_a_missing_term_fail).

The worst errors per case and route and the trained errors are written to nldiff_parity.json in the directory VN_RECORD_DIR
names (default: profile_out/ beside tests/; the committed copy: profiles/nldiff_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests import flux_ref, nldiff_ref
from tests.gradcheck import assert_grad_close, assert_pair_close, block_errors, fp32_deviation
from tests.nldiff_cases import (CASES, COEF, DEGENERATE, DIFF, FLUX, IDS, inputs, psi, ref_kw, reference, reference64, terms_of,
                                theta)
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.engine import (VN_KERNEL_AUTO, VN_KERNEL_FUSED, VN_KERNEL_FUSED16, VN_KERNEL_GENERIC, VN_KERNEL_LAYERED, VNEngine,
                               VNError)
from varnet_amd.varnet import VarNet

pytestmark = pytest.mark.gpu

pi = np.pi
KEYS = ['loss', 'BCloss', 'ICloss', 'varLoss']
RECORD = {}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'nldiff_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def register_terms(eng, i, variant, batch=0):
    nldiff, nlflux, reaction = terms_of(i, variant)
    if reaction is not None:
        eng.set_reaction(batch, *reaction)
    if nlflux is not None:
        eng.set_nlflux(batch, *nlflux)
    if nldiff is not None:
        eng.set_nldiff(batch, *nldiff)


def register_interior(eng, i, batch=0):
    d = inputs(i)[0]
    eng.set_interior(batch, d['Input'], d['gcoef'], d['source'], n_k=CASES[i][4], detJ=d['detJ'], N_rows=d['N_rows'],
                     dNt_rows=d['dNt_rows'])


def make_engine(i, kernel=VN_KERNEL_AUTO, variant='dpsi', xcheck=False, optimizer='adam'):
    d_in, dim, widths, q, n_k, nB, bDof, td, act, source, integW, detJvec, rows = CASES[i]
    d, _ = inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW, kernel=kernel, activationFun=act, xcheck=xcheck,
                   optimizer_name=optimizer)
    eng.set_params(theta(i))
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    register_interior(eng, i)
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
    eng.set_weights(d['w'])
    register_terms(eng, i, variant)
    return eng


def grad_of(eng, batch=0):
    gb = eng.bind_grad_buffer()
    eng.grad(batch)
    torch.cuda.synchronize()
    return gb.cpu().numpy().astype(np.float64)


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
    print('nldiff %s: %s' % (tag, json.dumps(rec, sort_keys=True)))
    assert np.all(np.isfinite(g))
    for got, key in zip(out, KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'eval', key, got, ref[key])
    for got, key in zip(g[P:], KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'grad', key, got, ref[key])
    assert rec['lossVec'] <= LVEC_RTOL, (tag, rec['lossVec'])
    if g32 is None:
        g32 = lambda: reference(i, variant, dtype=torch.float32)[1]
    assert_grad_close(g[:P], gref, d_in, widths, GRAD_RTOL, dim=dim, td=td, what=tag, g32=g32)
    return g


# ---- parity on every route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_parity(i, kernel):
    """D and psi together, on the automatic route of every case and on the generic kernels."""
    if max(CASES[i][2]) > 64 and kernel == VN_KERNEL_GENERIC:
        # the 128-wide case lies outside the generic kernels: the engine refuses the request (as it does without the term)
        with pytest.raises(VNError, match='error 5'):
            make_engine(i, kernel)
        return
    eng = make_engine(i, kernel)
    try:
        g1 = check_parity(i, eng, 'dpsi', '%s/%s' % (IDS[i], 'auto' if kernel == VN_KERNEL_AUTO else 'generic'))
        assert np.array_equal(g1, grad_of(eng))                     # two grad calls return the same bits
    finally:
        eng.close()


@pytest.mark.parametrize('variant', ['d', 'all', 'pm'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_parity_variants(i, variant):
    """On the automatic route: D alone (psi = None), D and psi together with the reaction's rate stream and the flux term's phi
    stream, and the degenerate D = (0, 0, 1) -- finite and at the bars; the tanh cases have rows with u on both sides of zero and
    within 0.05 of it, where D(u) vanishes."""
    if variant == 'pm' and i in (1, 4, 6):
        u = og.forward(theta(i).astype(np.float64), CASES[i][0], CASES[i][2], torch.float64, inputs(i)[0]['Input'].astype(np.float64),
                       CASES[i][8])
        assert u.min() < 0.0 < u.max() and np.sum(np.abs(u) < 0.05) >= 10
    eng = make_engine(i, variant=variant)
    try:
        check_parity(i, eng, variant, '%s/auto/%s' % (IDS[i], variant))
    finally:
        eng.close()


def test_routes_of_the_cases():
    """What the parity cases run on: integ_num 4, 16 and 64 on the single-launch 8-wave route (whose batches with the term take
    the two-pass sequence), 216 on the two-pass route, 128 wide layer by layer; 300 test functions cross a seed block."""
    want = {0: (VN_KERNEL_FUSED16, 0), 1: (VN_KERNEL_FUSED16, 0), 3: (VN_KERNEL_FUSED16, 0), 4: (VN_KERNEL_FUSED16, 1),
            5: (VN_KERNEL_LAYERED, 0)}
    for i, kp in want.items():
        eng = make_engine(i, variant='none')
        try:
            assert tuple(eng.kernel_path()) == kp, (IDS[i], eng.kernel_path())
        finally:
            eng.close()
    assert [CASES[i][3] for i in (0, 1, 3, 4)] == [4, 16, 64, 216] and CASES[0][4] == 300 > 256


def ref_kw_rows(i, rows, n_use, dtype=torch.float64):
    kw = ref_kw(i, dtype)
    for k in ('Input', 'gcoef', 'N', 'dNt'):
        kw[k] = kw[k][rows]
    kw['intShape'] = [n_use, CASES[i][3]]
    return kw


def test_psi_off_the_16_byte_grid_takes_the_one_row_kernels():
    """The elementwise kernels read four rows per thread when the pointers allow and one row per thread otherwise.  Case 1dt_tanh
    cut to 39 test functions (624 rows: a partly filled last block on either form), psi registered from an aligned tensor and from
    a view one float off the 16-byte grid; both against the reference of those rows."""
    i = 1
    d_in, dim, widths, q, n_k, nB, bDof, td, act = CASES[i][:9]
    d = inputs(i)[0]
    n_use = 39
    rows = slice(0, n_use * q)
    ref, gref = nldiff_ref.loss_and_grad(theta(i).astype(np.float64), d_in, widths, (psi(i)[rows].astype(np.float64), DIFF), None, None,
                                         torch.float64, **ref_kw_rows(i, rows, n_use))
    kw32 = ref_kw_rows(i, rows, n_use, torch.float32)
    g32 = lambda: nldiff_ref.loss_and_grad(theta(i), d_in, widths, (psi(i)[rows], DIFF), None, None, torch.float32, **kw32)[1]
    for tag, off in (('aligned', 0), ('offset_view', 1)):
        eng = VNEngine(dim, d_in, widths, td, q, activationFun=act)
        try:
            eng.set_params(theta(i))
            eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
            eng.set_interior(0, d['Input'][rows], d['gcoef'][rows], None, n_k=n_use, detJ=d['detJ'])
            eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
            eng.set_weights(d['w'])
            buf = torch.zeros(n_use * q + off, device='cuda')
            buf[off:] = torch.as_tensor(psi(i)[rows, 0], device='cuda')
            assert (buf[off:].data_ptr() % 16 == 0) == (off == 0)
            eng.set_nldiff(0, buf[off:], DIFF)
            g = grad_of(eng)
            assert abs(g[eng.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7
            rec = {}
            assert_grad_close(g[:eng.P], gref, d_in, widths, GRAD_RTOL, dim=dim, td=td, what=tag, g32=g32, rec=rec)
            RECORD['1dt_tanh_39/' + tag] = rec
        finally:
            eng.close()


# ---- de-duplicated step ---------------------------------------------------------------------------------------------
def _identity_map(i):
    nT = inputs(i)[0]['Input'].shape[0]
    idx = torch.arange(nT, dtype=torch.int32)
    return inputs(i)[0]['Input'], idx, torch.arange(nT + 1, dtype=torch.int32), idx


@pytest.mark.parametrize('variant', ['dpsi', 'd', 'all'])
def test_dedup_identity_map(variant):
    """Identity point map on the bench network, with and without psi and with the other two terms: against the reference (grad
    and both forms of vn_eval_loss), against the row-wise gradient of the same engine, and two calls give the same bits."""
    i = 3
    d_in, dim, widths = CASES[i][0], CASES[i][1], CASES[i][2]
    eng = make_engine(i, variant=variant)
    try:
        g_row = grad_of(eng)
        eng.set_dedup(0, *_identity_map(i))
        g1 = check_parity(i, eng, variant, '%s/dedup_identity/%s' % (IDS[i], variant))
        g2 = grad_of(eng)
        assert np.array_equal(g1, g2)
        assert not np.array_equal(g1, g_row)                       # another formulation ran
        dev32 = lambda: fp32_deviation(reference(i, variant, dtype=torch.float32)[1], reference64(i, variant)[1], d_in, widths, dim)
        RECORD['%s/dedup_identity/%s/vs_rowwise' % (IDS[i], variant)] = assert_pair_close(
            g1, g_row, d_in, widths, GRAD_RTOL, dim=dim, dev32=dev32, what='dedup vs row-wise')
        # row-wise eval_loss of the same batch (debug route 8) agrees with the de-duplicated one
        out_dd, _ = eng.eval_loss(0)
        eng.debug_point_route(8)
        out_rw, _ = eng.eval_loss(0)
        eng.debug_point_route(0)
        ref = reference64(i, variant)[0]
        for a, b, k in zip(out_dd, out_rw, KEYS):
            assert abs(a - b) <= LOSS_RTOL * abs(b) + 1e-7
            assert abs(b - ref[k]) <= LOSS_RTOL * abs(ref[k]) + 1e-7
    finally:
        eng.close()


def test_dedup_with_a_zero_table_entry_is_an_error_code():
    """The fold of the term into the de-duplicated assembly divides by N_p: a table with a zero entry is refused, on either
    order of the two registrations and at the step, and the batch stays usable row-wise."""
    i = 3
    d = inputs(i)[0]
    N0 = np.array(d['N1'], dtype=np.float32).copy()
    N0[5] = 0.0
    eng = make_engine(i, variant='none')
    try:
        eng.set_fe_table(N0, d['dNt1'], d['integW'])
        eng.set_nldiff(0, psi(i), DIFF)
        with pytest.raises(VNError, match=r'error 5: the diffusivity D\(u\) of batch 0 cannot be de-duplicated'):
            eng.set_dedup(0, *_identity_map(i))
        g = grad_of(eng)                                             # row-wise, with the term
        assert np.all(np.isfinite(g))
        eng.set_nldiff(0)
        eng.set_dedup(0, *_identity_map(i))
        with pytest.raises(VNError, match=r'error 5: the diffusivity D\(u\) of batch 0 cannot join its de-duplication map'):
            eng.set_nldiff(0, psi(i), DIFF)
        # the table changes after both registrations were accepted: the step itself returns the code
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        eng.set_nldiff(0, psi(i), DIFF)
        eng.set_fe_table(N0, d['dNt1'], d['integW'])
        with pytest.raises(VNError, match=r'error 5: the diffusivity D\(u\) of a de-duplicated batch needs'):
            eng.grad(0)
        with pytest.raises(VNError, match=r'error 5: the diffusivity D\(u\) of a de-duplicated batch needs'):
            eng.eval_loss(0)
    finally:
        eng.close()


def kappa_fun(x, t=0):
    return 1.0 + 0.5 * x ** 2 + 0.2 * t


def vel_fun(x, t=0):
    return 0.5 + 0.3 * x + 0.1 * t


def divv_fun(x, t=0):
    return 0.3 * np.ones([len(x), 1])


def w_fun(x, t=0):
    return 1.0 + 0.5 * x + t


def rate_fun(x, t=0):
    return 1.0 + 0.5 * x ** 2 + t


def _varnet_reference(vn, td, with_d, others, dtype=torch.float64):
    fd, d = vn.fixData, td.mor[0]
    f = np.float64 if dtype == torch.float64 else np.float32
    Nr, dNxr, dNtr = fd.rows()                                   # (rounded to fp32 below: the engine's tables are fp32)
    cpu = lambda t: t.cpu().numpy().astype(f)
    col = lambda t: cpu(t).reshape(-1, 1)
    kw = dict(Input=cpu(d['Input']), gcoef=cpu(d['gcoef']), source=None if d['source'] is None else col(d['source']),
              N=Nr.astype(np.float32).astype(f), dNt=dNtr.astype(np.float32).astype(f), integW=None, intShape=[fd.nt, fd.integNum],
              detJ=float(fd.detJ), detJvec=False, biInput=cpu(d['biInput']), biLabel=col(d['biLabel']), bDof=fd.bDofsum,
              biDimVal=float(fd.biDimVal), w=np.ones(3), dim=vn.dim, time_dependent=True, is_source=vn.lossOpt['isSource'],
              integWflag=False)
    nldiff = (col(d['psi']), DIFF if with_d else (1.0, 0.0, 0.0))
    nlflux = (col(d['phi']), FLUX) if others else None
    reaction = (col(d['rate']), COEF) if others else None
    return nldiff_ref.loss_and_grad(vn.engine.get_params().astype(f), vn.inpDim, vn.layerWidth, nldiff, nlflux, reaction, dtype, **kw)


@pytest.mark.parametrize('others', [False, True], ids=['nldiff', 'all'])
def test_dedup_shared_points_through_varnet(others):
    """A real shared-point map on a uniform 1D+t grid, built by VarNet with a variable kappa and velocity: gcoef = kappa dN/dx and
    the psi stream are uploaded per row, enable_dedup keeps the registration, and the de-duplicated gradient agrees with the
    reference and with the row-wise one; without and with a reaction and a flux term on the same batch.  (kappa ~ 1 and the initial
    parameters x 4: in the fp64 reference D then moves varLoss by 0.06 / 0.25 and the least-moved gradient tensor by 0.14 / 0.13.)"""
    kw = {'reaction': (rate_fun, list(COEF)), 'nlflux': (w_fun, list(FLUX))} if others else {}
    pde = ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=kappa_fun, vel=vel_fun, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x),
                nldiff=(list(DIFF), divv_fun), **kw)
    vn = VarNet(pde, layerWidth=[20, 20], discNum=12, bDiscNum=None, tDiscNum=10)
    eng = vn.engine
    tag = 'varnet_1dt' + ('_all' if others else '')
    try:
        eng.set_params(4.0 * (eng.get_params() + 0.05 * np.random.default_rng(5).standard_normal(eng.P).astype(np.float32)))
        td = vn._build_tdata()
        td.select_mor(0)
        eng.set_weights([1.0, 1.0, 1.0])
        X = td.mor[0]['Input_host']
        fd = vn.fixData
        x, t = X[:, 0:1], X[:, 1:2]
        dNx, N = np.tile(fd.dNx[:, 0:1], (fd.nt, 1)), np.tile(np.reshape(fd.N, (-1, 1)), (fd.nt, 1))
        np.testing.assert_allclose(td.mor[0]['psi'].cpu().numpy().reshape(-1, 1), vel_fun(x, t) * dNx + 0.3 * N, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(td.mor[0]['gcoef'].cpu().numpy(), kappa_fun(x, t) * dNx, rtol=1e-6, atol=1e-7)
        ref, gref = _varnet_reference(vn, td, True, others)
        ref0, g0 = _varnet_reference(vn, td, False, others)
        dl = abs(ref['varLoss'] - ref0['varLoss']) / abs(ref['varLoss'])
        blk = min(block_errors(g0, gref, vn.inpDim, vn.layerWidth, 1).values())
        print('nldiff %s: D moves varLoss by %.3g and the least-moved gradient tensor by %.3g' % (tag, dl, blk))
        assert dl >= 100 * LOSS_RTOL and blk >= 100 * GRAD_RTOL, (dl, blk)       # (a condition on the inputs, from the reference)
        g32 = lambda: _varnet_reference(vn, td, True, others, torch.float32)[1]
        g_row = grad_of(eng)
        P = eng.P
        assert abs(g_row[P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7
        rec = {}
        assert_grad_close(g_row[:P], gref, vn.inpDim, vn.layerWidth, GRAD_RTOL, dim=1, what='varnet row-wise', g32=g32, rec=rec)
        RECORD[tag + '/rowwise'] = rec
        U = td.enable_dedup()
        assert td.dedup_reason is None and 0 < U < vn.fixData.nT / 2, (td.dedup_reason, U)
        g1 = grad_of(eng)
        g2 = grad_of(eng)
        assert np.array_equal(g1, g2) and not np.array_equal(g1, g_row)
        for k in range(4):
            assert abs(g1[P + k] - ref[KEYS[k]]) <= LOSS_RTOL * abs(ref[KEYS[k]]) + 1e-7, (KEYS[k], g1[P + k], ref[KEYS[k]])
        rec = {}
        assert_grad_close(g1[:P], gref, vn.inpDim, vn.layerWidth, GRAD_RTOL, dim=1, what='varnet dedup', g32=g32, rec=rec)
        RECORD[tag + '/dedup'] = rec
        dev32 = lambda: fp32_deviation(g32(), gref, vn.inpDim, vn.layerWidth, 1)
        RECORD[tag + '/dedup_vs_rowwise'] = assert_pair_close(g1, g_row, vn.inpDim, vn.layerWidth, GRAD_RTOL, dim=1,
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
@pytest.mark.parametrize('variant', ['dpsi', 'd', 'all'])
@pytest.mark.parametrize('i', [0, 1, 2, 3, 4, 6], ids=[IDS[k] for k in (0, 1, 2, 3, 4, 6)])
def test_objective64_parity(i, variant):
    """vn_objective_f64 against the reference at the bars of tests/test_nlflux_gpu.py: loss components 1e-12, gradient blocks
    1e-11, lossVec 1e-11 of its maximum.  Parameters in fp64 (not fp32-representable)."""
    d_in, dim, widths, td = CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][7]
    th = theta(i).astype(np.float64) + 1e-3 * np.random.default_rng(6).standard_normal(theta(i).size)
    ref, gref = reference(i, variant, flat=th)
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
        print('nldiff objective64 %s %s: %s' % (IDS[i], variant, json.dumps(rec, sort_keys=True)))
        for key in KEYS:
            assert rec[key] <= 1e-12, (key, rec[key])
        assert rec['lossVec'] <= 1e-11, rec['lossVec']
        assert rec['worst_block_err'] <= 1e-11, (rec['worst_block'], rec['worst_block_err'])
        # loss-only form and a second call: same bits
        out2, _, _ = eng.objective64(0, theta=th, grad=False)
        assert out2 == out
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
    measured first without the term, then required to hold with it (tests/test_nlflux_gpu.py measures it the same way)."""
    eng = make_engine(i, variant='none')
    try:
        s0 = eng.export_state()
        flat = eng.get_params()
        gap = []
        for with_term in (False, True):
            if with_term:
                register_terms(eng, i, 'dpsi')
            a = _theta_after(eng, s0, lambda: eng.train_step(0))
            b = _theta_after(eng, s0, lambda: (eng.grad(0), eng.apply()))
            assert np.max(np.abs(a - flat)) > 1e-4                       # the step moved theta
            gap.append(float(np.max(np.abs(a - b))))
        assert gap[1] <= max(2.0 * gap[0], 1e-6), gap
    finally:
        eng.close()


def test_train_epoch_over_two_batches_one_with_the_term():
    i = 3
    eng = make_engine(i)                                                # batch 0 carries D and psi
    plain = make_engine(i, variant='none')
    try:
        register_interior(eng, i, batch=1)                              # batch 1: the same rows, no term
        g1 = grad_of(eng, 1)
        assert np.array_equal(g1, grad_of(plain))                       # ... keeps the single launch, bit for bit
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


def test_lbfgs_step_decreases_the_objective_with_the_term():
    i = 2
    eng = make_engine(i, optimizer='lbfgs')
    try:
        ref = reference64(i, 'dpsi')[0]
        info = eng.lbfgs_step(0)
        assert abs(info['f_k'] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7        # the objective has the term
        assert info['status'] == 0 and info['f_next'] < info['f_k'], info
        out, _ = eng.eval_loss(0)
        assert abs(out[0] - info['f_next']) <= LOSS_RTOL * abs(out[0]) + 1e-7
        # a change of the registration invalidates (f_k, g_k): the next call evaluates the new objective first
        eng.set_nldiff(0)
        out0, _ = eng.eval_loss(0)
        info = eng.lbfgs_step(0)
        assert abs(info['f_k'] - out0[0]) <= LOSS_RTOL * abs(out0[0]) + 1e-7 and info['pairs'] == 0, info
    finally:
        eng.close()


@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
def test_flux_bc_rows_and_the_term_together(kernel):
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
        res, g = reference(i, 'dpsi', dtype=dtype)
        w = inputs(i)[0]['w']
        F, gF, _ = flux_ref.flux_term(theta(i).astype(f), d_in, widths, dim, fx['X'].astype(f), fx['normal'].astype(f),
                                      fx['coef'].astype(f), fx['label'].astype(f), 2.0, CASES[i][8], dtype)
        res = dict(res)
        res['BCloss'] = res['BCloss'] + F
        res['loss'] = res['loss'] + w[0] * F
        return res, g + w[0] * gF

    ref = ref_with_flux(torch.float64)
    assert abs(ref[0]['BCloss'] - reference64(i, 'dpsi')[0]['BCloss']) > 1e-2 * abs(ref[0]['BCloss'])
    eng = make_engine(i, kernel)
    try:
        eng.set_flux_bc(fx['X'], fx['normal'], fx['coef'], fx['label'], 2.0)
        check_parity(i, eng, 'dpsi', '%s/flux_bc/%s' % (IDS[i], 'auto' if kernel == VN_KERNEL_AUTO else 'generic'), ref=ref,
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
    """Never registered; registered, stepped and cleared (coef None; D = 1 without psi); registered and a new vn_set_interior: the
    same bits in eval_loss, lossVec, grad and three training steps."""
    runs = []
    for how in ('never', 'cleared', 'cleared_unit', 'reregistered'):
        eng = make_engine(i, kernel, variant='none' if how == 'never' else 'dpsi')
        try:
            if how == 'cleared':
                eng.grad(0)                                             # a step with the term ...
                eng.set_nldiff(0)                                       # ... then cleared
            elif how == 'cleared_unit':
                eng.grad(0)
                eng.set_nldiff(0, None, (1.0, 0.0, 0.0))
            elif how == 'reregistered':
                eng.grad(0)
                register_interior(eng, i)                               # a new vn_set_interior clears the registration
            runs.append(_snapshot(eng))
        finally:
            eng.close()
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert np.array_equal(x, y)


def test_the_registrations_keep_each_other():
    """vn_set_dedup, vn_set_reaction, vn_set_nlflux and vn_set_nldiff in several orders give the same bits, with the three terms and
    the map in place; clearing D leaves the other two terms and the map (the de-duplicated step the engine had before)."""
    i = 3
    ref = reference64(i, 'all')[0]
    nldiff, nlflux, reaction = terms_of(i, 'all')
    steps = {'map': lambda e: e.set_dedup(0, *_identity_map(i)), 'react': lambda e: e.set_reaction(0, *reaction),
             'flux': lambda e: e.set_nlflux(0, *nlflux), 'diff': lambda e: e.set_nldiff(0, *nldiff)}
    grads = []
    for order in (('map', 'react', 'flux', 'diff'), ('diff', 'flux', 'react', 'map'), ('react', 'diff', 'map', 'flux'),
                  ('diff', 'map', 'react', 'flux')):
        eng = make_engine(i, variant='none')
        try:
            g_row = grad_of(eng).copy()
            for s in order:
                steps[s](eng)
            g = grad_of(eng)
            assert abs(g[eng.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7      # the three terms are there
            grads.append(g.copy())
            if order == ('map', 'react', 'flux', 'diff'):
                eng.debug_point_route(8)
                out_rw, _ = eng.eval_loss(0)                                              # row-wise evaluation of the same batch
                eng.debug_point_route(0)
                assert abs(out_rw[0] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7
                eng.set_nldiff(0)                                                         # the other terms and the map stay
                g_r = grad_of(eng)
                ref_r = reference64(i, 'rf')[0]
                assert abs(g_r[eng.P] - ref_r['loss']) <= LOSS_RTOL * abs(ref_r['loss']) + 1e-7
                only = make_engine(i, variant='rf')
                try:
                    only.set_dedup(0, *_identity_map(i))
                    assert np.array_equal(g_r, grad_of(only))
                finally:
                    only.close()
            assert not np.array_equal(g, g_row)
        finally:
            eng.close()
    for g in grads[1:]:
        assert np.array_equal(grads[0], g)


def test_refusals():
    i = 2
    ps = psi(i)
    eng = make_engine(i, VN_KERNEL_FUSED, variant='none')               # the 4-wave cross-check geometry
    try:
        with pytest.raises(VNError, match=r'error 5: the diffusivity D\(u\) is not built for VN_KERNEL_FUSED'):
            eng.set_nldiff(0, ps, DIFF)
        with pytest.raises(VNError, match=r'error 5: the diffusivity D\(u\) is not built for VN_KERNEL_FUSED'):
            eng.set_nldiff(0, ps, (1.0, 0.0, 0.0))                      # D = 1 WITH psi is a registration, not a clear
        eng.set_nldiff(0)                                               # clearing is always accepted
        eng.set_nldiff(0, None, (1.0, 0.0, 0.0))
    finally:
        eng.close()
    eng = make_engine(i, variant='none')
    try:
        with pytest.raises(VNError, match='error 1: diffusivity coefficients'):
            eng.set_nldiff(0, ps, (1.0, float('nan'), 0.0))
        with pytest.raises(VNError, match='error 1: diffusivity coefficients'):
            eng.set_nldiff(0, None, (float('inf'), 0.0, 0.0))
        with pytest.raises(VNError, match='error 3'):
            eng.set_nldiff(5, ps, DIFF)                                 # an unregistered batch
        d_in, dim = CASES[i][0], CASES[i][1]
        eng.set_interior(1, torch.zeros(0, d_in, device='cuda'), torch.zeros(0, dim, device='cuda'), None, n_k=0, detJ=0.1)
        with pytest.raises(VNError, match='error 1: batch 1 has no interior rows'):
            eng.set_nldiff(1, torch.zeros(0, device='cuda'), DIFF)
        with pytest.raises(ValueError, match='at most three coefficients'):
            eng.set_nldiff(0, ps, (1.0, 2.0, 3.0, 4.0))
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
    """VNEngine.residual(..., nldiff=coef) in fp64 at 1e-11 and in fp32 at 5e-5 of max(1, |residual|_inf) against
    nldiff_ref.residual: alone, at the degenerate D = u^2, and together with a flux term and a reaction.  The parameters are the
    initial ones x 3, so that grad u (~1e-3 at initialisation) makes kappa D'(u) |grad u|^2 a real part of the residual."""
    d_in, dim, widths = 3, 2, [10, 20, 30]
    rng = np.random.default_rng(0)
    n = 1000
    X = rng.uniform(-1, 1, (n, d_in))
    diff = rng.uniform(0.1, 1, (n, 1)); vel = rng.standard_normal((n, dim))
    src = rng.standard_normal((n, 1)); ddx = rng.standard_normal((n, dim))
    w = rng.standard_normal((n, dim)); divw = rng.standard_normal((n, 1)); rate = rng.uniform(0.5, 2.0, (n, 1))
    eng = VNEngine(dim, d_in, widths, True, 64)
    try:
        eng.init_params(seed=11)
        eng.set_params(3.0 * eng.get_params())
        flat = eng.get_params().astype(np.float64)
        _, ref0 = nldiff_ref.residual(flat, d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, None)
        for tag, dc, kw in (('D', DIFF, {}), ('degenerate', DEGENERATE, {}),
                            ('all', DIFF, dict(nlflux=(w, FLUX, divw), reaction=(rate, COEF)))):
            uref, ref = nldiff_ref.residual(flat, d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, dc, **kw)
            _, lin = nldiff_ref.residual(flat, d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, None, **kw)
            scale = max(1, np.max(np.abs(ref)))
            # the term is at least a hundred times the wider (fp32) bar: a residual without it fails both bars
            assert np.max(np.abs(ref - lin)) > 100 * 5e-5 * scale, (tag, np.max(np.abs(ref - lin)), scale)
            u, r = eng.residual(X, diff, vel, src, ddx, fp64=True, nldiff=dc, **kw)
            e64 = np.max(np.abs(r.cpu().numpy() - ref[:, 0])) / scale
            assert np.max(np.abs(u.cpu().numpy() - uref[:, 0])) < 1e-13
            u, r = eng.residual(X.astype(np.float32), diff, vel, src, ddx, fp64=False, nldiff=dc, **kw)
            e32 = np.max(np.abs(r.cpu().numpy() - ref[:, 0])) / scale
            RECORD['residual/' + tag] = {'fp64': float(e64), 'fp32': float(e32)}
            print('nldiff residual %s: fp64 %.2e (bar 1e-11), fp32 %.2e (bar 5e-5)' % (tag, e64, e32))
            assert e64 < 1e-11 and e32 < 5e-5
        # D = 1: the residual the engine computed before, bit for bit on the fp32 path's inputs
        _, r1 = eng.residual(X, diff, vel, src, ddx, fp64=True, nldiff=(1.0, 0.0, 0.0))
        assert np.max(np.abs(r1.cpu().numpy() - ref0[:, 0])) / max(1, np.max(np.abs(ref0))) < 1e-11
    finally:
        eng.close()


# ---- two trained problems, each against its twin --------------------------------------------------------------------------
E2E = dict(layerWidth=[20], discNum=20, bDiscNum=None, activationFun='tanh', learning_rate=0.01)
EPOCHS = 10000                                       # Adam epochs of every run, twins included
KAPPA, DCOEF = 0.1, [1.0, 0.0, 2.0]


def _train(pde, path, **kw):
    np.random.seed(0)
    vn = VarNet(pde, **dict(E2E, **kw))
    vn.train(str(path), epochNum=EPOCHS, tol=0.0, saveFreq=EPOCHS, verbose=False)
    err = vn.residual()[2]
    vn.engine.close()
    return float(err)


def _judge(name, err, twin, extra=None):
    """The twin rule of DESIGN.md sections 14-15: err <= 2 err_twin + 0.01, cap 0.2, and the twin itself has to reach 0.05."""
    RECORD['twin/' + name] = dict({'nldiff': err, 'twin': twin, 'bar': min(2.0 * twin + 0.01, 0.2), 'epochs': EPOCHS}, **(extra or {}))
    print('nldiff %s: l2 error %.4f with the term, %.4f for the twin (bar %.4f, cap 0.2), %d epochs%s'
          % (name, err, twin, 2.0 * twin + 0.01, EPOCHS, '' if not extra else ' ' + json.dumps(extra)))
    assert twin <= 0.05, (name, 'twin', twin)
    assert err <= 2.0 * twin + 0.01 and err <= 0.2, (name, err, twin)


def _manufactured(v):
    """u* = exp(-t) sin(pi x) on [-1,1] x [0,1]; sources of  u_t = (kappa D(u) u_x)_x - v u_x + s  (D = 1 + 2 u^2) and of its
    linear twin  u_t = kappa u_xx - v u_x + s'."""
    cEx = lambda x, t=0: np.exp(-t) * np.sin(pi * x)
    ux = lambda x, t: pi * np.exp(-t) * np.cos(pi * x)
    uxx = lambda x, t: -pi ** 2 * cEx(x, t)
    D = lambda u: DCOEF[0] + DCOEF[1] * u + DCOEF[2] * u ** 2
    dD = lambda u: DCOEF[1] + 2.0 * DCOEF[2] * u
    s_nl = lambda x, t=0: -cEx(x, t) - KAPPA * (D(cEx(x, t)) * uxx(x, t) + dD(cEx(x, t)) * ux(x, t) ** 2) + v * ux(x, t)
    s_lin = lambda x, t=0: -cEx(x, t) - KAPPA * uxx(x, t) + v * ux(x, t)
    common = dict(diff=KAPPA, vel=v, tInterval=[0, 1.0], IC=lambda x: cEx(x, 0.0), cEx=cEx, BCs=[[0.0, 1.0, cEx], [0.0, 1.0, cEx]])
    return common, s_nl, s_lin


def test_quasilinear_diffusion_against_its_twin(tmp_path):
    """u_t = (kappa (1 + 2 u^2) u_x)_x + s with the source manufactured from u* = exp(-t) sin(pi x), kappa = 0.1, against the
    linear problem the engine could already train (diff = 0.1, s' = u*_t - 0.1 u*_xx); same seed, network and epochs.  Also the
    same nonlinear source WITHOUT nldiff (a run that ignores the term solves another PDE): its error is recorded and only has to
    exceed the error of the run with the term."""
    dom = lambda: Domain1D(np.array([-1.0, 1.0]))
    common, s_nl, s_lin = _manufactured(0.0)
    twin = _train(ADPDE(dom(), source=s_lin, **common), tmp_path / 'twin', tDiscNum=10)
    err = _train(ADPDE(dom(), source=s_nl, nldiff=DCOEF, **common), tmp_path / 'nldiff', tDiscNum=10)
    left_out = _train(ADPDE(dom(), source=s_nl, **common), tmp_path / 'left_out', tDiscNum=10)
    _judge('quasilinear', err, twin, {'nldiff_left_out': left_out})
    assert left_out > err, (left_out, err)


def test_quasilinear_diffusion_with_advection_against_its_twin(tmp_path):
    """The same with vel = 0.5: the advection trains through the psi stream; its twin is the linear advection-diffusion run."""
    dom = lambda: Domain1D(np.array([-1.0, 1.0]))
    common, s_nl, s_lin = _manufactured(0.5)
    twin = _train(ADPDE(dom(), source=s_lin, **common), tmp_path / 'twin', tDiscNum=10)
    err = _train(ADPDE(dom(), source=s_nl, nldiff=DCOEF, **common), tmp_path / 'nldiff', tDiscNum=10)
    _judge('quasilinear_advection', err, twin)
