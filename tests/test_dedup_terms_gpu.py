"""
GPU tier: the three nonlinear terms (vn_set_reaction, vn_set_nlflux, vn_set_nldiff) in the de-duplicated step, on shared-point
maps.  The six term kernels of that step (vn_react_source / vn_react_gather, vn_nlflux_source / vn_nlflux_gather,
vn_nldiff_source / vn_nldiff_point) and their chaining through the engine's one s_eff buffer (run_dedup, eval_dedup) against the
fp64 restatement tests/nldiff_ref.py on the expanded rows Input = Xu[uid], at the branches tests/dedup_term_cases.py lists: rows
to (test function, quadrature point) by division, CSR segments of 1..11 rows, the integW factor, the periodic gcoef table, dim 3,
steady problems, MOR-shaped inputs, a plain source below each term alone, unique points that own no row, and batches of
different sizes sharing the engine-level buffers; and a real 2D+t grid (8 rows per interior point) built by VarNet.

Bars are the project's own (tests/parity_cases.py: LOSS_RTOL, GRAD_RTOL through tests/gradcheck.assert_grad_close with its fp32
conditioning callback, LVEC_RTOL).  That the inputs make a missing term fail is a condition asserted on the CPU
(tests/test_dedup_terms_host.py::test_inputs_make_a_missing_term_fail).

The errors per case, variant and route are written to dedup_terms_parity.json in the directory VN_RECORD_DIR names (default:
profile_out/ beside tests/; the committed copy: profiles/dedup_terms_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import nldiff_ref
from tests.dedup_term_cases import (BIDIMVAL, CASES, COEF, DETJ, DIFF, EMPTY, FLUX, IDS, ONE, PERIODIC, VARIANTS, big_batch, empty_map,
                                    inputs, reference, reference64, terms_of, theta)
from tests.gradcheck import assert_grad_close, assert_pair_close, block_errors, fp32_deviation
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import PolygonDomain2D
from varnet_amd.engine import VNEngine
from varnet_amd.varnet import VarNet

pytestmark = pytest.mark.gpu

pi = np.pi
KEYS = ['loss', 'BCloss', 'ICloss', 'varLoss']
RECORD = {}
BENCH = 0                                        # CASES[0]: the bench network on a random map


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'dedup_terms_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


# ---- engine-level helpers -------------------------------------------------------------------------------------------
def new_engine(i):
    """An engine of CASES[i] with its parameters, tables, BC/IC rows and weights; no batch yet."""
    d_in, dim, widths, q, n_k, U, nB, bDof, source, integW, td, act = CASES[i][:12]
    d = inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW, activationFun=act)
    eng.set_params(theta(i))
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, BIDIMVAL)
    eng.set_weights(d['w'])
    return eng


def register_interior(eng, i, batch=0, d=None, gcoef=None):
    d = inputs(i) if d is None else d
    eng.set_interior(batch, d['Input'], d['gcoef'] if gcoef is None else gcoef, d['source'], n_k=d['Input'].shape[0] // CASES[i][3],
                     detJ=DETJ)


def register_terms(eng, i, variant, batch=0, d=None, order=('react', 'flux', 'diff')):
    nldiff, nlflux, reaction = terms_of(i, variant, d)
    for which in order:
        if which == 'react' and reaction is not None:
            eng.set_reaction(batch, *reaction)
        if which == 'flux' and nlflux is not None:
            eng.set_nlflux(batch, *nlflux)
        if which == 'diff' and nldiff is not None:
            eng.set_nldiff(batch, *nldiff)


def register_map(eng, i, batch=0, d=None, empty=False):
    d = inputs(i) if d is None else d
    Xu, rowptr = empty_map(i) if empty else (d['Xu'], d['rowptr'])
    eng.set_dedup(batch, Xu, d['uid'], rowptr, d['rowidx'])


def make_engine(i, variant, empty=False):
    """The interior, the terms and then the map."""
    eng = new_engine(i)
    register_interior(eng, i)
    register_terms(eng, i, variant)
    register_map(eng, i, empty=empty)
    return eng


def grad_of(eng, batch=0):
    gb = eng.bind_grad_buffer()
    eng.grad(batch)
    torch.cuda.synchronize()
    return gb.cpu().numpy().astype(np.float64)


def _rel(got, want):
    return abs(got - want) / max(abs(want), 1e-300) if want != 0.0 else abs(got)


def check_parity(i, eng, tag, ref, g32, batch=0, rowwise_eval=False, net=None, record=None):
    """eval_loss (with lossVec) and grad of a batch against the reference (ref, gref); with rowwise_eval also the row-wise
    evaluation of a batch that carries a map (debug_point_route(8)).  Prints and records every figure, then asserts.  net, record:
    (d_in, dim, widths, td) and the record of a caller whose case is not one of CASES (tests/test_dedup_maps_gpu.py)."""
    d_in, dim, widths, td = (CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][10]) if net is None else net
    ref, gref = ref
    evals = {'eval': eng.eval_loss(batch, lossVec=True)}
    if rowwise_eval:
        eng.debug_point_route(8)
        try:
            evals['eval_rowwise'] = eng.eval_loss(batch, lossVec=True)
        finally:
            eng.debug_point_route(0)
    g = grad_of(eng, batch)
    P = eng.P
    lref = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1)
    rec = {}
    for name, (out, lv) in evals.items():
        rec.update({name + '_' + k: _rel(got, ref[k]) for got, k in zip(out, KEYS)})
        rec[name + '_lossVec'] = float(np.max(np.abs(lv.cpu().numpy().astype(np.float64) - lref)) / np.max(np.abs(lref)))
    rec.update({'grad_' + k: _rel(got, ref[k]) for got, k in zip(g[P:], KEYS)})
    errs = block_errors(g, gref, d_in, widths, dim, td)
    rec['worst_block'] = max(errs, key=errs.get)
    rec['worst_block_err'] = errs[rec['worst_block']]
    rec['kernel_path'] = list(eng.kernel_path())
    (RECORD if record is None else record)[tag] = rec
    print('dedup terms %s: %s' % (tag, json.dumps(rec, sort_keys=True)))
    assert np.all(np.isfinite(g))
    for name, (out, lv) in evals.items():
        for got, key in zip(out, KEYS):
            assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, name, key, got, ref[key])
        assert rec[name + '_lossVec'] <= LVEC_RTOL, (tag, name, rec[name + '_lossVec'])
        assert td or out[2] == 0.0
    for got, key in zip(g[P:], KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'grad', key, got, ref[key])
    if rowwise_eval:          # (a batch with a map) the loss scalars the step reports are those of the loss-only form of its assembly
        assert np.allclose(evals['eval'][0], g[P:P + 4], rtol=2e-6), (tag, evals['eval'][0], g[P:P + 4])
    assert_grad_close(g[:P], gref, d_in, widths, GRAD_RTOL, dim=dim, td=td, what=tag, g32=g32)
    return g


def both_routes(i, eng, variant, tag):
    """The checks of test_parity on an engine whose batch 0 carries the terms and a map: the de-duplicated step and both forms of
    eval_loss against the reference, two calls the same bits; then the map cleared: the row-wise step of the same engine against
    the reference and against the de-duplicated one, with other bits.  Returns (de-duplicated, row-wise) gradients."""
    d_in, dim, widths, td = CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][10]
    ref = reference64(i, variant)
    g32 = lambda: reference(i, variant, dtype=torch.float32)[1]
    g_dd = check_parity(i, eng, tag + '/dedup', ref, g32, rowwise_eval=True)
    assert np.array_equal(g_dd, grad_of(eng))                       # two de-duplicated calls: the same bits
    eng.set_dedup(0)                                                # the terms stay; the batch is row-wise again
    g_row = check_parity(i, eng, tag + '/rowwise', ref, g32)
    assert not np.array_equal(g_dd, g_row)                          # another formulation ran
    dev32 = lambda: fp32_deviation(g32(), ref[1], d_in, widths, dim, td)
    RECORD[tag + '/dedup_vs_rowwise'] = assert_pair_close(g_dd, g_row, d_in, widths, GRAD_RTOL, dim=dim, td=td, dev32=dev32,
                                                          what=tag + ' dedup vs row-wise')
    return g_dd, g_row


# ---- parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_parity(i, variant):
    """Every case with D, psi, the flux term and the reaction together and with each of the four alone."""
    eng = make_engine(i, variant)
    try:
        both_routes(i, eng, variant, '%s/%s' % (IDS[i], variant))
    finally:
        eng.close()


@pytest.mark.parametrize('i', EMPTY, ids=[IDS[k] for k in EMPTY])
def test_empty_points(i):
    """A map in which about 5 % of the unique points own no row (rowptr[j] == rowptr[j+1]): the same checks, and the gradient
    agrees with that of the map without those points (other launch shapes: the bits may differ)."""
    d_in, dim, widths, td = CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][10]
    eng = make_engine(i, 'all', empty=True)
    try:
        g_empty, _ = both_routes(i, eng, 'all', '%s/all/empty_points' % IDS[i])
        register_map(eng, i)
        g_full = grad_of(eng)
        dev32 = lambda: fp32_deviation(reference(i, 'all', dtype=torch.float32)[1], reference64(i, 'all')[1], d_in, widths, dim, td)
        RECORD['%s/all/empty_points/vs_full_map' % IDS[i]] = assert_pair_close(
            g_empty, g_full, d_in, widths, GRAD_RTOL, dim=dim, td=td, dev32=dev32, what='empty points vs the full map')
        for k in range(4):
            assert abs(g_empty[eng.P + k] - g_full[eng.P + k]) <= LOSS_RTOL * abs(g_full[eng.P + k]) + 1e-7
    finally:
        eng.close()


@pytest.mark.parametrize('variant', ['all', 'd'])
@pytest.mark.parametrize('i', PERIODIC, ids=[IDS[k] for k in PERIODIC])
def test_periodic_table_is_bitwise_the_csr_path(i, variant):
    """A gcoef that repeats with period integ_num is read as an integ_num-entry table by vn_nldiff_source_kernel and the assembly
    kernels; debug_point_route(4) at vn_set_dedup keeps the CSR-ordered copy instead.  Same gradient bits, same eval_loss numbers;
    one row perturbed off the period still meets the reference of that data."""
    q = CASES[i][3]
    eng = new_engine(i)
    try:
        def run(route, gcoef=None):
            register_interior(eng, i, gcoef=gcoef)
            register_terms(eng, i, variant)
            eng.debug_point_route(route)
            try:
                register_map(eng, i)
            finally:
                eng.debug_point_route(0)
            out, lv = eng.eval_loss(0, lossVec=True)
            return grad_of(eng), out, lv.cpu().numpy()
        g_tab, out_tab, lv_tab = run(0)
        g_csr, out_csr, lv_csr = run(4)
        assert np.array_equal(g_tab, g_csr)
        assert out_tab == out_csr and np.array_equal(lv_tab, lv_csr)
        g2 = np.array(inputs(i)['gcoef'])
        g2[5 * q + 3, 0] += np.float32(0.75 * CASES[i][13])
        run(0, g2)
        ref = reference(i, variant, gcoef=g2)
        g_off = check_parity(i, eng, '%s/%s/off_period' % (IDS[i], variant), ref,
                             lambda: reference(i, variant, dtype=torch.float32, gcoef=g2)[1], rowwise_eval=True)
        assert not np.array_equal(g_off, g_tab)
    finally:
        eng.close()


def test_registration_order():
    """The terms before vn_set_dedup, after it, and in reverse order: the same bits."""
    i = BENCH
    grads = []
    for order in (('react', 'flux', 'diff', 'map'), ('map', 'react', 'flux', 'diff'), ('diff', 'flux', 'react', 'map'),
                  ('diff', 'map', 'flux', 'react')):
        eng = new_engine(i)
        try:
            register_interior(eng, i)
            for s in order:
                if s == 'map':
                    register_map(eng, i)
                else:
                    register_terms(eng, i, 'all', order=(s,))
            grads.append(grad_of(eng))
        finally:
            eng.close()
    ref = reference64(i, 'all')[0]
    assert abs(grads[0][-4] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7          # the three terms are there
    for g in grads[1:]:
        assert np.array_equal(grads[0], g)


def test_shared_buffers_across_batches():
    """s_eff and the other work buffers of the terms belong to the engine, not to a batch.  Batch 0: a small case with the three
    terms and a map; batch 1: 4 x the test functions, the three terms and a map; batch 2: batch 1's data with a map and NO term.
    grad(0), grad(1), grad(2), grad(0), grad(1): repeated calls return the same bits, batches 0 and 1 meet their references, and
    batch 2's bits are those of an engine that never had a term registered."""
    i = IDS.index('mor6_q8')
    d_in, dim, widths, td = CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][10]
    big = big_batch(i)
    assert big['Input'].shape[0] == 4 * inputs(i)['Input'].shape[0]
    eng = new_engine(i)
    fresh = new_engine(i)
    try:
        register_interior(eng, i, 0)
        register_terms(eng, i, 'all', 0)
        register_map(eng, i, 0)
        for batch, variant in ((1, 'all'), (2, 'none')):
            register_interior(eng, i, batch, d=big)
            register_terms(eng, i, variant, batch, d=big)
            register_map(eng, i, batch, d=big)
        g = [grad_of(eng, b).copy() for b in (0, 1, 2, 0, 1)]
        assert np.array_equal(g[0], g[3]) and np.array_equal(g[1], g[4])
        assert not np.array_equal(g[1], g[2])
        ref_big = reference(i, 'all', d=big)
        g32_big = lambda: reference(i, 'all', dtype=torch.float32, d=big)[1]
        check_parity(i, eng, '%s/shared_buffers/batch1' % IDS[i], ref_big, g32_big, batch=1, rowwise_eval=True)
        check_parity(i, eng, '%s/shared_buffers/batch0' % IDS[i], reference64(i, 'all'),
                     lambda: reference(i, 'all', dtype=torch.float32)[1], batch=0, rowwise_eval=True)
        assert np.array_equal(grad_of(eng, 1), g[1])
        # nothing of s_eff leaks into the batch without a term
        register_interior(fresh, i, 0, d=big)
        register_map(fresh, i, 0, d=big)
        g_fresh = grad_of(fresh, 0)
        assert np.array_equal(g[2], g_fresh)
        assert np.array_equal(grad_of(eng, 2), g_fresh)
        out2, lv2 = eng.eval_loss(2, lossVec=True)
        outf, lvf = fresh.eval_loss(0, lossVec=True)
        assert out2 == outf and np.array_equal(lv2.cpu().numpy(), lvf.cpu().numpy())
        ref_none = reference(i, 'none', d=big)
        assert abs(g[2][eng.P] - ref_none[0]['loss']) <= LOSS_RTOL * abs(ref_none[0]['loss']) + 1e-7
        assert_grad_close(g[2][:eng.P], ref_none[1], d_in, widths, GRAD_RTOL, dim=dim, td=td, what='batch 2 (no term)',
                          g32=lambda: reference(i, 'none', dtype=torch.float32, d=big)[1])
    finally:
        eng.close()
        fresh.close()


def _theta_after(eng, state, fn):
    eng.import_state(state)
    fn()
    torch.cuda.synchronize()
    return eng.get_params()


def test_train_step_equals_grad_then_apply():
    """train_step folds the Adam update into the gradient reduction; grad + apply runs it as its own kernel.  Their relation is
    measured first on the de-duplicated batch without a term, then required to hold with the three terms
    (tests/test_nldiff_gpu.py measures it the same way on the row-wise routes)."""
    i = BENCH
    eng = new_engine(i)
    try:
        register_interior(eng, i)
        register_map(eng, i)
        s0 = eng.export_state()
        flat = eng.get_params()
        gap = []
        for with_terms in (False, True):
            if with_terms:
                register_terms(eng, i, 'all')
            a = _theta_after(eng, s0, lambda: eng.train_step(0))
            b = _theta_after(eng, s0, lambda: (eng.grad(0), eng.apply()))
            assert np.max(np.abs(a - flat)) > 1e-4                       # the step moved theta
            gap.append(float(np.max(np.abs(a - b))))
        RECORD['%s/train_step_vs_grad_apply' % IDS[i]] = {'without_terms': gap[0], 'with_terms': gap[1]}
        assert gap[1] <= max(2.0 * gap[0], 1e-6), gap
    finally:
        eng.close()


# ---- a real 2D+t grid through VarNet -----------------------------------------------------------------------------------
SQUARE = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
KAPPA, VEL = 0.8, [0.5, -0.3]
THETA_SCALE_2DT = 4.0


def w_fun(x, t=0):
    return np.hstack([1.0 + 0.5 * x[:, 0:1] + t, 0.5 - 0.4 * x[:, 1:2]])


def rate_fun(x, t=0):
    return 1.0 + 0.5 * x[:, 0:1] ** 2 + 0.3 * x[:, 1:2] + t


def pde_2dt():
    return ADPDE(PolygonDomain2D(SQUARE), diff=KAPPA, vel=VEL, tInterval=[0, 0.5], BCs=[[0.0, 1.0, 0.0]] * 4,
                 IC=lambda x: np.sin(pi * x[:, 0:1]) * np.sin(pi * x[:, 1:2]), nldiff=list(DIFF), reaction=(rate_fun, list(COEF)),
                 nlflux=(w_fun, list(FLUX)))


def varnet_reference(vn, td, with_d=True, dtype=torch.float64):
    """tests/nldiff_ref.py on the rows VarNet assembled (the method of tests/test_nldiff_gpu.py::_varnet_reference), with integW
    from the fixed data when the quadrature has weights."""
    fd, d = vn.fixData, td.mor[0]
    f = np.float64 if dtype == torch.float64 else np.float32
    Nr, dNxr, dNtr = fd.rows()                                   # (rounded to fp32 below: the engine's tables are fp32)
    cpu = lambda t: t.cpu().numpy().astype(f)
    col = lambda t: cpu(t).reshape(-1, 1)
    has_w = bool(vn.lossOpt['integWflag'])
    kw = dict(Input=cpu(d['Input']), gcoef=cpu(d['gcoef']), source=None if d['source'] is None else col(d['source']),
              N=Nr.astype(np.float32).astype(f), dNt=dNtr.astype(np.float32).astype(f),
              integW=np.reshape(fd.integW, (1, -1)).astype(np.float32).astype(f) if has_w else None, intShape=[fd.nt, fd.integNum],
              detJ=float(fd.detJ), detJvec=False, biInput=cpu(d['biInput']), biLabel=col(d['biLabel']), bDof=fd.bDofsum,
              biDimVal=float(fd.biDimVal), w=np.ones(3), dim=vn.dim, time_dependent=True, is_source=vn.lossOpt['isSource'],
              integWflag=has_w)
    nldiff = (col(d['psi']), DIFF if with_d else ONE)
    return nldiff_ref.loss_and_grad(vn.engine.get_params().astype(f), vn.inpDim, vn.layerWidth, nldiff, (col(d['phi']), FLUX),
                                    (col(d['rate']), COEF), dtype, **kw)


@pytest.mark.parametrize('integPnum', [2, 3], ids=['gauss2', 'gauss3'])
def test_2dt_grid_through_varnet(integPnum):
    """A real shared-point map on a uniform 2D+t grid (integ_num 64 and 216; interior quadrature points own 8 rows), built by
    VarNet with constant kappa and velocity, a variable flux field and reaction rate: enable_dedup keeps the registrations, gcoef is
    periodic (the table path; the same bits with the CSR-ordered copy), and the row-wise and the de-duplicated gradients and
    splitLoss agree with the reference."""
    vn = VarNet(pde_2dt(), layerWidth=[20, 20], discNum=[6, 5], bDiscNum=7, tDiscNum=5, integPnum=integPnum)
    eng = vn.engine
    tag = 'varnet_2dt_gauss%d' % integPnum
    dim = 2
    try:
        eng.set_params(THETA_SCALE_2DT * (eng.get_params() + 0.05 * np.random.default_rng(5).standard_normal(eng.P).astype(np.float32)))
        td = vn._build_tdata()
        td.select_mor(0)
        eng.set_weights([1.0, 1.0, 1.0])
        fd = vn.fixData
        assert fd.integNum == (64, 216)[integPnum - 2] and bool(vn.lossOpt['integWflag']) == (integPnum == 3)
        gc = td.mor[0]['gcoef'].cpu().numpy().reshape(fd.nt, fd.integNum, dim)
        assert np.array_equal(gc, np.broadcast_to(gc[0], gc.shape))           # constant kappa: gcoef repeats with period integ_num
        ref, gref = varnet_reference(vn, td)
        ref0, g0 = varnet_reference(vn, td, with_d=False)
        dl = abs(ref['varLoss'] - ref0['varLoss']) / abs(ref['varLoss'])
        blk = min(block_errors(g0, gref, vn.inpDim, vn.layerWidth, dim).values())
        print('dedup terms %s: D moves varLoss by %.3g and the least-moved gradient tensor by %.3g' % (tag, dl, blk))
        assert dl >= 100 * LOSS_RTOL and blk >= 100 * GRAD_RTOL, (dl, blk)       # (a condition on the inputs, from the reference)
        g32 = lambda: varnet_reference(vn, td, dtype=torch.float32)[1]
        P = eng.P
        lref = ref['lossVec'].reshape(-1)

        def check(g, what):
            rec = {'grad_' + k: _rel(g[P + n], ref[k]) for n, k in enumerate(KEYS)}
            out, lv = eng.eval_loss(0, lossVec=True)
            rec.update({'eval_' + k: _rel(out[n], ref[k]) for n, k in enumerate(KEYS)})
            rec['eval_lossVec'] = float(np.max(np.abs(lv.cpu().numpy().astype(np.float64) - lref)) / np.max(np.abs(lref)))
            RECORD['%s/%s' % (tag, what)] = rec
            try:
                for k in KEYS:
                    assert abs(rec['grad_' + k]) <= LOSS_RTOL + 1e-7 / max(abs(ref[k]), 1e-300), (what, 'grad', k, rec['grad_' + k])
                    assert abs(rec['eval_' + k]) <= LOSS_RTOL + 1e-7 / max(abs(ref[k]), 1e-300), (what, 'eval', k, rec['eval_' + k])
                assert rec['eval_lossVec'] <= LVEC_RTOL, (what, rec['eval_lossVec'])
                assert_grad_close(g[:P], gref, vn.inpDim, vn.layerWidth, GRAD_RTOL, dim=dim, what='%s %s' % (tag, what), g32=g32, rec=rec)
            finally:
                print('dedup terms %s/%s: %s' % (tag, what, json.dumps(rec, sort_keys=True)))

        g_row = grad_of(eng)
        check(g_row, 'rowwise')
        U = td.enable_dedup()
        assert td.dedup_reason is None and 0 < U < fd.nT / 2, (td.dedup_reason, U)
        rowptr = td._dd_cache[(0, 0)][2]
        counts = np.diff(rowptr.cpu().numpy() if isinstance(rowptr, torch.Tensor) else np.asarray(rowptr))
        hist = np.bincount(counts)
        print('dedup terms %s: %d unique points of %d rows, rows per point %s' % (tag, U, fd.nT, hist.tolist()))
        assert counts.max() == 8 and hist[8] >= integPnum ** 3             # interior points: 2^3 test functions share them
        g1 = grad_of(eng)
        assert np.array_equal(g1, grad_of(eng)) and not np.array_equal(g1, g_row)
        check(g1, 'dedup')
        dev32 = lambda: fp32_deviation(g32(), gref, vn.inpDim, vn.layerWidth, dim)
        RECORD[tag + '/dedup_vs_rowwise'] = assert_pair_close(g1, g_row, vn.inpDim, vn.layerWidth, GRAD_RTOL, dim=dim, dev32=dev32,
                                                               what=tag + ' dedup vs row-wise')
        comp, _, _ = vn.splitLoss(td)                                    # the monitor's loss split sees the three terms
        assert abs(comp[2, 0] - ref['varLoss']) <= LOSS_RTOL * abs(ref['varLoss']) + 1e-7
        # the periodic table was one choice of two: the CSR-ordered copy of gcoef gives the same bits
        eng.debug_point_route(4)
        try:
            td.enable_dedup()
        finally:
            eng.debug_point_route(0)
        assert np.array_equal(grad_of(eng), g1)
        td.disable_dedup()
        assert np.array_equal(grad_of(eng), g_row)                       # ... and the row-wise step is back, with the terms
    finally:
        eng.close()
