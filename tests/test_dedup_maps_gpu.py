"""
GPU tier: the de-duplicated step on heavily shared and skewed point maps (tests/dedup_map_cases.py).  Every other map of the suite
keeps a 256-point block of vn_dedup_gather_kernel inside one LDS chunk of VN_GATHER_CH entries and a point of csr_walk
(vn_terms.hip) at 20 rows or fewer (tests/test_dedup_maps_host.py asserts the former); here the chunk loop runs up to five times,
segments are cut by chunk boundaries, end exactly on them and span several chunks, whole blocks own no row, and the gathers of the
three nonlinear terms walk segments of 16 to more than 5000 rows.

Per map, the checks of tests/test_engine_gpu.py::dedup_checks: the row-wise and the de-duplicated step against the fp64 oracle on
the expanded rows at LOSS_RTOL / GRAD_RTOL, per block with the fp32 oracle as conditioning, de-duplicated against row-wise at 2e-4,
eval_loss with lossVec on the map and row-wise, a second grad bit-identical, the map cleared restoring the row-wise bits.  The
periodic table against the CSR-ordered copy bit for bit on maps of two and four chunks (the only check of the gcoef_csr offsets of
a later chunk on a periodic batch); the three terms together at the bars of tests/test_dedup_terms_gpu.py; a small batch's bits
unchanged by a larger batch registered and run in between.  No bar is new.

The errors per case are written to dedup_maps_parity.json in the directory VN_RECORD_DIR names (default: profile_out/ beside
tests/; the committed copy: profiles/dedup_maps_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import dedup_map_cases as mc
from tests.dedup_map_cases import BIDIMVAL, DETJ, inputs
from tests.gradcheck import assert_pair_close, fp32_deviation
from tests.parity_cases import GRAD_RTOL
from tests.test_dedup_terms_gpu import check_parity, grad_of
from tests.test_engine_gpu import dedup_checks
from varnet_amd.engine import VNEngine

pytestmark = pytest.mark.gpu

RECORD = {}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'dedup_maps_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def new_engine(name, terms=False):
    """An engine of a case with its parameters; no table, no batch yet."""
    d_in, dim, widths, q, act, source, integW = mc.config(name)[:7]
    eng = VNEngine(dim, d_in, widths, True, q, isSource=source, integWflag=integW, activationFun=act)
    eng.set_params(mc.theta(name, terms))
    return eng


def set_tables(eng, name):
    d = inputs(name)
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_bic(d['biInput'], d['biLabel'], d['bDof'], BIDIMVAL)
    eng.set_weights(d['w'])


def set_batch(eng, name, batch=0, gcoef='gcoef', route=0):
    """The interior rows of a case and its map (route 4: vn_set_dedup keeps the CSR-ordered copy of a periodic gcoef)."""
    d = inputs(name)
    eng.set_interior(batch, d['Input'], d[gcoef], d['source'], n_k=d['n_k'], detJ=DETJ)
    eng.debug_point_route(route)
    try:
        eng.set_dedup(batch, d['Xu'], d['uid'], d['rowptr'], d['rowidx'])
    finally:
        eng.debug_point_route(0)


def describe(name):
    d = inputs(name)
    be = mc.block_entries(d['rowptr'])
    return dict(rows=int(d['uid'].size), points=int(d['Xu'].shape[0]), integ_num=int(mc.config(name)[3]),
                largest_block=int(be.max()), chunks=int(-(-be.max() // mc.CH)), longest_segment=int(np.diff(d['rowptr']).max()))


@pytest.mark.parametrize('name', mc.IDS + mc.SWEEP_IDS)
def test_map_parity(name):
    """Every map of the table and every draw of the sweep under the checks of dedup_checks."""
    eng = new_engine(name)
    RECORD[name + '/map'] = describe(name)
    try:
        dedup_checks(eng, inputs(name), True, tag=name, act=mc.config(name)[4], oracle=lambda dt: mc.oracle(name, dt), errors=RECORD)
    finally:
        print('dedup maps %s: %s %s' % (name, json.dumps(RECORD[name + '/map'], sort_keys=True), json.dumps(RECORD.get(name), sort_keys=True)))
        eng.close()


@pytest.mark.parametrize('name', mc.BITWISE)
def test_periodic_table_is_bitwise_the_csr_path(name):
    """A periodic gcoef is read as an integ_num-entry table; debug_point_route(4) at vn_set_dedup keeps the CSR-ordered copy, which
    the gather kernel indexes by base + position in the chunk: the same gradient bits and eval_loss numbers on blocks of two
    (grid_3dt) and four (dense) chunks."""
    assert name in mc.PERIODIC and describe(name)['chunks'] >= 2
    eng = new_engine(name)
    try:
        set_tables(eng, name)

        def run(route):
            set_batch(eng, name, route=route)
            out, lv = eng.eval_loss(0, lossVec=True)
            return grad_of(eng), out, lv.cpu().numpy()
        g_tab, out_tab, lv_tab = run(0)
        g_csr, out_csr, lv_csr = run(4)
        ref, gref = mc.oracle(name)
        P = eng.P
        err = {k: float(np.max(np.abs(g[:P] - gref)) / np.max(np.abs(gref))) for k, g in (('table', g_tab), ('csr', g_csr))}
        RECORD[name + '/table_vs_csr'] = dict(err, bitwise=bool(np.array_equal(g_tab, g_csr)))
        print('dedup maps %s table vs CSR-ordered copy: %s' % (name, json.dumps(RECORD[name + '/table_vs_csr'], sort_keys=True)))
        assert np.array_equal(g_tab, g_csr)
        assert out_tab == out_csr and np.array_equal(lv_tab, lv_csr)
        assert err['csr'] <= GRAD_RTOL                                   # (and not two equal wrong answers)
    finally:
        eng.close()


@pytest.mark.parametrize('name', mc.TERM_CASES)
def test_three_terms_on_long_segments(name):
    """D(u) with psi, the flux and the reaction together (variant 'all' of tests/dedup_term_cases.py) on points of 16 rows
    (grid_3dt), 16..19 rows (long_tails) and more than 5000 rows (hot_point): the gathers of vn_terms.hip (csr_walk) against
    tests/nldiff_ref.py on the expanded rows, with the checks of tests/test_dedup_terms_gpu.py::both_routes."""
    net = mc.net_of(name)
    d_in, dim, widths, td = net
    eng = new_engine(name, terms=True)
    try:
        set_tables(eng, name)
        d = inputs(name)
        eng.set_interior(0, d['Input'], d['gcoef_terms'], d['source'], n_k=d['n_k'], detJ=DETJ)
        nldiff, nlflux, reaction = mc.terms_of(name, 'all')
        eng.set_reaction(0, *reaction)
        eng.set_nlflux(0, *nlflux)
        eng.set_nldiff(0, *nldiff)
        eng.set_dedup(0, d['Xu'], d['uid'], d['rowptr'], d['rowidx'])
        ref = mc.terms_reference(name)
        g32 = lambda: mc.terms_reference(name, 'all', torch.float32)[1]
        tag = name + '/terms'
        g_dd = check_parity(None, eng, tag + '/dedup', ref, g32, rowwise_eval=True, net=net, record=RECORD)
        assert np.array_equal(g_dd, grad_of(eng))                       # two de-duplicated calls: the same bits
        eng.set_dedup(0)                                                # the terms stay; the batch is row-wise again
        g_row = check_parity(None, eng, tag + '/rowwise', ref, g32, net=net, record=RECORD)
        assert not np.array_equal(g_dd, g_row)                          # another formulation ran
        dev32 = lambda: fp32_deviation(g32(), ref[1], d_in, widths, dim, td)
        RECORD[tag + '/dedup_vs_rowwise'] = assert_pair_close(g_dd, g_row, d_in, widths, GRAD_RTOL, dim=dim, td=td, dev32=dev32,
                                                              what=tag + ' dedup vs row-wise')
    finally:
        eng.close()


def test_small_batch_keeps_its_bits_after_a_larger_one():
    """The (u, grad u) records and the seeds of the unique points live in engine-level buffers that vn_set_dedup grows: batch 0 =
    grid_3dt_small (4096 points), batch 1 = grid_3dt (10 000 points, two-chunk blocks) registered after it.  grad(1), then grad(0):
    batch 0 gives the bits it gives on an engine of its own; batch 1 repeats its bits and agrees with its row-wise step."""
    small, big = 'grid_3dt_small', 'grid_3dt'
    d_in, dim, widths, td = mc.net_of(small)
    assert mc.config(small)[:7] == mc.config(big)[:7]                    # one network, one integ_num: two batches of one engine
    alone, eng = new_engine(small), new_engine(small)
    try:
        set_tables(alone, small)
        set_batch(alone, small)
        g_alone = grad_of(alone)
        set_tables(eng, small)
        set_batch(eng, small, 0)
        set_batch(eng, big, 1)
        g1 = grad_of(eng, 1).copy()
        g0 = grad_of(eng, 0).copy()
        assert np.array_equal(g0, g_alone)
        assert np.array_equal(grad_of(eng, 1), g1) and not np.array_equal(g1, g0)
        assert np.array_equal(grad_of(eng, 0), g_alone)
        eng.set_dedup(1)
        RECORD['batch_order/batch1_dedup_vs_rowwise'] = assert_pair_close(g1, grad_of(eng, 1), d_in, widths, 2e-4, dim=dim, td=td,
                                                                          what='batch 1 dedup vs row-wise')
        assert np.array_equal(grad_of(eng, 0), g_alone)
    finally:
        alone.close()
        eng.close()
