"""
CPU tier of the parity tests of the nonlinear terms on shared-point de-duplication maps (tests/test_dedup_terms_gpu.py): the
condition on the inputs of tests/dedup_term_cases.py (each term alone moves every compared quantity by at least 100 x its bar,
each term left out of 'all' by at least 10 x), the map builder, and the reference on the expanded rows against the oracle.
"""
import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests.dedup_term_cases import (ALONE, CASES, EMPTY, IDS, LEFT_OUT, ONE, VARIANTS, csr, empty_map, inputs, ref_kw, reference64,
                                    theta)
from tests import nldiff_ref
from tests.gradcheck import block_errors
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL

CASE_IDS = range(len(CASES))


def moved(i, with_term, without):
    """How far leaving a term out moves what the parity tests compare, each on the scale its bar uses: (loss, varLoss, lossVec,
    least-moved parameter tensor of the gradient) -- the rule of tests/test_nldiff_host.py."""
    (ra, ga), (rb, gb) = reference64(i, with_term), reference64(i, without)
    lv = np.max(np.abs(ra['lossVec'] - rb['lossVec'])) / np.max(np.abs(ra['lossVec']))
    blocks = block_errors(gb, ga, CASES[i][0], CASES[i][2], CASES[i][1], CASES[i][10])
    return (abs(ra['loss'] - rb['loss']) / abs(ra['loss']), abs(ra['varLoss'] - rb['varLoss']) / abs(ra['varLoss']), float(lv),
            min(blocks.values()))


# ---- the inputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', CASE_IDS, ids=IDS)
def test_inputs_make_a_missing_term_fail(i):
    """A condition on the INPUTS, from the fp64 reference alone (no engine, no tolerance of one).  Each of D, psi, the flux and the
    reaction alone, against no term, moves the loss and varLoss by >= 100 LOSS_RTOL, lossVec by >= 100 LVEC_RTOL of its maximum
    and EVERY parameter tensor of the gradient by >= 100 GRAD_RTOL of its own size; in 'all', leaving any one of the four out
    moves the same quantities by >= 10 x their bars.  (BCloss and ICloss do not contain the interior rows.)"""
    for alone in ALONE:
        dl, dv, lv, blk = moved(i, alone, 'none')
        print('dedup terms inputs %s, %s alone: loss %.3g varLoss %.3g lossVec %.3g least-moved gradient tensor %.3g'
              % (IDS[i], alone, dl, dv, lv, blk))
        assert dl >= 100 * LOSS_RTOL and dv >= 100 * LOSS_RTOL, (alone, dl, dv)
        assert lv >= 100 * LVEC_RTOL, (alone, lv)
        assert blk >= 100 * GRAD_RTOL, (alone, blk)
    for out in LEFT_OUT:
        dl, dv, lv, blk = moved(i, 'all', out)
        print('dedup terms inputs %s, %s: loss %.3g varLoss %.3g lossVec %.3g least-moved gradient tensor %.3g'
              % (IDS[i], out, dl, dv, lv, blk))
        assert dl >= 10 * LOSS_RTOL and dv >= 10 * LOSS_RTOL, (out, dl, dv)
        assert lv >= 10 * LVEC_RTOL, (out, lv)
        assert blk >= 10 * GRAD_RTOL, (out, blk)


@pytest.mark.parametrize('i', CASE_IDS, ids=IDS)
def test_table_has_no_zero_entry_and_streams_are_fp32(i):
    """The term folds of the de-duplicated step divide by N_p (a zero entry is an error code, not a case of these tests); every
    registered stream is fp32 and has one entry per row; a periodic case repeats its gcoef bitwise with period integ_num."""
    q, n_k, periodic = CASES[i][3], CASES[i][4], CASES[i][12]
    d = inputs(i)
    assert np.all(d['N1'] >= np.float32(0.1))
    for k in ('rate', 'phi', 'psi'):
        assert d[k].dtype == np.float32 and d[k].shape == (n_k * q, 1)
    g = d['gcoef'].reshape(n_k, q, -1)
    assert np.array_equal(g, np.broadcast_to(g[0], g.shape)) == bool(periodic)


# ---- the map --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', CASE_IDS, ids=IDS)
def test_map_builder(i):
    q, n_k, U, dim = CASES[i][3], CASES[i][4], CASES[i][5], CASES[i][1]
    d = inputs(i)
    uid, rowptr, rowidx = d['uid'], d['rowptr'], d['rowidx']
    nT = n_k * q
    assert rowptr.dtype == np.int32 and rowidx.dtype == np.int32
    assert rowptr.shape == (U + 1,) and rowidx.shape == (nT,) and uid.shape == (nT,)
    assert rowptr[0] == 0 and rowptr[U] == nT and np.all(np.diff(rowptr) >= 0)
    assert np.array_equal(np.sort(rowidx), np.arange(nT))                       # every row once
    owner = np.repeat(np.arange(U), np.diff(rowptr))                            # the point whose segment holds e
    assert np.array_equal(uid[rowidx], owner)
    for j in range(U):
        seg = rowidx[rowptr[j]:rowptr[j + 1]]
        assert np.all(np.diff(seg) > 0), j                                      # rows of a point in increasing order
    assert np.array_equal(d['Input'], d['Xu'][uid])
    # the segment lengths the four-in-flight loops of the gather kernels see: every tail, and more than two passes
    counts = np.diff(rowptr)
    hist = np.bincount(counts)
    print('dedup terms map %s: rows per point %s' % (IDS[i], hist.tolist()))
    assert counts.min() >= 1                                                    # every point is used
    for c in range(1, 8):
        assert hist[c] > 0, (c, hist.tolist())
    if dim >= 2:
        assert counts.max() >= 8, hist.tolist()


def test_csr_on_a_small_map():
    uid = np.array([2, 0, 2, 4, 0, 2], dtype=np.int32)
    rowptr, rowidx = csr(uid, 6)
    assert rowptr.tolist() == [0, 2, 2, 5, 5, 6, 6]
    assert rowidx.tolist() == [1, 4, 0, 2, 5, 3]


@pytest.mark.parametrize('i', EMPTY, ids=[IDS[k] for k in EMPTY])
def test_empty_point_map(i):
    """The variant map: the appended points, and only they, own no row; everything else is the case's own map."""
    d = inputs(i)
    U = CASES[i][5]
    Xu, rowptr = empty_map(i)
    extra = Xu.shape[0] - U
    assert 0.04 * U <= extra <= 0.06 * U
    assert rowptr.dtype == np.int32 and rowptr.shape == (U + extra + 1,)
    assert np.array_equal(Xu[:U], d['Xu']) and np.array_equal(rowptr[:U + 1], d['rowptr'])
    counts = np.diff(rowptr)
    assert np.all(counts[:U] >= 1) and np.all(counts[U:] == 0)
    assert rowptr[-1] == d['uid'].size
    assert d['uid'].max() < U
    assert np.all(np.abs(Xu[U:]) <= 1) and Xu.dtype == np.float32


# ---- the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', CASE_IDS, ids=IDS)
def test_reference_without_a_term_is_the_oracle_exactly(i):
    """D = (1, 0, 0), psi = None, no flux and no reaction: the reference on Xu[uid] is the oracle's, bit for bit -- through the
    chain of references ('none') and through nldiff_ref's own loss function."""
    d_in, widths = CASES[i][0], CASES[i][2]
    flat = theta(i).astype(np.float64)
    ref, g = og.loss_and_grad(flat, d_in, widths, torch.float64, **ref_kw(i))
    for got, gg in (reference64(i, 'none'), nldiff_ref.loss_and_grad(flat, d_in, widths, (None, ONE), None, None, torch.float64,
                                                                     **ref_kw(i))):
        for k in ('loss', 'BCloss', 'ICloss', 'varLoss'):
            assert got[k] == ref[k], (k, got[k], ref[k])
        assert np.array_equal(got['lossVec'], ref['lossVec'])
        assert np.array_equal(gg, g)
    if not CASES[i][10]:
        assert ref['ICloss'] == 0.0


@pytest.mark.parametrize('i', CASE_IDS, ids=IDS)
def test_reference_gradients_are_finite(i):
    for variant in VARIANTS + LEFT_OUT + ['none']:
        ref, g = reference64(i, variant)
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(ref['lossVec'])) and np.isfinite(ref['loss']), variant
