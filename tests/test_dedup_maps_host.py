"""
CPU tier of the parity tests of the de-duplicated step on heavily shared and skewed point maps (tests/test_dedup_maps_gpu.py): from
rowptr and the two constants of vn_dedup_gather_kernel, the property every map of tests/dedup_map_cases.py exists for; that every
OTHER map of the suite stays inside one LDS chunk (so that the statement "only these cases reach the chunk loop" stays true); and
the conditioning of every case: the fp32 oracle within a tenth of the bars of the fp64 oracle.
"""
import numpy as np
import pytest
import torch

from tests import dedup_map_cases as mc
from tests import dedup_term_cases as tc
from tests import fuzz_routes as fz
from tests.dedup_map_cases import CH, PB, block_entries, inputs
from tests.gradcheck import block_errors
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL

ALL = mc.IDS + mc.SWEEP_IDS


def chunks(rowptr):
    """Passes of the chunk loop per block: ceil(entries / CH)."""
    return -(-block_entries(rowptr) // CH)


def cut_segments(rowptr, block=0):
    """(segments cut by a chunk boundary, segments longer than a whole chunk, chunk boundaries that fall exactly between two
    segments) of one block; boundaries at e0 + m CH inside (e0, e1)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    j0, j1 = block * PB, min((block + 1) * PB, rowptr.size - 1)
    e0, e1 = rowptr[j0], rowptr[j1]
    s0, s1 = rowptr[j0:j1], rowptr[j0 + 1:j1 + 1]
    cut = between = 0
    for b in range(e0 + CH, e1, CH):
        cut += int(np.sum((s0 < b) & (b < s1)))
        between += int(np.any((s1 == b) & (s1 > s0)) and not np.any((s0 < b) & (b < s1)))
    return cut, int(np.sum(s1 - s0 > CH)), between


# ---- the constants and the maps -------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    """The two constants come out of vn_dedup.hip; the LDS buffer and the row-pointer table are declared with them, and the
    kernel's 256 threads cover a block's points one each."""
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'varnet_amd', 'csrc', 'vn_dedup.hip')
    text = open(path).read()
    assert 'float sp[VN_GATHER_CH][4]' in text and 'int sptr[VN_GATHER_PB + 1]' in text
    assert (PB, CH) == mc.gather_constants() and PB == 256 and CH > PB


@pytest.mark.parametrize('name', ALL)
def test_map_is_valid(name):
    """Every map is a consistent one (the rules of vn_dedup_check_kernel): nothing here may be refused or fault."""
    d = inputs(name)
    uid, rowptr, rowidx = d['uid'], d['rowptr'], d['rowidx']
    U, nT = d['Xu'].shape[0], uid.size
    assert nT == d['n_k'] * mc.config(name)[3] and nT <= 65536
    assert uid.dtype == np.int32 and rowptr.dtype == np.int32 and rowidx.dtype == np.int32
    assert uid.min() >= 0 and uid.max() < U
    assert rowptr.shape == (U + 1,) and rowptr[0] == 0 and rowptr[U] == nT and np.all(np.diff(rowptr) >= 0)
    assert np.array_equal(np.sort(rowidx), np.arange(nT))
    assert np.array_equal(uid[rowidx], np.repeat(np.arange(U), np.diff(rowptr)))
    inner = np.ones(nT, dtype=bool)
    inner[rowptr[:-1][np.diff(rowptr) > 0]] = False                        # first entry of every segment
    assert np.all(np.diff(rowidx)[inner[1:]] > 0)                          # rows of a point in increasing order
    assert np.array_equal(d['Input'], d['Xu'][uid])
    g = d['gcoef'].reshape(d['n_k'], -1, d['gcoef'].shape[1])
    assert np.array_equal(g, np.broadcast_to(g[0], g.shape)) == bool(mc.config(name)[7]) or d['n_k'] == 1
    assert np.all(d['N1'] >= np.float32(0.1))


def test_grid_maps():
    """The geometry: 4 axes with `nodes` hat functions each, integ_num 4^4; interior points shared by 2^4 test functions."""
    for name, nodes, rows, U, largest in (('grid_3dt', 4, 65536, 10000, 2768), ('grid_3dt_small', 3, 20736, 4096, 1728)):
        d = inputs(name)
        counts = np.diff(d['rowptr'])
        assert mc.config(name)[3] == 256 and d['n_k'] == nodes ** 4 and d['uid'].size == rows and d['Xu'].shape[0] == U
        hist = np.bincount(counts)
        assert counts.min() == 1 and counts.max() == 16 and set(np.flatnonzero(hist)) == {1, 2, 4, 8, 16}
        assert hist[16] == (2 * (nodes - 1)) ** 4 and hist[1] == 4 ** 4         # per axis: 2 (nodes - 1) shared points, 4 not
        assert block_entries(d['rowptr']).max() == largest
    # a test function's 256 points are 4 consecutive points on each axis, starting at twice its node index
    uid = inputs('grid_3dt')['uid'].reshape(256, 256)
    assert uid[0, 0] == 0 and uid[0, 1] == 1 and uid[0, 4] == 10 and uid[1, 0] == 2 and uid[4, 0] == 20 and uid[-1, -1] == 9999
    ch = chunks(inputs('grid_3dt')['rowptr'])
    assert ch.max() == 2 and np.sum(ch == 1) > 0 and np.sum(ch == 2) > 0          # blocks of one and of two chunks
    assert chunks(inputs('grid_3dt_small')['rowptr']).max() == 1                  # the control never re-enters the loop


def test_hot_single_dense():
    rp = inputs('hot_point')['rowptr']
    counts = np.diff(rp)
    assert rp[-1] == 7680 and counts.size == 300 and counts.min() >= 1
    assert counts.max() >= 0.65 * 7680 and counts.max() > 2 * CH                  # one segment longer than two whole chunks
    assert chunks(rp)[0] == 4 and int(np.argmax(counts)) < PB
    cut, longer, _ = cut_segments(rp)
    assert cut >= 1 and longer == 1
    rp = inputs('single_point')['rowptr']
    assert rp.tolist() == [0, 7680] and chunks(rp).tolist() == [4]
    rp = inputs('dense')['rowptr']
    counts = np.diff(rp)
    assert counts.size == 40 and 150 <= counts.min() and counts.max() <= 240 and chunks(rp).tolist() == [4]
    assert cut_segments(rp) == (3, 0, 0)                                          # every chunk boundary cuts a segment


def test_chunk_edges():
    want = {'edge_ch': CH, 'edge_ch1': CH + 1, 'edge_2ch': 2 * CH, 'edge_between': CH + 700}
    for name, entries in want.items():
        rp = inputs(name)['rowptr']
        be = block_entries(rp)
        assert be[0] == entries and be.size == 2 and 0 < be[1] <= CH, (name, be)
        assert np.diff(rp)[:PB].min() >= 1
    assert chunks(inputs('edge_ch')['rowptr'])[0] == 1                            # n == CH, the loop ends after one pass
    assert chunks(inputs('edge_ch1')['rowptr'])[0] == 2                           # a last chunk of one entry
    assert chunks(inputs('edge_2ch')['rowptr'])[0] == 2                           # n == CH on both passes
    rp = inputs('edge_between')['rowptr']
    assert CH in rp[:PB + 1].tolist() and cut_segments(rp) == (0, 0, 1)           # hi == lo for the segment that ends at CH
    for name in ('edge_ch1', 'edge_2ch'):
        assert cut_segments(inputs(name)['rowptr'])[1] == 0


def test_empty_blocks():
    rp = inputs('empty_blocks')['rowptr']
    counts = np.diff(rp)
    U = counts.size
    be = block_entries(rp)
    assert U > 2 * PB and be.size == 3 and be[1] == 0 and be[0] > 0 and be[2] > 0 and be.max() <= CH
    assert np.all(counts[PB:2 * PB] == 0)                                         # e0 == e1: a block that owns no row
    for j in (0, PB - 1, 2 * PB, U - 1):
        assert counts[j] == 0
    assert np.all(counts[1:PB - 1] >= 1) and np.all(counts[2 * PB + 1:U - 1] >= 1)


def test_long_tails():
    """csr_walk: four entries per pass; 16..19 rows are four full passes plus every tail (0, 1, 2, 3 entries in a fifth)."""
    counts = np.diff(inputs('long_tails')['rowptr'])
    hist = np.bincount(counts, minlength=20)
    for c in (16, 17, 18, 19):
        assert hist[c] == 3
    assert counts.max() == 19 and counts.min() >= 1 and all(hist[c] > 0 for c in range(1, 10))
    assert block_entries(inputs('long_tails')['rowptr']).max() <= CH
    for name in mc.TERM_CASES:
        assert np.diff(inputs(name)['rowptr']).max() >= 16
    assert np.diff(inputs('hot_point')['rowptr']).max() > 5000


def test_sweep_draws():
    """12 draws, integ_num from {16, 36, 64, 256}, at most 20 000 rows, odd seeds Zipf-distributed; most of them enter the chunk
    loop a second time."""
    assert len(mc.SWEEP_SEEDS) == 12 and len(set(mc.SWEEP_SEEDS)) == 12
    multi = 0
    qs = set()
    for s in mc.SWEEP_SEEDS:
        q, uid, U = mc.sweep_map(s)
        rp = inputs('sweep%d' % s)['rowptr']
        assert q in (16, 36, 64, 256) and uid.size <= 20000 and 1 <= uid.size // U <= 40
        if s % 2:
            assert np.diff(rp).max() >= 10 * uid.size / U                         # a few points own most rows
        multi += int(chunks(rp).max() >= 2)
        qs.add(q)
    print('dedup maps sweep: %d of 12 draws with a block of two or more chunks, integ_num %s' % (multi, sorted(qs)))
    assert multi >= 6 and len(qs) >= 3


# ---- every other map of the suite stays inside one chunk ----------------------------------------------------------------
def largest_block(uid, U):
    rowptr = np.zeros(U + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(uid, minlength=U))
    return int(block_entries(rowptr).max())


def test_the_suites_other_maps_stay_inside_one_chunk():
    """The hand cases of tests/test_engine_gpu.py (time-dependent and steady; also the map of its periodic-table test), the maps
    of tests/dedup_term_cases.py (with its larger batch), the map draws of tests/fuzz_routes.py (seeds 0..39 x 30 cases, whether or
    not a draw can run de-duplicated) and a uniform 2D+t grid (8 rows per point) never own more than CH entries in one block."""
    from tests import test_engine_gpu as te
    worst = {}
    hand = 0
    for case in te.DEDUP_CASES + te.DEDUP_STEADY:
        q, n_k, U = case[3], case[4], case[5]
        rng = np.random.default_rng(21)
        rng.uniform(-1, 1, (U, case[0]))
        uid = rng.integers(0, U, n_k * q)
        uid[:U] = np.arange(U)
        rng.shuffle(uid)
        hand = max(hand, largest_block(uid, U))
    worst['hand cases'] = hand
    worst['term cases'] = max(max(int(block_entries(tc.inputs(i)['rowptr']).max()) for i in range(len(tc.CASES))),
                              int(block_entries(tc.big_batch(tc.IDS.index('mor6_q8'))['rowptr']).max()))
    fuzz = 0
    for seed in range(40):
        rng = np.random.default_rng(seed)
        for case in range(30):
            c = fz.draw_case(rng, case)
            if c['q'] > 256:
                continue
            n = (c['n_k'] if c['big'] else min(c['n_k'], 40)) * c['q']
            r5 = np.random.default_rng(5000 + case)
            U = max(1, n // int(r5.integers(1, 9)))
            uid = r5.integers(0, U, n)
            uid[:U] = np.arange(U)
            fuzz = max(fuzz, largest_block(uid, U))
    worst['fuzz draws'] = fuzz
    uid, U = mc.grid_map(6, axes=3)
    assert np.bincount(uid).max() == 8 and 8 * PB <= CH                           # any 2D+t grid: at most 8 rows on each of 256 points
    worst['2D+t grid'] = largest_block(uid, U)
    worst['control'] = int(block_entries(inputs(mc.CONTROL)['rowptr']).max())
    print('dedup maps: largest block of the other maps of the suite %s (CH = %d)' % (worst, CH))
    for what, entries in worst.items():
        assert entries <= CH, (what, entries)


# ---- conditioning ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL)
def test_fp32_oracle_is_within_a_tenth_of_the_bars(name):
    """A condition on the inputs, not a measurement of the engine: the oracle's own fp32 evaluation on the expanded rows deviates
    from its fp64 evaluation by at most LOSS_RTOL / 10 on the loss and GRAD_RTOL / 10 on the gradient (|.|_inf over |g|_inf, the
    norm of the bar).  A case that misses gets another seed, never another bar.  Measured with these inputs: at most 4.4e-7 on
    the loss (sweep1) and 2.2e-6 on the gradient (hot_point)."""
    d_in, dim, widths = mc.config(name)[:3]
    (r64, g64), (r32, g32) = mc.oracle(name), mc.oracle(name, torch.float32)
    dl = abs(r32['loss'] - r64['loss']) / abs(r64['loss'])
    dg = float(np.max(np.abs(g32 - g64)) / np.max(np.abs(g64)))
    blk = max(block_errors(g32, g64, d_in, widths, dim, True).values())
    print('dedup maps conditioning %s: fp32 oracle loss %.3g gradient %.3g worst block %.3g' % (name, dl, dg, blk))
    assert np.all(np.isfinite(g64)) and np.isfinite(r64['loss'])
    assert dl <= LOSS_RTOL / 10 and dg <= GRAD_RTOL / 10, (name, dl, dg)


@pytest.mark.parametrize('name', mc.TERM_CASES)
def test_terms_matter_on_the_term_cases(name):
    """With the three terms registered, leaving any one of D, psi, the flux and the reaction out moves the loss, lossVec and every
    parameter tensor of the gradient by at least 10 x its bar (the rule of tests/test_dedup_terms_host.py), and the fp32 reference
    stays within a tenth of the bars: a gather of a term that dropped rows cannot hide below the bars."""
    d_in, dim, widths = mc.config(name)[:3]
    ra, ga = mc.terms_reference(name, 'all')
    for out in ('no_d', 'no_psi', 'no_flux', 'no_react'):
        rb, gb = mc.terms_reference(name, out)
        dl = abs(ra['loss'] - rb['loss']) / abs(ra['loss'])
        lv = float(np.max(np.abs(ra['lossVec'] - rb['lossVec'])) / np.max(np.abs(ra['lossVec'])))
        blk = min(block_errors(gb, ga, d_in, widths, dim, True).values())
        print('dedup maps terms %s, %s: loss %.3g lossVec %.3g least-moved gradient tensor %.3g' % (name, out, dl, lv, blk))
        assert dl >= 10 * LOSS_RTOL and lv >= 10 * LVEC_RTOL and blk >= 10 * GRAD_RTOL, (out, dl, lv, blk)
    r32, g32 = mc.terms_reference(name, 'all', torch.float32)
    dl = abs(r32['loss'] - ra['loss']) / abs(ra['loss'])
    dg = float(np.max(np.abs(g32 - ga)) / np.max(np.abs(ga)))
    print('dedup maps terms conditioning %s: fp32 reference loss %.3g gradient %.3g' % (name, dl, dg))
    assert dl <= LOSS_RTOL / 10 and dg <= GRAD_RTOL / 10, (name, dl, dg)
