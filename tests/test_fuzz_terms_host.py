"""
CPU tier of the nonlinear-term fuzz (tests/fuzz_terms.py): conditions on the committed seed lists that keep the GPU tier
(tests/test_fuzz_terms_gpu.py) honest, checked from the fp64 reference alone for exactly the cases the GPU tier runs -- the
reference reduces to the oracle without terms, every drawn term moves the gradient by at least 10 x the bar the case is judged
at (a route that forgets it fails), the fp32-conditioning whitelist is the exception, no case is left out, and the lists reach
the one-row forms of the elementwise kernels, every sub-form of the layer-by-layer route, the deep fused nets, integ_num beyond
one tile, wide inputs, steady problems with a flux term and with D(u), and boundary-flux rows on nets that take them.
"""
import functools
import time

import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests import fuzz_routes as fz
from tests import fuzz_terms as ft

IDS = ['%s%s%d' % ('steady' if st else 'td', '_mor' if mor else '', seed) for seed, n, st, mor in ft.SEED_LISTS]


@functools.lru_cache(maxsize=None)
def cases(k):
    return ft.draw_list(*ft.SEED_LISTS[k])


@functools.lru_cache(maxsize=None)
def evaluated(k):
    """[(case, inputs, theta, (result, gradient) in fp64, seconds)] of list k: computed once, shared, never modified."""
    out = []
    for c in cases(k):
        d, _ = ft.case_inputs(c)
        flat = ft.theta(c)
        t0 = time.perf_counter()
        ref = ft.reference(c, d, flat)
        out.append((c, d, flat, ref, time.perf_counter() - t0))
    return out


def test_the_draw_sequence_of_fuzz_routes_is_kept():
    """A seed names the same net, inputs and flags as in tests/fuzz_routes.py; only the sizes are cut (n_k <= 40, n_k * q <=
    20 000, a block-crossing draw replaces q and n_k) and nothing is left out: every list holds its cases 0..n-1."""
    for k, (seed, n, steady, mor) in enumerate(ft.SEED_LISTS):
        assert n <= 8
        rng = np.random.default_rng(seed)
        got = cases(k)
        assert [c['case'] for c in got] == list(range(n))
        for c in got:
            base = fz.draw_case(rng, c['case'], steady=steady, mor=mor)
            for key in ('L', 'act', 'widths', 'dim', 'd_in', 'nB', 'bDof', 'src', 'iw', 'djv', 'rows', 'td'):
                assert c[key] == base[key], (seed, c['case'], key)
            assert not c['big'] and c['terms'] and set(c['terms']) <= set(ft.TERMS)
            if c['crossing']:
                assert c['q'] in (4, 8, 16) and 257 <= c['n_k'] <= 300
            else:
                assert c['q'] == base['q'] and c['n_k'] == min(base['n_k'], ft.MAX_NK, ft.MAX_ROWS // c['q']) >= 1
            assert c['n_k'] * c['q'] <= ft.MAX_ROWS
            if c['grow']:
                assert 2 * c['n_k'] <= c['grow']['n_k'] <= 3 * c['n_k'] and set(c['grow']['terms']) != set(c['terms'])
            assert (c['grow'] is not None) == (c['case'] % 4 == 0)
            if c['flux']:
                nF = len(c['flux']['X'])
                assert 10 <= nF <= 60 and np.count_nonzero(c['flux']['coef']) == nF - nF // 2
                np.testing.assert_allclose(np.linalg.norm(c['flux']['normal'], axis=1), 1.0, rtol=1e-6)


@pytest.mark.parametrize('k', range(len(ft.SEED_LISTS)), ids=IDS)
def test_without_terms_the_reference_is_the_oracle_bit_for_bit(k):
    for c, d, flat, _, _ in evaluated(k):
        res, g = ft.reference(c, d, flat, terms={})
        want_l, want_g = fz.oracle(c, d, flat, torch.float64)
        assert res['loss'] == want_l and np.array_equal(g, want_g), (c['seed'], c['case'])


@pytest.mark.parametrize('k', range(len(ft.SEED_LISTS)), ids=IDS)
def test_every_drawn_term_moves_the_gradient_by_ten_bars(k):
    """A condition on the INPUTS, from the fp64 reference alone: dropping one drawn term (the others kept) moves the gradient by at
    least 10 x GRAD_BAR of its max norm -- the bar the case is judged at.  No (case, term) pair is exempt.  The same for the terms
    of batch 1 of the buffer-growth check; the boundary-flux rows move BCloss by at least 1e-2 of itself."""
    for c, d, flat, (ref, g), _ in evaluated(k):
        assert np.all(np.isfinite(g))
        sc = np.max(np.abs(g))
        for name in c['terms']:
            less = {t: v for t, v in c['terms'].items() if t != name}
            moved = np.max(np.abs(ft.reference(c, d, flat, terms=less)[1] - g)) / sc
            print('seed %d case %d: without %s %s the gradient moves by %.3g' % (c['seed'], c['case'], name, c['terms'][name][1], moved))
            assert moved >= 10 * ft.GRAD_BAR, (c['seed'], c['case'], name, moved)
        if c['flux'] is not None and ft.in_kernel_range(c):
            # the flux rows enter the BC component alone (the interior gradient, at gcoef x 8, dwarfs theirs): a pass that
            # forgets them misses BCloss, which every route is held to at LOSS_BAR -- the condition of
            # tests/test_nldiff_gpu.py::test_flux_bc_rows_and_the_term_together
            rf = ft.reference(c, d, flat, flux=c['flux'])[0]
            moved = abs(rf['BCloss'] - ref['BCloss']) / abs(rf['BCloss'])
            print('seed %d case %d: without the flux rows BCloss moves by %.3g' % (c['seed'], c['case'], moved))
            assert moved >= 1e-2 >= 100 * ft.LOSS_BAR, (c['seed'], c['case'], 'flux rows', moved)
        if c['grow'] is not None:
            d1, _ = ft.case_inputs(c, 1)
            t1, n_k1 = c['grow']['terms'], c['grow']['n_k']
            g1 = ft.reference(c, d1, flat, terms=t1, n_k=n_k1)[1]
            for name in t1:
                less = {t: v for t, v in t1.items() if t != name}
                moved = np.max(np.abs(ft.reference(c, d1, flat, terms=less, n_k=n_k1)[1] - g1)) / np.max(np.abs(g1))
                print('seed %d case %d batch 1: without %s %s the gradient moves by %.3g' % (c['seed'], c['case'], name, t1[name][1], moved))
                assert moved >= 10 * ft.GRAD_BAR, (c['seed'], c['case'], 'batch 1', name, moved)


@pytest.mark.parametrize('k', range(len(ft.SEED_LISTS)), ids=IDS)
def test_at_most_one_ill_conditioned_case_per_list(k):
    """The whitelist of tests/fuzz_routes.py (cond = dev32 / 2^-24 > COND_WHITELIST widens the bars) may apply to one case of a
    list at the most."""
    n = 0
    for c, d, flat, (ref, g), _ in evaluated(k):
        g32 = ft.reference(c, d, flat, torch.float32)[1]
        dev32 = np.max(np.abs(g32 - g)) / np.max(np.abs(g))
        print('seed %d case %d: dev32 %.2e' % (c['seed'], c['case'], dev32))
        n += dev32 / ft.U32 > ft.COND_WHITELIST
    assert n <= 1


def test_the_reference_of_every_case_takes_under_two_seconds():
    """The cost of the reference, not the load of the machine: a case timed above the bar is timed again, twice at the most, and
    its fastest evaluation counts."""
    worst = 0.0
    for k in range(len(ft.SEED_LISTS)):
        for c, d, flat, _, t in evaluated(k):
            for _ in range(2):
                if t < 2.0:
                    break
                t0 = time.perf_counter()
                ft.reference(c, d, flat)
                t = min(t, time.perf_counter() - t0)
            worst = max(worst, t)
    print('slowest fp64 reference evaluation: %.2f s' % worst)
    assert worst < 2.0


def test_the_lists_reach_the_one_row_forms_and_every_route():
    """From the case table alone (which kernel an engine then picks is asserted on the device:
    tests/test_fuzz_terms_gpu.py::test_the_lists_reach_every_route_on_the_device)."""
    cs = ft.all_cases()
    wider = lambda c, w: sum(1 for h in c['widths'] if h > w)
    assert sum(1 for c in cs if (c['n_k'] * c['q']) % 4 != 0) >= 2                  # the one-row forms and their tails
    assert any(c['offset'] for c in cs)
    assert any(c['offset'] and len(c['terms']) == 3 and all(v[0] is not None for v in c['terms'].values()) for c in cs)
    assert any(c['crossing'] for c in cs)
    # layer by layer: the GEMM form's widths, the layer-serial reverse of the tile kernels, two row-tile passes
    assert any(max(c['widths']) > 256 for c in cs)
    assert any(wider(c, 96) >= 5 for c in cs)
    assert any(128 < max(c['widths']) <= 256 for c in cs)
    assert any(c['L'] in (7, 8) and max(c['widths']) <= 50 and c['d_in'] <= ft.VN_KMAX_DIN for c in cs)     # the deep fused nets
    assert any(c['q'] > 256 for c in cs)
    assert any(c['q'] in (128, 256, 1296) and c['iw'] for c in cs)
    assert any(c['d_in'] >= 5 for c in cs)
    assert any(c['dim'] == 3 for c in cs)
    assert any(not c['td'] and 'nlflux' in c['terms'] for c in cs)
    assert any(not c['td'] and 'nldiff' in c['terms'] for c in cs)
    assert any(c['iw'] and c['djv'] and c['rows'] for c in cs)                     # integW + detJ vector + per-row tables + a term
    # boundary-flux rows on a net that AUTO and the generic kernels take, and on one whose rows share points (de-duplicated step)
    assert any(c['flux'] and ft.in_kernel_range(c) for c in cs)
    assert any(c['flux'] and ft.in_kernel_range(c) and ft.shares_points(c) for c in cs)
    assert any(c['flux'] and not ft.in_kernel_range(c) for c in cs)                # ... and one that must refuse them
    # batches of different size with different term sets
    assert sum(1 for c in cs if c['grow']) >= len(ft.SEED_LISTS)
