"""
CPU tier of the learnt-vector fuzz (tests/fuzz_learnt.py): conditions on the committed seed lists that keep the GPU tier
(tests/test_fuzz_learnt_gpu.py) honest, checked from the fp64 reference tests/joint_ref.py alone for exactly the cases the GPU tier
runs -- the draw sequence of tests/fuzz_terms.py is kept and no case is left out; the joint reference reduces to
tests/fuzz_terms.reference and to the single-vector modules; every drawn edge set, learnt vector and weight vector moves what the
GPU tier judges; the conditioning floor of the vector bar and the fp32 whitelist are the exception; and the lists reach the
shape-dependent paths of vn_learnt.hip, restated from the drawn shapes by the rule of vn_rows4.h::rows4_ok.
"""
import functools

import numpy as np
import pytest
import torch

from tests import bic_ref, fbc_ref, field_ref, inverse_ref, source_ref
from tests import fuzz_learnt as fl
from tests import fuzz_terms as ft
from tests import joint_ref

IDS = ['%s%s%d' % ('steady' if st else 'td', '_mor' if mor else '', seed) for seed, n, st, mor in fl.SEED_LISTS]
LISTS = range(len(fl.SEED_LISTS))
EDGE_SETS = ('flux', 'periodic', 'obs')


@functools.lru_cache(maxsize=None)
def cases(k):
    return fl.draw_list(*fl.SEED_LISTS[k])


def full_pieces(c):
    """What an engine of the hand-written kernels carries (edge sets only inside VN_KMAX_*)."""
    return fl.pieces_of(c, ft.in_kernel_range(c))


@functools.lru_cache(maxsize=None)
def evaluated(k):
    """[(case, batch-0 data, theta, pieces, fp64 (result, gradient, vectors), fp32 the same)] of list k: computed once, shared,
    never modified."""
    out = []
    for c in cases(k):
        p, flat = fl.prepare(c), ft.theta(c)
        pieces = full_pieces(c)
        out.append((c, p, flat, pieces, fl.reference(c, p, flat, pieces), fl.reference(c, p, flat, pieces, torch.float32, scales=False)))
    return out


def _moved(g, g0):
    return float(np.max(np.abs(g - g0)) / np.max(np.abs(g0)))


def test_the_seed_lists_have_the_shape_of_fuzz_terms():
    assert len(fl.SEED_LISTS) == 5 and all(n <= 8 for _, n, _, _ in fl.SEED_LISTS)
    assert [(st, mor) for _, _, st, mor in fl.SEED_LISTS] == [(False, False)] * 3 + [(True, False), (False, True)]


def test_the_draw_sequence_of_fuzz_terms_is_kept():
    """A seed names the same net, sizes, terms, flux rows and flags as in tests/fuzz_terms.py, and every list holds its cases
    0..n-1: nothing is left out."""
    for k, lst in enumerate(fl.SEED_LISTS):
        base = ft.draw_list(*lst)
        got = cases(k)
        assert [c['case'] for c in got] == list(range(lst[1]))
        for c, b in zip(got, base):
            assert set(c) == set(b) | {'x'}
            np.testing.assert_equal({key: c[key] for key in b}, b)


def test_the_extra_draws_are_what_the_module_says():
    n_learn = n_all = 0
    for k in LISTS:
        five = [c for c in cases(k) if c['x']['mode'] == 'learn' and c['flux'] is not None]
        assert not five or any(set(c['x']['learn']) == set(fl.VECTORS) for c in cases(k))
        for c in cases(k):
            x, v = c['x'], c['x']['vec']
            if x['mode'] == 'weights':
                assert not x['learn'] and np.all((x['omega'] >= 0.25) & (x['omega'] <= 4.0))
                if x['causal'] is not None:
                    assert c['td'] and 2 <= x['causal'][1] <= 6 and set(x['causal'][0]) == set(range(x['causal'][1]))
                continue
            n_learn += 1
            n_all += set(x['learn']) == set(fl.VECTORS)
            assert x['learn'] and set(x['learn']) <= set(x['can']) and ('fluxbc' in x['can']) == (c['flux'] is not None)
            here = [3 * i + j for i, t in enumerate(('reaction', 'nlflux', 'nldiff')) if t in c['terms'] for j in range(3)]
            m9 = v['coef']['mask']
            assert m9[here].any() and m9.sum() - m9[here].sum() <= 1
            assert v['source']['J'] in fl.SRC_J and v['field']['J'] in fl.FLD_J and v['bic']['J'] in fl.BIC_J
            assert (v['fluxbc']['Jl'], v['fluxbc']['J'] - v['fluxbc']['Jl']) in fl.FBC_J
            for name in fl.VECTORS[1:]:
                assert v[name]['mask'].any() and v[name]['mask'].size == v[name]['J'] == v[name]['amp'].size
                assert np.array_equal(v[name]['amp'], v[name]['amp'].astype(np.float32).astype(np.float64))
            if x['periodic']:
                nP = len(x['periodic']['X']) // 2
                assert 1 <= nP <= 40 and x['periodic']['gamma'] in (0.0, 0.5, 1.0)
                assert np.array_equal(x['periodic']['dir'][:nP], x['periodic']['dir'][nP:])
            if x['obs']:
                o = x['obs']
                nO = len(o['value'])
                assert 1 <= nO <= 50 and o['lam'] in (0.5, 2.0)
                if o['rowptr'] is not None:
                    assert o['rowptr'][0] == 0 and o['rowptr'][-1] == len(o['X']) and set(np.diff(o['rowptr'])) <= {1, 2, 3, 4}
            assert c['n_k'] * c['q'] <= ft.MAX_ROWS                            # the capped grids belong to the *_on_a_capped_grid tests
    assert 2 * n_learn >= sum(n for _, n, _, _ in fl.SEED_LISTS) and n_all >= 1


@pytest.mark.parametrize('k', LISTS, ids=IDS)
def test_with_nothing_learnt_the_joint_reference_is_fuzz_terms_reference_bit_for_bit(k):
    """No vector, no weights, no periodic pairs, no observations: loss pieces, lossVec and gradient equal tests/fuzz_terms.reference
    bit for bit, with the flux rows on the nets that take them."""
    for c, p, flat, _, _, _ in evaluated(k):
        flux = c['flux'] if ft.in_kernel_range(c) else None
        res, g, vec = fl.reference(c, p, flat, frozenset(['flux'] if flux is not None else []), weights=False)
        want, gw = ft.reference(c, p['d'], flat, flux=flux)
        assert not vec
        for key in fl.KEYS:
            assert res[key] == want[key], (c['seed'], c['case'], key)
        assert np.array_equal(res['lossVec'], want['lossVec']) and np.array_equal(g, gw), (c['seed'], c['case'])


@pytest.mark.parametrize('k', LISTS, ids=IDS)
def test_with_one_vector_the_joint_reference_is_the_single_vector_module(k):
    """Bit for bit -- loss pieces, theta-gradient, vector gradient and scale S -- for every vector a case learns: the interior graph
    is built by the expressions of tests/source_ref.py, tests/field_ref.py, tests/bic_ref.py and tests/inverse_ref.py, and the flux
    rows go through tests/fbc_ref.evaluate itself, added as tests/fuzz_terms.reference adds tests/flux_ref.flux_term."""
    for c, p, flat, _, _, _ in evaluated(k):
        d, b, v = p['d'], p['bases'], c['x']['vec']
        kw = fl.ref_kw(c, d, p['n_k'])
        t = c['terms']
        three = (t.get('nldiff'), t.get('nlflux'), t.get('reaction'))
        nine = inverse_ref.nine(*three)
        for name in c['x']['learn']:
            pieces = frozenset([name] + (['flux'] if name == 'fluxbc' else []))
            res, g, vec = fl.reference(c, p, flat, pieces)
            if name == 'coef':
                want = inverse_ref.evaluate(flat, c['d_in'], c['widths'], fl.nine_of(c), *three, **kw)
            elif name == 'source':
                want = source_ref.evaluate(flat, c['d_in'], c['widths'], d['source'], b['source'].T, v[name]['amp'], nine, *three, **kw)
            elif name == 'field':
                kw2 = dict(kw)
                want = field_ref.evaluate(flat, c['d_in'], c['widths'], kw2.pop('gcoef'), b['field'], v[name]['amp'], nine, *three, **kw2)
            elif name == 'bic':
                kw2 = dict(kw)
                want = bic_ref.evaluate(flat, c['d_in'], c['widths'], kw2.pop('biLabel'), b['bic'].T, v[name]['amp'], nine, *three, **kw2)
            else:
                fx = c['flux']
                f64 = lambda a: np.asarray(a, dtype=np.float64)
                F, gF, ga, S = fbc_ref.evaluate(f64(flat), c['d_in'], c['widths'], c['dim'], f64(fx['X']), f64(fx['normal']), f64(fx['coef']),
                                                f64(fx['label']), f64(b['fluxbc']), v[name]['Jl'], v[name]['amp'], fl.BIDIMVAL,
                                                float(d['w'][0]), c['act'])
                r0, g0, _ = fl.reference(c, p, flat, frozenset())
                assert res['BCloss'] == r0['BCloss'] + F and res['loss'] == r0['loss'] + d['w'][0] * F
                assert np.array_equal(g, g0 + d['w'][0] * gF)
                assert np.array_equal(vec[name][0], ga) and np.array_equal(vec[name][1], S), (c['seed'], c['case'], name)
                continue
            for key in fl.KEYS:
                assert res[key] == want[0][key], (c['seed'], c['case'], name, key)
            assert np.array_equal(g, want[1]), (c['seed'], c['case'], name)
            assert np.array_equal(vec[name][0], want[2]) and np.array_equal(vec[name][1], want[3]), (c['seed'], c['case'], name)


@pytest.mark.parametrize('k', LISTS, ids=IDS)
def test_every_drawn_piece_counts(k):
    """Conditions on the INPUTS, from the fp64 reference alone, as the issue sets them.  Dropping a drawn edge set moves the loss
    piece it joins by at least 100 x LOSS_BAR: BCloss for the flux rows and the periodic pairs, `loss` (which lambda O joins) for the
    observations.  Setting any learnt vector to zero -- the coefficients: every term with a learnt entry switched off -- or dropping
    the weights moves the theta-gradient by at least 10 x GRAD_BAR of its max norm.  At the scales of tests/fuzz_terms.py (gcoef x
    8) the interior part dwarfs the boundary and observation parts on most draws, so the seeds and list lengths of
    tests/fuzz_learnt.SEED_LISTS are the ones whose cases meet these conditions; the conditions themselves are never moved."""
    bad = [f for entry in evaluated(k) for f in piece_failures(entry)]
    assert not bad, bad


def piece_failures(entry):
    """The conditions of test_every_drawn_piece_counts on one case: [(case, piece, figure)] of those it misses."""
    c, p, flat, pieces, (res, g, vec), _ = entry
    tag, bad = 'seed %d case %d' % (c['seed'], c['case']), []
    for s in EDGE_SETS:
        if s not in pieces:
            continue
        less = pieces - {s, 'fluxbc'} if s == 'flux' else pieces - {s}
        r0 = fl.reference(c, p, flat, less, scales=False)[0]
        if s == 'obs':
            moved = abs(res['loss'] - r0['loss']) / abs(res['loss'])
            print('%s: without the observations loss moves by %.3g; the misfit is %.3g' % (tag, moved, res['obs']))
            if 'obs' in r0 or not moved >= 100 * fl.LOSS_BAR:
                bad.append((tag, s, moved))
        else:
            moved = abs(res['BCloss'] - r0['BCloss']) / abs(res['BCloss'])
            print('%s: without %s BCloss moves by %.3g' % (tag, s, moved))
            if not moved >= 100 * fl.LOSS_BAR:
                bad.append((tag, s, moved))
    for name in c['x']['learn']:
        if name not in pieces:
            continue
        r0, g0, _ = fl.reference(c, p, flat, pieces, zero=(name,), scales=False)
        moved = _moved(g0, g)
        print('%s: with %s at zero the gradient moves by %.3g' % (tag, name, moved))
        if not moved >= 10 * fl.GRAD_BAR:
            bad.append((tag, name, moved))
    if c['x']['mode'] == 'weights':
        moved = _moved(fl.reference(c, p, flat, pieces, weights=False)[1], g)
        print('%s: without the %s weights the gradient moves by %.3g' % (tag, 'causal' if c['x']['causal'] is not None else 'static', moved))
        if not moved >= 10 * fl.GRAD_BAR:
            bad.append((tag, 'weights', moved))
    return bad


def test_the_floor_is_the_exception_and_the_fp32_reference_stays_inside_the_bars():
    """Over all masked-in components of all vectors of all lists COND_FLOOR S_j is the binding branch of the bar for at most
    BINDING_FRAC of them, and the fp32 run of the joint reference stays within every component's bar."""
    n = binding = 0
    for k in LISTS:
        for c, p, flat, pieces, (_, g, vec), (_, g32, vec32) in evaluated(k):
            line = []
            for name, (gv, S) in vec.items():
                on = fl.mask_of(c, name) & (S > 0.0)          # (a coefficient of a term the batch does not carry: 0 of 0)
                bar = fl.vector_bars(gv, S)
                n += int(on.sum())
                binding += int(np.sum(fl.COND_FLOOR * S[on] > np.abs(gv[on])))
                err = np.abs(vec32[name][0] - gv)
                assert np.all(err[on] <= bar[on]), (c['seed'], c['case'], name, err / np.maximum(bar, 1e-300))
                line.append('%s min|g|/S %.1e fp32 err/bar %.2f' % (name, np.min(np.abs(gv[on]) / S[on]) if on.any() else np.nan,
                                                                   np.max(err[on] / bar[on]) if on.any() else 0.0))
            dev32 = _moved(g32, g)
            print('seed %d case %d {%s}: %s dev32 %.2e' % (c['seed'], c['case'], ' '.join(sorted(vec)), '; '.join(line), dev32))
    print('%d of %d components have the floor as the binding branch (%.3f)' % (binding, n, binding / n))
    assert binding <= fl.BINDING_FRAC * n, (binding, n)


@pytest.mark.parametrize('k', LISTS, ids=IDS)
def test_at_most_one_ill_conditioned_case_per_list(k):
    """The whitelist of tests/fuzz_routes.py (cond = dev32 / 2^-24 > COND_WHITELIST widens the bars) may apply to one case of a
    list at the most."""
    n = 0
    for c, _, _, _, (_, g, _), (_, g32, _) in evaluated(k):
        n += _moved(g32, g) / fl.U32 > fl.COND_WHITELIST
    assert n <= 1


# ---- reach: the rule of vn_rows4.h::rows4_ok restated on the drawn shapes ------------------------------------------------
def rows4(n, c):
    """The four-row form: the row count is a multiple of 4 and every stream is 16-byte aligned (`offset` registers them one float
    off the grid)."""
    return n % 4 == 0 and not c['offset']


def reach(cs):
    """{path: reached} for a set of cases, from the drawn shapes alone."""
    learns = lambda c, name: name in c['x']['learn']
    nT = lambda c: c['n_k'] * c['q']
    v = lambda c, name: c['x']['vec'][name]
    kr = ft.in_kernel_range
    got = {}
    rows = dict(source=nT, field=lambda c: nT(c) * c['dim'], bic=lambda c: c['nB'], fluxbc=lambda c: len(c['flux']['X']))
    for name, n in rows.items():                                                    # the mix: both forms
        got['mix4 ' + name] = any(learns(c, name) and rows4(n(c), c) for c in cs)
        got['mix1 ' + name] = any(learns(c, name) and not rows4(n(c), c) for c in cs)
    for name in ('coef', 'source'):                                                 # the row reductions: both forms
        got['rows4 ' + name] = any(learns(c, name) and rows4(nT(c), c) for c in cs)
        got['rows1 ' + name] = any(learns(c, name) and not rows4(nT(c), c) for c in cs)
    got['source rows4, q % 4 != 0, FE table'] = any(learns(c, 'source') and rows4(nT(c), c) and c['q'] % 4 != 0 and not c['rows'] for c in cs)
    got['source per-row tables'] = any(learns(c, 'source') and c['rows'] for c in cs)
    for dim in (1, 2, 3):
        got['field dim %d' % dim] = any(learns(c, 'field') and c['dim'] == dim for c in cs)
    got['field on a map with >= 4 rows per point'] = any(
        learns(c, 'field') and ft.shares_points(c) and kr(c) and nT(c) / (np.max(fl.prepare(c)['dd'][1]) + 1) >= 4.0 for c in cs)
    group0 = lambda m: any(not m[8 * i:8 * i + 8].any() for i in range((m.size + 7) // 8))
    got['an all-zero group of eight'] = any(learns(c, name) and v(c, name)['J'] > 8 and group0(v(c, name)['mask'])
                                            for c in cs for name in fl.VECTORS[1:])
    part = lambda c: learns(c, 'fluxbc') and kr(c) and v(c, 'fluxbc')['J'] > v(c, 'fluxbc')['Jl']
    got['part boundary inside a group'] = any(part(c) and 0 < v(c, 'fluxbc')['Jl'] < 8 for c in cs)
    got['part boundary at the end of a group'] = any(part(c) and v(c, 'fluxbc')['Jl'] == 8 for c in cs)
    got['part boundary beyond the first group'] = any(part(c) and v(c, 'fluxbc')['Jl'] > 8 for c in cs)
    got['steady BC/IC'] = any(learns(c, 'bic') and not c['td'] for c in cs)
    got['a vector on routes 4 and 40'] = any(c['x']['learn'] for c in cs)           # (every net runs both forms)
    got['a vector under AUTO layer by layer'] = any(c['x']['learn'] and not kr(c) for c in cs)
    got['a vector on route 30'] = any(c['x']['learn'] and ft.shares_points(c) and kr(c) for c in cs)
    got['a 6- or 7-layer net with a vector'] = any(c['x']['learn'] and c['L'] in (6, 7) and max(c['widths']) <= 64 for c in cs)
    got['d_in >= 5'] = any(c['x']['learn'] and c['d_in'] >= 5 for c in cs)
    got['causal on a shared-point map'] = any(c['x']['mode'] == 'weights' and c['x']['causal'] is not None and ft.shares_points(c) and kr(c)
                                              for c in cs)
    got['periodic + observations + two vectors'] = any(c['x']['periodic'] and c['x']['obs'] and len(c['x']['learn']) >= 2 and kr(c) for c in cs)
    got['all five vectors'] = any(set(c['x']['learn']) == set(fl.VECTORS) for c in cs)
    got['learnt slots grow'] = any(c['grow'] and learns(c, 'source') and learns(c, 'field') for c in cs)
    return got


def test_the_lists_reach_the_shape_dependent_paths():
    """From the drawn shapes; that every vector then runs on every route that carries it is asserted on the device
    (tests/test_fuzz_learnt_gpu.py::test_every_vector_ran_on_every_route_that_carries_it)."""
    got = reach([c for k in LISTS for c in cases(k)])
    assert all(got.values()), [k for k, ok in got.items() if not ok]


def test_joint_ref_takes_a_dtype():
    c = cases(0)[0]
    p, flat = fl.prepare(c), ft.theta(c)
    res, g, vec = joint_ref.evaluate(flat, c['d_in'], c['widths'], p['terms'], fl.ref_kw(c, p['d'], p['n_k']), torch.float32)
    assert res['lossVec'].dtype == np.float32 and not vec and np.all(np.isfinite(g))
