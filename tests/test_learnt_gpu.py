"""
GPU tier of the lifecycle the three learnt vectors share -- the nine polynomial coefficients (vn_set_coef_learn), the source
amplitudes (vn_set_source_learn) and the field amplitudes (vn_set_field_learn) -- with all three on one engine: an epoch against
single steps, snapshot / rollback / replay, one vector switched off next to the other two, one vector registered again at another
length, and every setter invalidating the snapshot.  Case 0 of tests/field_cases.py and tests/source_cases.py, J = 3, on the
automatic route and on the case's shared-point map.  Every comparison is bitwise.

And the paths of the reductions that no case of a few hundred rows reaches (the large-row cases of tests/source_cases.py): a capped
grid, where a thread takes more than one row of a partial, on the one-row and on the four-row kernels, with learnt entries on both
sides of the boundary between two stream groups -- the amplitude gradients of the source and of the field against their fp64
restatements, within the bars of their case modules.
"""
import numpy as np
import pytest
import torch

from tests import field_cases as fc
from tests import source_cases as sc
from tests import test_source_gpu as tsg
from tests.test_field_gpu import check_amp_grad as check_field_grad
from tests.test_field_gpu import grad_of, make_engine
from varnet_amd.engine import VNError

pytestmark = pytest.mark.gpu

CASE, J = 0, 3
LR = 0.02


def learnt_engine(route, source=True, params=None, coef=None, field=None):
    """An engine of the case with coefficients and field amplitudes learnt (from `coef` / `field`: the case's own) and, with
    `source`, the source basis registered and its amplitudes learnt; without, the batch's source is the plain stream."""
    eng = make_engine(CASE, route, J, lr=0.01)
    try:
        if params is not None:
            eng.set_params(params)
        eng.set_coef_learn([1] * 9, fc.coefs_of(CASE) if coef is None else coef, lr=LR)
        if source:
            Phi, samp = sc.basis(CASE, J)
            eng.set_source_basis(0, Phi)
            eng.set_source_learn([1] * J, samp, lr=LR)
        eng.set_field_learn([1] * J, fc.basis(CASE, J)[1] if field is None else field, lr=LR)
    except Exception:
        eng.close()
        raise
    return eng


def state(eng):
    """(parameters and their slots, coefficients, source amplitudes, field amplitudes, step counter) on the host."""
    torch.cuda.synchronize()
    return eng.export_state().copy(), eng.get_coefs(), eng.get_source_amps(), eng.get_field_amps(), eng.step


def same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


@pytest.mark.parametrize('route', ['auto', 'dedup'])
def test_shared_lifecycle_of_the_three_vectors(route):
    a, b = learnt_engine(route), learnt_engine(route)
    twin = None
    try:
        # 1. an epoch is its single steps; snapshot -> three steps -> rollback -> the same three steps
        start = state(a)
        a.train_epoch([0, 0, 0, 0])
        for _ in range(4):
            b.train_step(0)
        s4 = state(a)
        assert same(s4, state(b)), route
        assert s4[4] == 4 and all(np.all(s4[k] != start[k]) for k in (1, 2, 3)), (route, s4[1:], start[1:])
        a.state_snapshot()
        for _ in range(3):
            a.train_step(0)
        s7 = state(a)
        assert s7[4] == 7 and not any(np.array_equal(s7[k], s4[k]) for k in (0, 1, 2, 3))
        a.state_rollback()
        assert same(state(a), s4), route
        for _ in range(3):
            a.train_step(0)
        assert same(state(a), s7), route

        # 2. the source vector off, the other two on: their gradients are those of an engine that never learnt the source
        a.set_source_learn(None)
        with pytest.raises(VNError, match='no learnt source amplitudes'):
            a.get_source_amps(J=J)
        ga = grad_of(a)
        twin = learnt_engine(route, source=False, params=a.get_params(), coef=a.get_coefs(), field=a.get_field_amps())
        gt = grad_of(twin)
        assert np.array_equal(ga, gt), route
        for get in ('get_coefs', 'get_field_amps'):
            va, vt = getattr(a, get)(grad=True), getattr(twin, get)(grad=True)
            assert np.array_equal(va[0], vt[0]) and np.array_equal(va[1], vt[1]), (route, get, va, vt)
            assert np.all(va[1] != 0.0), (route, get, va)

        # 3. the source vector again, at another length
        Phi2, samp2 = sc.basis(CASE, 2)
        a.set_source_basis(0, Phi2)
        a.set_source_learn([1, 1], samp2, lr=LR)
        assert np.array_equal(a.get_source_amps(), samp2)
        with pytest.raises(VNError, match='the engine holds 2 source amplitudes, the caller asks for 3'):
            a.get_source_amps(J=J)
        grad_of(a)
        g2 = a.get_source_amps(grad=True)[1]
        assert g2.shape == (2,) and np.all(np.isfinite(g2)) and np.all(g2 != 0.0), (route, g2)
        a.train_step(0)
        assert a.step == 8 and np.all(a.get_source_amps() != samp2)

        # 4. a set of any one vector invalidates the snapshot
        for setter, args in (('set_coefs', (a.get_coefs(),)), ('set_source_amps', (samp2,)), ('set_field_amps', (a.get_field_amps(),)),
                             ('set_coef_learn', ([1] * 9, a.get_coefs(), None, None, LR)),
                             ('set_source_learn', ([1, 1], samp2, None, None, LR)),
                             ('set_field_learn', ([1] * J, a.get_field_amps(), None, None, LR))):
            a.state_snapshot()
            getattr(a, setter)(*args)
            with pytest.raises(VNError, match='error 3: no snapshot to roll back to'):
                a.state_rollback()
    finally:
        a.close()
        b.close()
        if twin is not None:
            twin.close()


@pytest.mark.parametrize('vector', ['source', 'field'])
@pytest.mark.parametrize('k', range(len(sc.BIG)), ids=sc.BIG_IDS)
def test_amplitude_gradient_on_a_capped_grid(k, vector):
    """nT > 256 x 256 (one-row kernels) and nT > 4 x 256 x 256 (four-row kernels), J = 9, entries 0, 7 and 8 learnt, automatic
    row-wise route."""
    i, n, mask = sc.N_CASES + k, sc.BIG_J, sc.BIG_MASK
    q, n_k = sc.case(i)[3:5]
    assert n_k * q > (1 if k == 0 else 4) * 256 * 256 and (n_k * q) % 4 == (2 if k == 0 else 0)
    cases = sc if vector == 'source' else fc
    _, _, g64, S = cases.reference64(i, n)
    on = np.array(mask, dtype=bool)
    assert np.all(np.abs(g64[on]) > cases.COND_FLOOR * S[on]), (g64, S)    # the bar of a learnt component is relative to itself
    eng = tsg.make_engine(i, 'auto', n) if vector == 'source' else make_engine(i, 'auto', n)
    try:
        if vector == 'source':
            eng.set_source_learn(mask, sc.basis(i, n)[1], lr=0.01)
            grad_of(eng)
            tsg.check_amp_grad('%s/J%d/auto/amp' % (sc.BIG_IDS[k], n), eng.get_source_amps(grad=True)[1], i, n, mask)
        else:
            eng.set_field_learn(mask, fc.basis(i, n)[1], lr=0.01)
            grad_of(eng)
            check_field_grad('%s/J%d/auto/amp' % (sc.BIG_IDS[k], n), eng.get_field_amps(grad=True)[1], g64, S, mask)
    finally:
        eng.close()
