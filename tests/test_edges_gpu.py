"""
The three edge row sets -- boundary-flux rows (set_flux_bc), periodic pairs (set_periodic), observations (set_observations) --
through what they share on the host layer: one record, one pass, one registration path and one fold of the step's reduction.

Every comparison is bitwise: an engine is compared with a twin that reached the same registration another way.  Nothing here
knows a reference value; the parity of each set is tests/test_flux_bc_gpu.py, test_periodic_gpu.py and test_obs_gpu.py.

Row counts {1, 33, 257, 600}: 33 is one past the generic kernels' 32-row tile, 257 one past the seed kernels' 256-thread block,
and 600 rows give 19 reverse partials, so one group of the reduction sums two of them.  A size is the count of flux rows, of
pairs (twice as many rows) and of point observations.
"""
import numpy as np
import pytest
import torch

from tests.obs_cases import CASES
from tests.test_flux_bc_gpu import flux_rows
from tests.test_obs_gpu import evaluate, register
from tests.test_obs_gpu import setup as case_engine
from tests.test_periodic_gpu import BDV, periodic_rows
from varnet_amd.engine import VN_KERNEL_AUTO, VN_KERNEL_GENERIC, VNError

pytestmark = pytest.mark.gpu

CI = 2                                                      # the small 2D+t case
D_IN, DIM = CASES[CI][0], CASES[CI][1]
SIZES = [1, 33, 257, 600]
KINDS = ['flux', 'periodic', 'obs']
ROUTES = ['auto', 'generic', 'dedup']
LAM = 0.5


def obs_points(seed, nO, with_dir):
    """nO point sensors (rowptr None) with quadrature weights, weights and, with_dir, directions; fp32 as the engine holds them."""
    rng = np.random.default_rng(seed)
    o = dict(X=rng.uniform(-1, 1, (nO, D_IN)).astype(np.float32), q=rng.uniform(0.5, 1.5, nO).astype(np.float32),
             dir=(0.5 * rng.standard_normal((nO, DIM))).astype(np.float32), value=rng.standard_normal(nO).astype(np.float32),
             wgt=(1.0 / rng.uniform(0.5, 2.0, nO) ** 2).astype(np.float32), rowptr=None)
    if not with_dir:
        o['dir'] = None
    return o


def engine(route):
    """An engine on the case without any edge set; 'dedup': the automatic route on the identity point map."""
    eng, flat, d = case_engine(CI, VN_KERNEL_GENERIC if route == 'generic' else VN_KERNEL_AUTO)
    if route == 'dedup':
        nT = d['Input'].shape[0]
        idx = torch.arange(nT, dtype=torch.int32)
        eng.set_dedup(0, d['Input'], idx, torch.arange(nT + 1, dtype=torch.int32), idx)
    return eng


def put(eng, kind, size, deriv=True):
    """Register `kind` at `size`; the rows depend on (kind, size) only.  deriv False: gamma = 0 / no directions."""
    if kind == 'flux':
        fx = flux_rows(100 + size, D_IN, DIM, size)
        eng.set_flux_bc(fx['X'], fx['normal'], fx['coef'], fx['label'], BDV)
    elif kind == 'periodic':
        pr = periodic_rows(200 + size, D_IN, DIM, size)
        eng.set_periodic(pr['X'], pr['dir'], 1.0 if deriv else 0.0, BDV)
    else:
        register(eng, obs_points(300 + size, size, deriv), LAM)


def clear(eng, kind):
    {'flux': eng.set_flux_bc, 'periodic': eng.set_periodic, 'obs': eng.set_observations}[kind](None)


def bits(eng):
    """eval_loss's four scalars, the gradient buffer (gradient and the four scalars of grad) and both misfits, as bytes."""
    out, m0, g, m1 = evaluate(eng)
    return out.tobytes(), g.tobytes(), m0, m1


# ---- 1. all three sets on one engine ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('route', ROUTES)
def test_all_three_sets(route, size):
    eng, twin = engine(route), engine(route)
    try:
        for e in (eng, twin):
            for kind in KINDS:
                put(e, kind, size)
        gb = eng.bind_grad_buffer()
        runs = []
        for _ in range(2):
            eng.grad(0)
            torch.cuda.synchronize()
            runs.append((gb.cpu().numpy().tobytes(), eng.obs_misfit()))
        assert runs[0] == runs[1]
        assert np.isfinite(np.frombuffer(runs[0][0], dtype=np.float32)).all() and runs[0][1] > 0.0
        eng.train_epoch([0, 0, 0, 0])
        for _ in range(4):
            twin.train_step(0)
        torch.cuda.synchronize()
        assert eng.step == 4 and twin.step == 4
        assert np.array_equal(eng.get_params(), twin.get_params())
        assert eng.export_state().tobytes() == twin.export_state().tobytes()          # parameters, optimizer slots, step counter
    finally:
        eng.close()
        twin.close()


# ---- 2. one set cleared next to the other two ---------------------------------------------------------------------------------
@pytest.mark.parametrize('gone', KINDS)
@pytest.mark.parametrize('route', ROUTES)
def test_one_set_cleared_next_to_the_other_two(route, gone):
    eng, twin = engine(route), engine(route)
    try:
        size = dict(flux=257, periodic=33, obs=600)
        for kind in KINDS:
            put(eng, kind, size[kind])
            if kind != gone:
                put(twin, kind, size[kind])
        eng.grad(0)                                                      # a step with all three ...
        clear(eng, gone)                                                 # ... then one of them cleared
        a, b = bits(eng), bits(twin)
        assert a == b
        assert (a[2] is None) == (gone == 'obs')                         # the misfit is compared whenever observations remain
    finally:
        eng.close()
        twin.close()


# ---- 3. re-registration: buffers reused, shrunk, grown, tangent buffers allocated late ----------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('route', ROUTES)
def test_reregistration_walk(route, kind):
    """600 -> 1 -> 33 -> 257 on one engine; periodic pairs start at gamma = 0 and observations without directions, so the
    tangent buffers of those two are first allocated at the second stop.  Each stop equals a fresh engine registered there."""
    eng = engine(route)
    try:
        for kind2 in KINDS:
            if kind2 != kind:
                put(eng, kind2, 33)
        for stop, size in enumerate([600, 1, 33, 257]):
            deriv = stop > 0
            put(eng, kind, size, deriv)
            fresh = engine(route)
            try:
                for kind2 in KINDS:
                    put(fresh, kind2, size if kind2 == kind else 33, deriv if kind2 == kind else True)
                assert bits(eng) == bits(fresh), (kind, size)
            finally:
                fresh.close()
    finally:
        eng.close()


# ---- 4. a refused registration drops the previous one and leaves the other two alone ------------------------------------------
@pytest.mark.parametrize('kind,match', [('periodic', 'error 1: periodic pairs: the derivative weight gamma'),
                                        ('obs', 'error 1: observations: the weight lambda')])
@pytest.mark.parametrize('route', ROUTES)
def test_refused_registration_drops_the_previous_one(route, kind, match):
    eng, twin = engine(route), engine(route)
    try:
        for k in KINDS:
            put(eng, k, 33)
            if k != kind:
                put(twin, k, 33)
        eng.grad(0)
        with pytest.raises(VNError, match=match):                        # a plain error code: the argument check precedes every launch
            if kind == 'periodic':
                pr = periodic_rows(7, D_IN, DIM, 33)
                eng.set_periodic(pr['X'], pr['dir'], -1.0, BDV)
            else:
                o = obs_points(7, 33, True)
                eng.set_observations(o['X'], o['value'], q=o['q'], dir=o['dir'], wgt=o['wgt'], weight=-1.0)
        if kind == 'obs':
            with pytest.raises(VNError, match='error 3: vn_get_obs_misfit: no observations are registered'):
                eng.obs_misfit()
        assert bits(eng) == bits(twin)
    finally:
        eng.close()
        twin.close()
