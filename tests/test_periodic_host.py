"""
CPU tier of the periodic boundary pairs (`ADPDE(..., periodic=[(A, B)])`, `VarNet(periodicDeriv=...)`, vn_set_periodic): the
refusals of `ADPDE`, host assembly of the paired rows on both domains and both vertex orders, the Dirichlet and flux rows
leaving the paired indicators out, the default leaving everything as it was, the BC component through a stand-in engine (the
oracle engine plus the fp64 restatement of tests/periodic_ref.py), the declaration and binding of the entry point, and the
restatement's own gradient against central differences.
"""
import os
import re

import numpy as np
import pytest

from oracle import tf1_graph as og
from tests import periodic_ref
from tests.oracle_engine import OracleEngine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D, PolygonDomain2D
from varnet_amd.mor import MOR
from varnet_amd.utility import UF
from varnet_amd.varnet import VarNet

uf = UF()
pi = np.pi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class PeriodicOracleEngine(OracleEngine):
    """The oracle engine with vn_set_periodic (and a vn_set_flux_bc that records its rows): the periodic mean of
    tests/periodic_ref.py added to the BC component, w0 times it to the loss and the gradient."""
    per = None
    flux = None

    def set_periodic(self, X=None, dir=None, gamma=1.0, biDimVal=1.0):
        if X is None or len(X) == 0:
            self.per = None
            return
        self.per = (np.array(X, dtype=float), np.array(dir, dtype=float), float(gamma), float(biDimVal))

    def set_flux_bc(self, X=None, normal=None, coef=None, label=None, biDimVal=1.0):
        self.flux = None if X is None or len(X) == 0 else np.array(X, dtype=float)

    def _eval(self, batch):
        res, g = super()._eval(batch)
        if self.per is None:
            return res, g
        X, d, gamma, bdv = self.per
        P, gP, _, _ = periodic_ref.periodic_term(self.theta.astype(np.float64), self.inpDim, self.layerWidth, self.dim, X, d, gamma,
                                                 bdv)
        res = dict(res)
        res['BCloss'] = res['BCloss'] + P
        res['loss'] = res['loss'] + self.w[0] * P
        return res, g + self.w[0] * gP


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return PeriodicOracleEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                                    isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                                    learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


SQUARE = np.array([[0., 0.], [1., 0.], [1., 1.], [0., 1.]])             # counter-clockwise: bottom, right, top, left
SQUARE_CW = SQUARE[[0, 3, 2, 1]]                                        # clockwise: left, top, right, bottom
IC1 = lambda x: np.cos(2 * pi * x)
IC2 = lambda x: np.sin(pi * x[:, 1:2])
g0 = lambda x, t=0: np.zeros([len(x), 1])


def pde1d(periodic, t=True, BCs=None, **kw):
    return ADPDE(Domain1D(np.array([0.0, 1.0])), diff=0.05, vel=0.5, tInterval=[0, 0.5] if t else None, BCs=BCs,
                 IC=IC1 if t else None, periodic=periodic, **kw)


def pde2d(periodic, vertices=SQUARE, BCs=None, **kw):
    return ADPDE(PolygonDomain2D(vertices), diff=0.1, vel=[1.0, 0.0], tInterval=[0, 1.0], BCs=BCs, IC=IC2, periodic=periodic, **kw)


# ---- ADPDE -------------------------------------------------------------------------------------------------------------------
def test_adpde_refusals():
    for bad in ([], (), 'x', [(0,)], [(0, 1, 2)], [(0, 1.0)], [[0, True]], [3]):
        with pytest.raises(ValueError, match='periodic must be a non-empty list of boundary indicator pairs'):
            pde1d(bad)
    with pytest.raises(ValueError, match=r'periodic pair \(0, 2\): boundary indicator 2 outside \[0, 2\)'):
        pde1d([(0, 2)])
    with pytest.raises(ValueError, match=r'periodic pair \(-1, 1\): boundary indicator -1 outside \[0, 2\)'):
        pde1d([(-1, 1)])
    with pytest.raises(ValueError, match=r'periodic pair \(1, 1\): the two boundary indicators must be distinct'):
        pde1d([(1, 1)])
    with pytest.raises(ValueError, match=r'periodic pair \(1, 2\): boundary indicator 1 appears in more than one pair'):
        pde2d([(3, 1), (1, 2)])
    with pytest.raises(ValueError, match=r'periodic pair \(0, 1\): BCs\[1\] must be empty, a periodic edge has no \[a, b, g\]'):
        pde1d([(0, 1)], BCs=[[], [1.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match=r'periodic pair \(3, 1\): BCs\[3\] must be empty'):
        pde2d([(3, 1)], BCs=[[], [], [], [0.0, 1.0, g0]])
    # geometry: neighbouring edges of the square have equal lengths but normals at a right angle ...
    with pytest.raises(ValueError, match=r'periodic pair \(0, 1\): the outward normals of edges 0 and 1 are not opposite'):
        pde2d([(0, 1)])
    # ... a trapezium's slanted sides have neither, and its parallel sides have opposite normals but unequal lengths
    trap = np.array([[0., 0.], [2., 0.], [1.5, 1.], [0., 1.]])
    with pytest.raises(ValueError, match=r'periodic pair \(0, 2\): edges 0 and 2 have unequal lengths'):
        pde2d([(0, 2)], vertices=trap)
    with pytest.raises(ValueError, match=r'periodic pair \(1, 3\): edges 1 and 3 have unequal lengths'):
        pde2d([(1, 3)], vertices=trap)
    obs = np.array([[0.25, 0.25], [0.75, 0.25], [0.75, 0.75], [0.25, 0.75]])
    with pytest.raises(ValueError, match=r'periodic pair \(3, 5\): obstacle edges cannot be paired'):
        ADPDE(PolygonDomain2D(SQUARE, [obs]), diff=0.1, vel=[1.0, 0.0], periodic=[(3, 5)])


def test_adpde_bctype_and_pairs():
    assert pde1d([(0, 1)]).BCtype == ['Periodic', 'Periodic'] and pde1d([(0, 1)]).periodic == [(0, 1)]
    assert pde1d([[1, 0]]).periodic == [(1, 0)]                        # either order, lists or tuples
    p = pde2d([(3, 1)], BCs=[[], [], [1.0, 0.0, g0], []])
    assert p.BCtype == ['Dirichlet', 'Periodic', 'Neumann', 'Periodic'] and p.periodic == [(3, 1)]
    assert pde2d([(3, 1), (0, 2)]).BCtype == ['Periodic'] * 4
    assert pde2d([(np.int64(0), np.int32(2))]).periodic == [(0, 2)]


def test_adpde_without_periodic_is_unchanged():
    a, b = pde2d(None, BCs=[[], [2.0, 0.0, g0], [], []]), pde2d(None, BCs=[[], [2.0, 0.0, g0], [], []])
    assert a.periodic is None
    assert a.BCtype == ['Dirichlet', 'Neumann', 'Dirichlet', 'Dirichlet']
    keys = set(a.__dict__) - {'periodic'}
    # the attributes a PDE had before the keyword existed, every one of them as it was
    assert keys == {'diff', 'diffFun', 'velFun', 'vel', 'source', 'sourceFun', 'd_diff', 'd_diffFun', 'reaction', 'nlflux', 'nldiff',
                    'dim', 'domain', 'timeDependent', 'tInterval', 'BCs', 'BCtype', 'IC', 'cEx', 'MORvar'}
    x = np.array([[0.3, 0.4]])
    for bc_a, bc_b in zip(a.BCs, b.BCs):
        assert bc_a[:2] == bc_b[:2] and np.array_equal(bc_a[2](x), bc_b[2](x))


def test_mor_with_periodic_raises():
    def diffFun(x, t=0, D=0.01):
        return D * np.ones([len(x), 1])

    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    with pytest.raises(NotImplementedError, match='periodic boundaries with model-order reduction'):
        ADPDE(Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x), MORvar=mor,
              periodic=[(0, 1)])


# ---- VarNet: the paired rows -------------------------------------------------------------------------------------------------
def test_periodic_rows_1d():
    # time-dependent: the two ends paired with the time nodes, shifted by b - a = 1; no Dirichlet row is left
    vn = VarNet(pde1d([(0, 1)]), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4)
    r = vn.periodicRows
    t = vn.timeDisc()[1]
    assert r['pairs'] == [(0, 1, 4)] and r['X'].shape == (8, 2) and r['dir'].shape == (8, 1)
    np.testing.assert_array_equal(r['X'][:4], np.hstack([np.zeros((4, 1)), np.reshape(t, (4, 1))]))
    np.testing.assert_array_equal(r['X'][4:] - r['X'][:4], np.tile([1.0, 0.0], (4, 1)))
    np.testing.assert_array_equal(r['dir'], -np.ones((8, 1)))           # the outward normal of side A, on both sides
    assert vn.fixData.bDofsum == 0 and vn.fixData.biDof == [8]          # the initial slice alone
    X, d, gamma, bdv = vn.engine.per                                    # registered once, with the domain measure as biDimVal
    np.testing.assert_array_equal(X, r['X'])
    assert gamma == 1.0 and bdv == vn.fixData.biDimVal and vn.periodicDeriv == 1.0
    # the pair given the other way round: side A is the right end
    r = VarNet(pde1d([(1, 0)]), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, periodicDeriv=0.25).periodicRows
    np.testing.assert_array_equal(r['X'][:4, 0], np.ones(4))
    np.testing.assert_array_equal(r['X'][4:] - r['X'][:4], np.tile([-1.0, 0.0], (4, 1)))
    np.testing.assert_array_equal(r['dir'], np.ones((8, 1)))
    # steady: one pair of points
    vn = VarNet(pde1d([(0, 1)], t=False), layerWidth=[5], discNum=8, bDiscNum=None, periodicDeriv=0.0)
    r = vn.periodicRows
    assert r['pairs'] == [(0, 1, 1)]
    np.testing.assert_array_equal(r['X'], [[0.0], [1.0]])
    np.testing.assert_array_equal(r['dir'], [[-1.0], [-1.0]])
    assert vn.engine.per[2] == 0.0 and vn.periodicDeriv == 0.0


def test_periodic_rows_unit_square_both_orientations():
    """(left, right) paired, top and bottom Dirichlet, for a counter-clockwise and a clockwise vertex list: the same rows."""
    out = []
    for verts, pair, dirichlet in ((SQUARE, (3, 1), [0, 2]), (SQUARE_CW, (0, 2), [1, 3])):
        vn = VarNet(pde2d([pair], vertices=verts), layerWidth=[5], discNum=[6, 5], bDiscNum=7, tDiscNum=3)
        r = vn.periodicRows
        mesh = vn.PDE.domain.getMesh(vn.discNum, vn.bDiscNum)
        t = vn.timeDisc()[1]
        n = mesh.bdof[pair[0]] * 3
        assert r['pairs'] == [(pair[0], pair[1], n)] and r['X'].shape == (2 * n, 3)
        np.testing.assert_array_equal(r['X'][:n], uf.pairMats(mesh.bCoordinates[pair[0]], t))
        np.testing.assert_array_equal(r['X'][n:] - r['X'][:n], np.tile([1.0, 0.0, 0.0], (n, 1)))     # X_B - X_A == s, exactly
        np.testing.assert_array_equal(r['dir'], np.tile([-1.0, 0.0], (2 * n, 1)))
        # side B lies on edge B, but not in the order of its own boundary points (the edges run in opposite senses)
        xb = np.asarray(uf.pairMats(mesh.bCoordinates[pair[1]], t))
        key = lambda a: a[np.lexsort(np.round(a, 9).T[::-1])]
        np.testing.assert_allclose(key(r['X'][n:]), key(xb), rtol=0, atol=1e-14)
        assert np.max(np.abs(r['X'][n:] - xb)) > 0.1
        # the Dirichlet rows are those of top and bottom alone
        assert vn.fixData.bDofsum == sum(mesh.bdof[b] for b in dirichlet) * 3
        order = np.lexsort(np.round(r['X'][:n], 9).T[::-1])
        out.append((r['X'][:n][order], r['X'][n:][order]))
    for a, b in zip(out[0], out[1]):                                     # both vertex orders: the same pairs (1 - y against y:
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-14)             # to the rounding of the edge's own parametrisation)


def test_flux_and_dirichlet_rows_exclude_the_pair():
    BCs = [[], [], [2.0, 0.0, g0], []]                                   # bottom Dirichlet, top Neumann, left and right paired
    vn = VarNet(pde2d([(3, 1)], BCs=BCs), layerWidth=[5], discNum=[6, 5], bDiscNum=7, tDiscNum=3, fluxBC=True)
    mesh = vn.PDE.domain.getMesh(vn.discNum, vn.bDiscNum)
    assert [(b, k) for b, k, _ in vn.fluxRows['edges']] == [(2, 'Neumann')]
    assert vn.fluxRows['X'].shape[0] == mesh.bdof[2] * 3 == vn.engine.flux.shape[0]
    assert vn.fixData.bDofsum == mesh.bdof[0] * 3
    bi = vn.fixData.uniform_biInput[:vn.fixData.bDofsum]
    np.testing.assert_array_equal(bi[:, 1], np.zeros(len(bi)))          # every Dirichlet row lies on the bottom edge
    assert vn.periodicRows['pairs'] == [(3, 1, mesh.bdof[3] * 3)]


def test_periodic_deriv_refusals():
    for kw in ({'periodicDeriv': 1.0}, {'periodicDeriv': 0.0}):
        with pytest.raises(ValueError, match='periodicDeriv=.* is an option of a PDE with periodic boundaries'):
            VarNet(pde1d(None), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, **kw)
    for bad in (-1.0, float('nan'), float('inf'), 'x', [1.0], True):
        with pytest.raises(ValueError, match='periodicDeriv=.* must be a finite number >= 0'):
            VarNet(pde1d([(0, 1)]), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=4, periodicDeriv=bad)


def _case_lines(path):
    return [ln for ln in open(path).read().splitlines(True) if not ln.startswith('Simulation date')]


def test_without_periodic_nothing_changes(tmp_path):
    """No pair: no rows, no registration, and the training data, the case file and two epochs are those of a PDE built without
    the keyword."""
    outs = []
    for i, kw in enumerate(({}, {'periodic': None})):
        np.random.seed(0)
        pde = ADPDE(PolygonDomain2D(SQUARE), diff=0.1, vel=[1.0, 0.0], tInterval=[0, 1.0], IC=IC2, **kw)
        vn = VarNet(pde, layerWidth=[5], discNum=[6, 5], bDiscNum=7, tDiscNum=4)
        assert vn.periodicRows is None and vn.periodicDeriv is None and vn.engine.per is None
        td = vn._build_tdata()
        res = vn.train(str(tmp_path / str(i)), epochNum=2, saveFreq=1, verbose=False)
        outs.append((td.mor[0], _case_lines(str(tmp_path / str(i) / 'caseData.txt')), res.lossAll, vn.engine.get_params()))
    (a, ca, la, pa), (b, cb, lb, pb) = outs
    for k in ('Input', 'gcoef', 'biInput', 'biLabel'):
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]))
    assert ca == cb and not any('periodic' in ln.lower() for ln in ca)
    assert la == lb
    np.testing.assert_array_equal(pa, pb)
    # ... and with a pair, caseData.txt names it with its row count
    vn = VarNet(pde2d([(3, 1)]), layerWidth=[5], discNum=[6, 5], bDiscNum=7, tDiscNum=4, periodicDeriv=0.5)
    vn.train(str(tmp_path / 'on'), epochNum=1, saveFreq=1, verbose=False)
    lines = [ln for ln in open(str(tmp_path / 'on' / 'caseData.txt')) if 'periodic pair' in ln]
    assert lines == ['\tBC4 and BC2: periodic pair enforced on %d rows each, derivative weight 0.5\n' % vn.periodicRows['pairs'][0][2]]


def test_bc_component_is_dirichlet_mean_plus_periodic_mean():
    vn = VarNet(pde2d([(3, 1)]), layerWidth=[6, 4], discNum=[6, 5], bDiscNum=7, tDiscNum=4, periodicDeriv=2.0)
    eng = vn.engine
    eng.set_params(eng.get_params() + 0.1)
    td = vn._build_tdata()
    comp, _, _ = vn.splitLoss(td)
    kept = eng.per
    eng.set_periodic(None)                                              # Dirichlet mean alone: the same engine without its pairs
    comp0, _, _ = vn.splitLoss(td)
    eng.per = kept
    r = vn.periodicRows
    P, _, r0, r1 = periodic_ref.periodic_term(eng.theta, vn.inpDim, vn.layerWidth, vn.dim, r['X'], r['dir'], 2.0, vn.fixData.biDimVal)
    assert P > 1e-3 * comp0[0, 0]
    np.testing.assert_allclose(comp[0, 0], comp0[0, 0] + P, rtol=1e-12)
    np.testing.assert_allclose(comp[1:], comp0[1:], rtol=1e-12)
    # the jumps themselves, by hand on one pair: u and -du/dx (the direction is the left edge's normal) by central differences
    n = len(r0)
    i = n - 1
    fwd = lambda z: float(eng.forward(z)[0])
    h = 1e-6
    ux = []
    for row in (i, i + n):
        xp, xm = r['X'][row:row + 1].copy(), r['X'][row:row + 1].copy()
        xp[0, 0] += h
        xm[0, 0] -= h
        ux.append((fwd(xp) - fwd(xm)) / (2 * h))
    assert abs(r0[i] - (fwd(r['X'][i:i + 1]) - fwd(r['X'][i + n:i + n + 1]))) < 1e-14
    assert abs(r1[i] - (-(ux[0] - ux[1]))) < 1e-8


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entry_point():
    import ctypes as C
    from varnet_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'int\s+vn_set_periodic\s*\(\s*vn_engine\s*\*\s*h\s*,\s*const\s+float\s*\*\s*X_dev\s*,\s*const\s+float\s*\*\s*dir_dev\s*,'
                     r'\s*int64_t\s+nP\s*,\s*double\s+gamma\s*,\s*double\s+biDimVal\s*\)\s*;', code)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr)            # additive: the version stays
    assert 'vn_set_periodic' in engine.ABI_SYMBOLS
    res, args = engine._SIGS['vn_set_periodic']
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double]
    assert callable(getattr(engine.VNEngine, 'set_periodic'))


# ---- the restatement checks itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gamma', [0.0, 1.0, 3.5])
def test_reference_gradient_against_central_differences(gamma):
    d_in, dim, widths, nP = 3, 2, [5], 7
    rng = np.random.default_rng(4)
    flat = og.glorot_init(d_in, widths, 1).astype(np.float64) + 0.3 * rng.standard_normal(og.param_count(d_in, widths))
    X = rng.uniform(-1, 1, (2 * nP, d_in))
    n = rng.standard_normal((nP, dim))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = np.vstack([n, n])
    P, g, r0, r1 = periodic_ref.periodic_term(flat, d_in, widths, dim, X, d, gamma, 2.0, 'tanh')
    assert P > 0 and r0.shape == r1.shape == (nP,)
    np.testing.assert_allclose(P, np.mean(2.0 * (r0 ** 2 + gamma * r1 ** 2)), rtol=1e-14)
    h = 1e-6
    fd = np.zeros_like(flat)
    for p in range(flat.size):
        e = np.zeros_like(flat)
        e[p] = h
        fd[p] = (periodic_ref.periodic_term(flat + e, d_in, widths, dim, X, d, gamma, 2.0, 'tanh')[0]
                 - periodic_ref.periodic_term(flat - e, d_in, widths, dim, X, d, gamma, 2.0, 'tanh')[0]) / (2 * h)
    err = np.max(np.abs(fd - g)) / np.max(np.abs(g))
    print('periodic_ref gamma %g: gradient vs central differences, relative error %.3e' % (gamma, err))
    assert err <= 1e-6
    # swapping the two sides of every pair changes the sign of both jumps and nothing else
    Xs = np.vstack([X[nP:], X[:nP]])
    Ps, gs, r0s, r1s = periodic_ref.periodic_term(flat, d_in, widths, dim, Xs, d, gamma, 2.0, 'tanh')
    np.testing.assert_allclose(Ps, P, rtol=1e-14)
    np.testing.assert_allclose(r0s, -r0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(gs, g, rtol=1e-12, atol=1e-15)
