"""
CPU tier of the boundary-flux term (`VarNet(fluxBC=True)`, vn_set_flux_bc): outward normals of the domains, host assembly of
the flux rows, the flag's default leaving everything as it was, the BC component through a stand-in engine (the oracle engine
plus the fp64 restatement of tests/flux_ref.py), and the MOR refusal.
"""
import numpy as np
import pytest

from tests import flux_ref
from tests.oracle_engine import OracleEngine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D, PolygonDomain2D
from varnet_amd.mor import MOR
from varnet_amd.utility import UF
from varnet_amd.varnet import VarNet

uf = UF()
pi = np.pi


class FluxOracleEngine(OracleEngine):
    """The oracle engine with vn_set_flux_bc: the flux mean of tests/flux_ref.py added to the BC component, w0 times it to the
    loss and the gradient."""
    flux = None

    def set_flux_bc(self, X=None, normal=None, coef=None, label=None, biDimVal=1.0):
        if X is None or len(X) == 0:
            self.flux = None
            return
        self.flux = (np.array(X, dtype=float), np.array(normal, dtype=float), np.reshape(coef, -1).astype(float),
                     np.reshape(label, -1).astype(float), float(biDimVal))

    def _eval(self, batch):
        res, g = super()._eval(batch)
        if self.flux is None:
            return res, g
        X, n, c, lab, bdv = self.flux
        F, gF, _ = flux_ref.flux_term(self.theta.astype(np.float64), self.inpDim, self.layerWidth, self.dim, X, n, c, lab, bdv)
        res = dict(res)
        res['BCloss'] = res['BCloss'] + F
        res['loss'] = res['loss'] + self.w[0] * F
        return res, g + self.w[0] * gF


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return FluxOracleEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                                isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                                learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


SQUARE = np.array([[0., 0.], [1., 0.], [1., 1.], [0., 1.]])


def test_boundary_normals():
    np.testing.assert_array_equal(Domain1D(np.array([0.0, 1.0])).boundaryNormals(), [[-1.0], [1.0]])
    ccw = [[0, -1], [1, 0], [0, 1], [-1, 0]]                         # bottom, right, top, left
    np.testing.assert_allclose(PolygonDomain2D(SQUARE).boundaryNormals(), ccw, atol=1e-15)
    cw = SQUARE[[0, 3, 2, 1]]                                        # left, top, right, bottom
    np.testing.assert_allclose(PolygonDomain2D(cw).boundaryNormals(), [[-1, 0], [0, 1], [1, 0], [0, -1]], atol=1e-15)
    rect = np.array([[0., 0.], [2., 0.], [2., 1.], [0., 1.]])
    obs = np.array([[0.5, 0.25], [1.0, 0.25], [1.0, 0.75], [0.5, 0.75]])     # counter-clockwise obstacle
    got = PolygonDomain2D(rect, [obs]).boundaryNormals()
    # outer walls outward; obstacle edges point out of the computational domain, into the obstacle
    want = ccw + [[0, 1], [-1, 0], [0, -1], [1, 0]]
    np.testing.assert_allclose(got, want, atol=1e-15)
    # the same obstacle listed clockwise: edges top, right, bottom, left
    np.testing.assert_allclose(PolygonDomain2D(rect, [obs[::-1]]).boundaryNormals()[4:], [[0, -1], [-1, 0], [0, 1], [1, 0]],
                               atol=1e-15)


def gN(x, t):
    return np.reshape(np.sin(x[:, 0:1]) * (1 + t), [-1, 1])


def gR(x, t):
    return np.reshape(x[:, 1:2] ** 2 + t, [-1, 1])


def pde2dt(BCs):
    return ADPDE(PolygonDomain2D(SQUARE), diff=0.1, vel=[1.0, 0.0], tInterval=[0, 1.0], BCs=BCs,
                 IC=lambda x: np.sin(pi * x[:, 0:1]))


def test_flux_rows_2dt():
    # bottom: Dirichlet; right: Neumann (a = 2, g = gN); top: Dirichlet; left: Robin (a = 0.5, b = 1.5, g = gR)
    vn = VarNet(pde2dt([[], [2.0, 0.0, gN], [], [0.5, 1.5, gR]]), layerWidth=[5], discNum=[6, 5], bDiscNum=7, tDiscNum=4,
                fluxBC=True)
    r = vn.fluxRows
    mesh = vn.PDE.domain.getMesh(vn.discNum, vn.bDiscNum)
    t = vn.timeDisc()[1]
    assert [(b, k) for b, k, _ in r['edges']] == [(1, 'Neumann'), (3, 'Robin')]
    assert r['X'].shape[0] == (mesh.bdof[1] + mesh.bdof[3]) * 4 == sum(n for _, _, n in r['edges'])
    n1 = mesh.bdof[1] * 4
    X1, X3 = r['X'][:n1], r['X'][n1:]
    np.testing.assert_array_equal(X1, uf.pairMats(mesh.bCoordinates[1], t))
    np.testing.assert_array_equal(X3, uf.pairMats(mesh.bCoordinates[3], t))
    np.testing.assert_array_equal(r['normal'][:n1], np.tile([1.0, 0.0], (n1, 1)))
    np.testing.assert_array_equal(r['normal'][n1:], np.tile([-1.0, 0.0], (len(X3), 1)))
    np.testing.assert_array_equal(r['coef'], np.r_[np.zeros(n1), np.full(len(X3), 3.0)])
    np.testing.assert_allclose(r['label'][:n1], np.sin(X1[:, 0]) * (1 + X1[:, 2]) / 2.0, rtol=1e-15)
    np.testing.assert_allclose(r['label'][n1:], (X3[:, 1] ** 2 + X3[:, 2]) / 0.5, rtol=1e-15)
    # registered once, with the domain measure as biDimVal
    X, nrm, c, lab, bdv = vn.engine.flux
    np.testing.assert_array_equal(X, r['X'])
    assert bdv == vn.fixData.biDimVal


def _case_lines(path):
    return [ln for ln in open(path).read().splitlines(True) if not ln.startswith('Simulation date')]


def test_flag_off_changes_nothing(tmp_path):
    BCs = [[], [2.0, 0.0, gN], [], [0.5, 1.5, gR]]
    outs = []
    for i, kw in enumerate(({}, {'fluxBC': False})):
        np.random.seed(0)
        vn = VarNet(pde2dt(BCs), layerWidth=[5], discNum=[6, 5], bDiscNum=7, tDiscNum=4, **kw)
        assert vn.fluxRows is None and vn.engine.flux is None
        td = vn._build_tdata()
        res = vn.train(str(tmp_path / str(i)), epochNum=2, saveFreq=1, verbose=False)
        outs.append((td.mor[0], _case_lines(str(tmp_path / str(i) / 'caseData.txt')), res.lossAll, vn.engine.get_params()))
    (a, ca, la, pa), (b, cb, lb, pb) = outs
    for k in ('Input', 'gcoef', 'biInput', 'biLabel'):
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]))
    assert ca == cb and not any('flux' in ln for ln in ca)
    assert la == lb
    np.testing.assert_array_equal(pa, pb)
    # ... and with the flag on, caseData.txt names each enforced flux boundary with its row count
    vn = VarNet(pde2dt(BCs), layerWidth=[5], discNum=[6, 5], bDiscNum=7, tDiscNum=4, fluxBC=True)
    vn.train(str(tmp_path / 'on'), epochNum=1, saveFreq=1, verbose=False)
    lines = [ln for ln in open(str(tmp_path / 'on' / 'caseData.txt')) if 'boundary flux term' in ln]
    n = {b: k for b, _, k in vn.fluxRows['edges']}
    assert lines == ['\tBC2: Neumann condition enforced as a boundary flux term on %d rows\n' % n[1],
                     '\tBC4: Robin condition enforced as a boundary flux term on %d rows\n' % n[3]]


def test_bc_component_is_dirichlet_mean_plus_flux_mean():
    BCs = [[], [2.0, 0.0, gN], [], [0.5, 1.5, gR]]
    vn = VarNet(pde2dt(BCs), layerWidth=[6, 4], discNum=[6, 5], bDiscNum=7, tDiscNum=4, fluxBC=True)
    eng = vn.engine
    eng.set_params(eng.get_params() + 0.1)
    td = vn._build_tdata()
    comp, _, _ = vn.splitLoss(td)
    # Dirichlet mean alone: the same engine without its flux rows
    kept = eng.flux
    eng.set_flux_bc(None)
    comp0, _, _ = vn.splitLoss(td)
    eng.flux = kept
    r = vn.fluxRows
    F, _, res = flux_ref.flux_term(eng.theta, vn.inpDim, vn.layerWidth, vn.dim, r['X'], r['normal'], r['coef'], r['label'],
                                   vn.fixData.biDimVal)
    assert F > 1e-3 * comp0[0, 0]
    np.testing.assert_allclose(comp[0, 0], comp0[0, 0] + F, rtol=1e-12)
    np.testing.assert_allclose(comp[1:], comp0[1:], rtol=1e-12)
    # the residual itself, by hand on one Robin row: n . grad_x u + (b/a) u - g/a with a central difference for grad_x u
    i = len(res) - 1
    x = r['X'][i:i + 1].copy()
    h = 1e-6
    xp, xm = x.copy(), x.copy()
    xp[0, 0] += h
    xm[0, 0] -= h
    fwd = lambda z: float(eng.forward(z)[0])
    ux = (fwd(xp) - fwd(xm)) / (2 * h)
    assert abs(res[i] - (-ux + 3.0 * fwd(x) - r['label'][i])) < 1e-6


def test_mor_with_flux_raises():
    def diffFun(x, t=0, D=0.01):
        return D * np.ones([len(x), 1])

    def disc():
        return np.array([[0.003], [0.03]])

    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    pde = ADPDE(Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], BCs=[[], [1.0, 0.0, 0.0]],
                IC=lambda x: -np.sin(pi * x), MORvar=mor)
    with pytest.raises(NotImplementedError, match='model-order reduction'):
        VarNet(pde, layerWidth=[5, 5], discNum=5, bDiscNum=None, tDiscNum=6, MORdiscScheme=disc, fluxBC=True)
