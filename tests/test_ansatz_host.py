"""
CPU tier of the hard-constraint ansatz u = A + B n (vn_set_ansatz, `ADPDE(ansatz={...})`).

The restatement tests/ansatz_ref.py is pinned three ways: against direct torch autograd of a composite A(x,t) + B(x,t) net(x,t)
with analytic A and B (1e-12), against central differences of its own loss (1e-7 of the gradient's scale, as
tests/test_nldiff_host.py does), and against the references it restates with A = 0, B = 1 (bit for bit).  From the fp64
reference alone: A alone and B alone each move everything the GPU parity tests compare by at least 100 x the bar it is
compared at.  Then the host layer without a device: the entry points are declared and bound, `ADPDE(ansatz=...)` checks its
arguments and the gradients, `VarNet._assemble` contracts dA, dB with the gcoef it uploads, `evaluate()` and `residual()` see
the constrained solution, and every refusal that needs no device raises.
"""
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests import ansatz_cases as ac
from tests import ansatz_ref, flux_ref, nldiff_ref, obs_ref, periodic_ref
from tests.ansatz_cases import CASES, IDS
from tests.gradcheck import block_errors
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL
from tests.test_nldiff_host import NldiffOracleEngine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pi = np.pi


# ---- the reference, pinned three ways ---------------------------------------------------------------------------------
def A_t(X, dim):
    """A = sin(pi x0) [sin(pi x1)] cos t as a torch function of the rows X = [x, t]."""
    a = torch.cos(X[:, dim])
    for d in range(dim):
        a = a * torch.sin(pi * X[:, d])
    return a


def B_t(X, dim):
    """B = t (1 - x0^2) [(1 - x1^2)] + 0.2"""
    b = X[:, dim]
    for d in range(dim):
        b = b * (1.0 - X[:, d] ** 2)
    return b + 0.2


@pytest.mark.parametrize('i', [1, 3], ids=['1d+t', '2d+t'])
def test_reference_against_autograd_of_the_composite(i):
    """tests/nldiff_ref.loss_fun run on the composite model A(x,t) + B(x,t) net(x,t) itself (the oracle's model and model_grad
    replaced by the composite, its gradient by autograd through A and B) against tests/ansatz_ref.py fed the four streams."""
    d_in, dim, widths = CASES[i][0], CASES[i][1], CASES[i][2]
    kw = ac.ref_kw(i)
    model, model_grad = og.model, og.model_grad

    def comp_model(params, X, activation='sigmoid'):
        return (A_t(X, dim) + B_t(X, dim) * model(params, X, activation)[:, 0]).reshape(-1, 1)

    def comp_model_grad(params, Input, dim_, time_dependent=True, need_hess=False, activation='sigmoid'):
        u = comp_model(params, Input, activation)
        g = torch.autograd.grad(u.sum(), Input, create_graph=True)[0]
        return u, g[:, :dim_], None, None

    with mock.patch.object(og, 'model', comp_model), mock.patch.object(og, 'model_grad', comp_model_grad):
        want, gwant = nldiff_ref.loss_and_grad(ac.theta(i).astype(np.float64), d_in, widths, (None, nldiff_ref.ONE), None, None,
                                               torch.float64, **kw)

    def streams(X, G):
        Xt = torch.as_tensor(X, dtype=torch.float64).clone().requires_grad_(True)
        A, B = A_t(Xt, dim), B_t(Xt, dim)
        z = dict(A=A.detach().numpy(), B=B.detach().numpy(), a=None, b=None)
        if G is not None:
            z['a'] = (torch.autograd.grad(A.sum(), Xt)[0][:, :dim].numpy() * G).sum(1)
            z['b'] = (torch.autograd.grad(B.sum(), Xt)[0][:, :dim].numpy() * G).sum(1)
        return z

    az = dict(int=streams(kw['Input'], kw['gcoef']), bic=streams(kw['biInput'], None))
    got, ggot = ansatz_ref.loss_and_grad(ac.theta(i).astype(np.float64), d_in, widths, az, **kw)
    for k in ('loss', 'BCloss', 'ICloss', 'varLoss'):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    assert np.max(np.abs(got['lossVec'] - want['lossVec'])) <= 1e-12 * np.max(np.abs(want['lossVec']))
    assert np.max(np.abs(ggot - gwant)) <= 1e-12 * np.max(np.abs(gwant))
    assert abs(want['loss'] - nldiff_ref.loss_and_grad(ac.theta(i).astype(np.float64), d_in, widths, (None, nldiff_ref.ONE), None, None,
                                                       torch.float64, **kw)[0]['loss']) > 1e-3 * abs(want['loss'])   # the composite is in play


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_reference_gradient_against_central_differences(i):
    """6 sampled coordinates agree with central differences of the reference's own loss to 1e-7 of the gradient's largest entry,
    and each to 1e-4 of itself (coordinates with |g| < 1e-8 are not judged there)."""
    ref, g = ac.reference64(i)
    flat = ac.theta(i).astype(np.float64)
    h = 1e-5
    judged = 0
    for p in np.random.default_rng(7).choice(flat.size, 6, replace=False):
        if abs(g[p]) < 1e-8:
            continue
        e = np.zeros_like(flat)
        e[p] = h
        fd = (ac.reference(i, flat=flat + e)[0]['loss'] - ac.reference(i, flat=flat - e)[0]['loss']) / (2 * h)
        print('case %s coordinate %d: autograd %.6e, central difference %.6e' % (IDS[i], p, g[p], fd))
        assert abs(fd - g[p]) <= 1e-7 * np.max(np.abs(g)), (IDS[i], p, g[p], fd, np.max(np.abs(g)))
        assert abs(fd - g[p]) <= 1e-4 * abs(g[p]), (IDS[i], p, g[p], fd)
        judged += 1
    assert judged >= 3


def unit(n, deriv=True):
    z = dict(A=np.zeros(n), B=np.ones(n), a=None, b=None)
    if deriv:
        z['a'], z['b'] = np.zeros(n), np.zeros(n)
    return z


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_unit_ansatz_is_the_underlying_reference_exactly(i):
    """A = 0, B = 1, a = b = 0: tests/nldiff_ref.py's result bit for bit."""
    d_in, widths, q, n_k = CASES[i][0], CASES[i][2], CASES[i][3], CASES[i][4]
    kw = ac.ref_kw(i)
    flat = ac.theta(i).astype(np.float64)
    want, gwant = nldiff_ref.loss_and_grad(flat, d_in, widths, (None, nldiff_ref.ONE), None, None, torch.float64, **kw)
    got, ggot = ansatz_ref.loss_and_grad(flat, d_in, widths, dict(int=unit(n_k * q), bic=unit(kw['biInput'].shape[0], False)), **kw)
    for k in ('loss', 'BCloss', 'ICloss', 'varLoss'):
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(got['lossVec'], want['lossVec']) and np.array_equal(ggot, gwant)


@pytest.mark.parametrize('kind', ac.EDGE_KINDS)
def test_unit_ansatz_on_an_edge_set_is_its_reference_exactly(kind):
    """... and the edge sets' restatements those of tests/flux_ref.py, tests/periodic_ref.py and tests/obs_ref.py."""
    i = ac.EDGE_CASE
    d_in, dim, widths, act = CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][8]
    name, reg, z = ac.edge(kind, 33)
    flat = ac.theta(i).astype(np.float64)
    f64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in reg.items()}
    if name == 'flux':
        want, gwant, _ = flux_ref.flux_term(flat, d_in, widths, dim, f64['X'], f64['normal'], f64['coef'], f64['label'], ac.BIDIMVAL, act)
        term = lambda p, zz: ansatz_ref.flux_term(p, dim, f64['X'], f64['normal'], f64['coef'], f64['label'], ac.BIDIMVAL, act, torch.float64, zz)
    elif name == 'periodic':
        want, gwant = periodic_ref.periodic_term(flat, d_in, widths, dim, f64['X'], f64['dir'], f64['gamma'], ac.BIDIMVAL, act)[:2]
        term = lambda p, zz: ansatz_ref.periodic_term(p, dim, f64['X'], f64['dir'], f64['gamma'], ac.BIDIMVAL, act, torch.float64, zz)
    else:
        args = (f64['X'], f64['value'], f64.get('q'), f64.get('dir'), f64.get('rowptr'), f64.get('wgt'))
        want, gwant, _ = obs_ref.obs_term(flat, d_in, widths, dim, *args, activation=act)
        term = lambda p, zz: ansatz_ref.obs_term(p, dim, *args, act, torch.float64, zz)
    for zz in (None, unit(len(z['B']), z['a'] is not None)):
        params = og.unflatten(flat, d_in, widths, dtype=torch.float64, requires_grad=True)
        got = term(params, zz)
        got.backward()
        assert float(got.detach()) == want and np.array_equal(og.flatten_grads(params).detach().numpy(), gwant), (kind, zz is None)


# ---- the inputs -------------------------------------------------------------------------------------------------------
def moved(i, ra_ga, rb_gb):
    (ra, ga), (rb, gb) = ra_ga, rb_gb
    lv = np.max(np.abs(ra['lossVec'] - rb['lossVec'])) / np.max(np.abs(ra['lossVec']))
    blocks = block_errors(gb, ga, CASES[i][0], CASES[i][2], CASES[i][1], CASES[i][7])
    return (abs(ra['loss'] - rb['loss']) / abs(ra['loss']), abs(ra['varLoss'] - rb['varLoss']) / abs(ra['varLoss']), float(lv),
            min(blocks.values()))


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_inputs_make_a_missing_stream_fail(i):
    """A condition on the INPUTS, from the fp64 reference alone: A alone (against A = 0, a = 0) and B alone (against B = 1, b = 0)
    each move the loss and varLoss by >= 100 LOSS_RTOL, lossVec by >= 100 LVEC_RTOL of its maximum and EVERY parameter tensor of the
    gradient by >= 100 GRAD_RTOL of its own size; on the BC/IC rows each moves the BC component likewise."""
    az = ac.ansatz(i)
    n, nB = CASES[i][3] * CASES[i][4], CASES[i][5]
    zero, one = np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32)
    without = {'A': dict(az, int=dict(az['int'], A=zero, a=zero)), 'B': dict(az, int=dict(az['int'], B=one, b=zero))}
    for name, other in without.items():
        dl, dv, lv, blk = moved(i, ac.reference64(i), ac.reference(i, other))
        print('ansatz inputs %s, %s alone: loss %.3g varLoss %.3g lossVec %.3g least-moved gradient tensor %.3g' % (IDS[i], name, dl, dv, lv, blk))
        assert dl >= 100 * LOSS_RTOL and dv >= 100 * LOSS_RTOL, (name, dl, dv)
        assert lv >= 100 * LVEC_RTOL, (name, lv)
        assert blk >= 100 * GRAD_RTOL, (name, blk)
    bic = {'A': dict(az['bic'], A=np.zeros(nB, dtype=np.float32)), 'B': dict(az['bic'], B=np.ones(nB, dtype=np.float32))}
    ref = ac.reference64(i)[0]
    for name, z in bic.items():
        other = ac.reference(i, dict(az, bic=z))[0]
        assert abs(other['BCloss'] - ref['BCloss']) >= 100 * LOSS_RTOL * abs(ref['BCloss']), (name, other['BCloss'], ref['BCloss'])
    assert np.all(np.isfinite(ac.reference64(i)[1]))


# ---- the ABI and the binding --------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound():
    from varnet_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    for name in ('vn_set_ansatz', 'vn_set_ansatz_points', 'vn_set_ansatz_rows'):
        assert re.search(r'\bint %s\(vn_engine\* h, int32_t' % name, hdr) and name in engine.ABI_SYMBOLS
    assert re.search(r'VN_ANSATZ_BIC = 0, VN_ANSATZ_FLUX = 1, VN_ANSATZ_PERIODIC = 2, VN_ANSATZ_OBS = 3', hdr)
    assert {k: v[0] for k, v in engine.ANSATZ_SETS.items()} == {'bic': 0, 'flux': 1, 'periodic': 2, 'obs': 3}
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr)
    mk = open(os.path.join(ROOT, 'varnet_amd', 'csrc', 'Makefile')).read()
    assert 'vn_ansatz.hip' in mk and 'vn_ansatz.h' in mk
    assert 'vn_ansatz' not in open(os.path.join(ROOT, 'varnet_amd', 'csrc', 'vn_internal.h')).read()


# ---- ADPDE ------------------------------------------------------------------------------------------------------------
def Afun(x, t=0):
    return np.sin(pi * x)


def Bfun(x, t=0):
    return t * (1.0 - x ** 2)


AZ = dict(A=Afun, B=Bfun, dA=lambda x, t=0: pi * np.cos(pi * x), dB=lambda x, t=0: -2.0 * x * t)
AZ_FULL = dict(AZ, A_t=lambda x, t=0: np.zeros_like(x), B_t=lambda x, t=0: 1.0 - x ** 2, lapA=lambda x, t=0: -pi ** 2 * np.sin(pi * x),
               lapB=lambda x, t=0: -2.0 * t * np.ones_like(x))


def _pde(ansatz=AZ, **kw):
    kw.setdefault('tInterval', [0, 1.0])
    kw.setdefault('IC', lambda x: np.sin(pi * x))
    return ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, vel=0.0, ansatz=ansatz, **kw)


def test_adpde_ansatz_argument():
    assert not hasattr(_pde(None), 'ansatz') and sorted(_pde().ansatz) == ['A', 'B', 'dA', 'dB'] and len(_pde(AZ_FULL).ansatz) == 8
    for bad in ('A', [Afun, Bfun], dict(A=Afun, B=Bfun, dA=AZ['dA']), dict(AZ, B=1.0), dict(AZ, lapA=3.0), dict(AZ, C=Afun)):
        with pytest.raises(ValueError):
            _pde(bad)
    with pytest.raises(ValueError, match='must return one value per point'):
        _pde(dict(AZ, A=lambda x, t=0: np.hstack([x, x])))
    with pytest.raises(ValueError, match='finite'):
        _pde(dict(AZ, B=lambda x, t=0: np.full_like(x, np.inf)))


def test_construction_checks_the_gradients():
    """dA / dB against fp64 central differences at 64 seeded points, 1e-6 relative: a wrong sign, a missing factor and a gradient
    that forgot the time factor are refused; an error below the tolerance is not."""
    for key, wrong in (('dA', lambda x, t=0: -pi * np.cos(pi * x)), ('dA', lambda x, t=0: np.cos(pi * x)), ('dB', lambda x, t=0: -2.0 * x),
                       ('dB', lambda x, t=0: -2.0 * x * t * (1.0 + 1e-5))):
        with pytest.raises(ValueError, match="ansatz\\['%s'\\] is not the spatial gradient" % key):
            _pde(dict(AZ, **{key: wrong}))
    _pde(dict(AZ, dB=lambda x, t=0: -2.0 * x * t * (1.0 + 1e-8)))
    # a steady 1D problem: the callables take x alone
    ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, vel=0.0, ansatz=dict(A=lambda x: 0.5 * x, B=lambda x: 1.0 - x ** 2,
                                                                          dA=lambda x: 0.5 * np.ones_like(x), dB=lambda x: -2.0 * x))


def test_mor_with_ansatz_raises():
    def srcFun(x, t=0, a=1.0):
        return a * np.ones([len(x), 1])
    mor = MOR([srcFun], [['a']], [[[0.5, 1.5]]])
    with pytest.raises(NotImplementedError, match='model-order reduction'):
        ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, vel=0.0, source=srcFun, tInterval=[0, 1.0], IC=lambda x: np.sin(pi * x), MORvar=mor,
              ansatz=AZ)


# ---- VarNet host layer through a stand-in engine ------------------------------------------------------------------------
class AnsatzOracleEngine(NldiffOracleEngine):
    """The stand-in engine of tests/test_nldiff_host.py with the three ansatz registrations (kept as fp64 arrays)."""

    def _np(self, streams):
        return tuple(None if s is None else np.array(s.numpy() if isinstance(s, torch.Tensor) else s, dtype=float) for s in streams)

    def set_interior(self, batch, *a, **kw):
        super().set_interior(batch, *a, **kw)
        self.__dict__.setdefault('az', {}).pop(batch, None)
        self.__dict__.setdefault('azp', {}).pop(batch, None)

    def set_ansatz(self, batch, A=None, B=None, a=None, b=None):
        self.__dict__.setdefault('az', {})[batch] = self._np((A, B, a, b))

    def set_ansatz_points(self, batch, A=None, B=None, gA=None, gB=None):
        self.__dict__.setdefault('azp', {})[batch] = self._np((A, B, gA, gB))

    def set_ansatz_rows(self, which, A=None, B=None, a=None, b=None):
        self.__dict__.setdefault('azr', {})[which] = self._np((A, B, a, b))

    def forward(self, X):
        X = np.asarray(X.numpy() if isinstance(X, torch.Tensor) else X, dtype=np.float64)
        return torch.as_tensor(og.forward(self.theta.astype(np.float64), self.inpDim, self.layerWidth, torch.float64, X)[:, 0])

    def forward_grad(self, X):
        X = np.asarray(X.numpy() if isinstance(X, torch.Tensor) else X, dtype=np.float64)
        u, g = nldiff_ref.value_and_grad(self.theta.astype(np.float64), self.inpDim, self.layerWidth, torch.float64, X, self.dim, self.td)
        return torch.as_tensor(u[:, 0]), torch.as_tensor(g)


@pytest.fixture
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return AnsatzOracleEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                                  isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                                  learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


def kappaFun(x, t=0):
    return 0.1 + 0.05 * x ** 2 + 0.02 * t


def velFun(x, t=0):
    return 0.5 + 0.3 * x + 0.1 * t


def test_assembly_contracts_the_gradients_with_the_uploaded_gcoef(cpu_engine):
    """Per mini-batch block the registered streams are A, B at the rows and a = dA . gcoef, b = dB . gcoef with the gcoef of the
    same registration (kappa dN/dx + v N: hat-function rows), dA and dB taken here from torch autograd of A and B; the BC/IC rows
    get A and B alone; under nldiff the contraction is with kappa dN/dx alone."""
    for kw in ({}, {'nldiff': [0.7, 0.4, 0.3]}):
        pde = ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=kappaFun, vel=velFun, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x), ansatz=AZ,
                    **kw)
        vn = VarNet(pde, layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
        eng, fd = vn.engine, vn.fixData
        td = vn._build_tdata(batchNum=3)
        seen = 0
        for bi in range(td.batchNum):
            X, g, n_k = eng.batches[bi][0], eng.batches[bi][1], eng.batches[bi][3]
            if kw:
                np.testing.assert_allclose(g, kappaFun(X[:, 0:1], X[:, 1:2]) * np.tile(fd.dNx[:, 0:1], (n_k, 1)), rtol=1e-13, atol=1e-15)
            A, B, a, b = eng.az[bi]
            Xt = torch.as_tensor(X, dtype=torch.float64).clone().requires_grad_(True)
            At, Bt = torch.sin(pi * Xt[:, 0]), Xt[:, 1] * (1.0 - Xt[:, 0] ** 2)
            np.testing.assert_allclose(A, At.detach().numpy(), rtol=1e-13, atol=1e-15)
            np.testing.assert_allclose(B, Bt.detach().numpy(), rtol=1e-13, atol=1e-15)
            for got, f in ((a, At), (b, Bt)):
                want = torch.autograd.grad(f.sum(), Xt, retain_graph=True)[0][:, 0].numpy() * g[:, 0]
                np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.max(np.abs(want)))
            seen += len(A)
        assert seen == fd.nt * fd.integNum
        td.select_mor(0)
        bx = eng.bic[0]
        A, B, a, b = eng.azr['bic']
        assert a is None and b is None
        np.testing.assert_allclose(A, Afun(bx[:, 0]), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(B, Bfun(bx[:, 0], bx[:, 1]), rtol=1e-13, atol=1e-15)
        assert np.max(np.abs(B[fd.bDofsum:])) == 0.0                   # t = 0 on the initial rows: the data hold exactly
    vn = VarNet(_pde(None), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)      # no ansatz: nothing registered
    td = vn._build_tdata()
    assert not getattr(vn.engine, 'az', {}) and td.mor[0]['az'] is None and td.mor[0]['az_bic'] is None


def test_evaluate_and_residual_see_the_constrained_solution(cpu_engine):
    vn = VarNet(_pde(AZ_FULL, source=lambda x, t=0: 0.3 * x + t, cEx=lambda x, t=0: np.exp(-t) * np.sin(pi * x)), layerWidth=[5], discNum=8,
                bDiscNum=None, tDiscNum=6)
    vn.engine.set_params(og.glorot_init(2, [5], 4))
    x = np.linspace(-1, 1, 9).reshape(-1, 1)
    N0 = vn.engine.forward(np.hstack([x, np.zeros_like(x)])).numpy().reshape(-1, 1)
    assert np.max(np.abs(N0)) > 1e-2
    np.testing.assert_array_equal(vn.evaluate(x, 0.0), np.sin(pi * x))                         # the initial state, exactly
    edge = vn.evaluate(np.array([[-1.0], [1.0]]), 0.7)
    assert np.max(np.abs(edge)) <= 1e-15                                                       # the walls
    # the composed strong residual against autograd of the composite
    res, resVec, err, cApp = vn.residual()
    X = torch.as_tensor(vn.fixData.uniform_input, dtype=torch.float64).clone().requires_grad_(True)
    params = og.unflatten(vn.engine.theta.astype(np.float64), 2, [5], dtype=torch.float64)
    u = torch.sin(pi * X[:, 0]) + X[:, 1] * (1.0 - X[:, 0] ** 2) * og.model(params, X)[:, 0]
    gu = torch.autograd.grad(u.sum(), X, create_graph=True)[0]
    uxx = torch.autograd.grad(gu[:, 0].sum(), X)[0][:, 0]
    want = (-gu[:, 1] + 0.1 * uxx + 0.3 * X[:, 0] + X[:, 1]).detach().numpy().reshape(-1, 1)
    np.testing.assert_allclose(resVec, want, rtol=1e-10, atol=1e-10 * np.max(np.abs(want)))
    np.testing.assert_allclose(cApp, u.detach().numpy().reshape(-1, 1), rtol=1e-13, atol=1e-15)
    assert err is not None and np.isfinite(res)


def test_varnet_refusals(cpu_engine):
    """Every refusal that needs no device, one sentence each."""
    kw = dict(layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
    with pytest.raises(NotImplementedError, match='towers'):
        VarNet(_pde(), processors=[0, 1], **kw)
    with pytest.raises(NotImplementedError, match='lbfgsLoss64'):
        VarNet(_pde(), optimizer='lbfgs', lbfgsLoss64=True, **kw)
    obs = dict(X=np.array([[0.1, 0.2], [0.3, 0.4]]), value=np.array([0.5, 0.6]))
    with pytest.raises(NotImplementedError, match='an ansatz with learnCoef'):
        VarNet(_pde(reaction=(1.0, [1.0])), observations=obs, learnCoef={'reaction': [0]}, **kw)
    vn = VarNet(_pde(), **kw)
    with pytest.raises(NotImplementedError, match="ansatz\\['A_t'\\], 'B_t', 'lapA', 'lapB'|A_t.*B_t.*lapA.*lapB"):
        vn.residual()
    with pytest.raises(NotImplementedError, match='fp64'):
        VarNet(_pde(AZ_FULL), **kw).residual(fp64=True)
    with pytest.raises(NotImplementedError, match='polynomial term'):
        VarNet(_pde(AZ_FULL, reaction=(1.0, [1.0])), **kw).residual()
    td = vn._build_tdata()
    with pytest.raises(NotImplementedError, match='splitLoss'):
        vn.splitLoss(td, fp64=True)
    with pytest.raises(NotImplementedError, match='precisionReport'):
        vn.precisionReport(td)
    with pytest.raises(NotImplementedError, match='shuffleData'):
        vn.train('/nonexistent', epochNum=1, batchNum=2, shuffleData=True)


def test_checkpoint_carries_a_flag_only_with_an_ansatz(cpu_engine):
    kw = dict(layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
    with_az, without = VarNet(_pde(), **kw), VarNet(_pde(None), **kw)
    a, b = with_az.checkpoint_arrays(), without.checkpoint_arrays()
    assert 'ansatz' in a and 'ansatz' not in b and set(a) - set(b) == {'ansatz'}
    with_az.restore_arrays(a)
    without.restore_arrays(b)
    with pytest.raises(ValueError, match='was trained with an ansatz'):
        without.restore_arrays(a)
    with pytest.raises(ValueError, match='was trained without an ansatz'):
        with_az.restore_arrays(b)
