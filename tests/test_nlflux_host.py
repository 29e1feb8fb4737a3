"""
CPU tier of the polynomial flux term (`ADPDE(nlflux=(w, [f1, f2, f3]))`, vn_set_nlflux): the fp64 restatement of
tests/nlflux_ref.py against tests/reaction_ref.py and the oracle (zero coefficients: bit for bit) and against central differences,
`ADPDE` validation and the MOR refusal, the declaration and binding of the new entry point, the host assembly of the phi stream
through a stand-in engine (periodic tables and per-row tables; mini-batches and shuffles pick the same rows as the other interior
arrays), and flux-free case files.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests import nlflux_ref, reaction_ref
from tests.nlflux_cases import CASES, COEF, FLUX, IDS, inputs, phi, ref_kw, reference, reference64, theta
from tests.oracle_engine import OracleEngine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pi = np.pi


# ---- the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_zero_coefficients_are_the_oracle_and_the_reaction_reference_exactly(i):
    d_in, widths = CASES[i][0], CASES[i][2]
    flat = theta(i).astype(np.float64)
    ph = phi(i).astype(np.float64)
    rate = inputs(i)[1].astype(np.float64)
    for reaction, want in ((None, og.loss_and_grad(flat, d_in, widths, torch.float64, **ref_kw(i))),
                           ((rate, COEF), reaction_ref.loss_and_grad(flat, d_in, widths, (rate, COEF), torch.float64, **ref_kw(i)))):
        ref, g = want
        got, gg = nlflux_ref.loss_and_grad(flat, d_in, widths, (ph, (0.0, 0.0, 0.0)), reaction, torch.float64, **ref_kw(i))
        for k in ('loss', 'BCloss', 'ICloss', 'varLoss'):
            assert got[k] == ref[k], (k, got[k], ref[k])
        assert np.array_equal(got['lossVec'], ref['lossVec'])
        assert np.array_equal(gg, g)


@pytest.mark.parametrize('variant', ['flux', 'both'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_reference_gradient_against_central_differences(i, variant):
    """6 sampled coordinates agree with central differences to 1e-7 of the gradient's largest entry, and each to 1e-4 of itself
    (the bar of tests/test_reaction_host.py; coordinates with |g| < 1e-8 are not judged there).  The scale of the first bar: a
    central difference with step h carries the rounding error eps |f| / h of the two losses, an ABSOLUTE error that does not
    shrink with the coordinate, so it is judged against the gradient's scale and not against a small coordinate's own value.
    The term is a real part of the objective on these inputs."""
    ref, g = reference64(i, variant)
    ref0, g0 = reference64(i, 'none')
    assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss'])
    assert np.linalg.norm(g - g0) > 1e-2 * np.linalg.norm(g)
    flat = theta(i).astype(np.float64)
    h = 1e-5
    judged = 0
    for p in np.random.default_rng(7).choice(flat.size, 6, replace=False):
        if abs(g[p]) < 1e-8:
            continue
        e = np.zeros_like(flat)
        e[p] = h
        fp = reference(i, variant, flat + e)[0]['loss']
        fm = reference(i, variant, flat - e)[0]['loss']
        fd = (fp - fm) / (2 * h)
        err = abs(fd - g[p]) / abs(g[p])
        print('case %s %s coordinate %d: autograd %.6e, central difference %.6e, relative %.2e' % (IDS[i], variant, p, g[p], fd, err))
        assert abs(fd - g[p]) <= 1e-7 * np.max(np.abs(g)), (IDS[i], p, g[p], fd, np.max(np.abs(g)))
        assert err <= 1e-4, (IDS[i], p, g[p], fd)
        judged += 1
    assert judged >= 3


def test_reference_residual_adds_the_term():
    rng = np.random.default_rng(0)
    n, d_in, dim, widths = 50, 3, 2, [10, 20]
    X = rng.uniform(-1, 1, (n, d_in))
    diff, vel = rng.uniform(0.1, 1, (n, 1)), rng.standard_normal((n, dim))
    src, ddx = rng.standard_normal((n, 1)), rng.standard_normal((n, dim))
    w, divw = rng.standard_normal((n, dim)), rng.standard_normal((n, 1))
    flat = og.glorot_init(d_in, widths, 3).astype(np.float64)
    u, r0 = og.residual(flat, d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, True)
    u1, r1 = nlflux_ref.residual(flat, d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, (w, FLUX, divw))
    assert np.array_equal(u, u1)
    # w . grad u from the oracle's own residual, which is affine in vel with slope -grad u
    _, rw = og.residual(flat, d_in, widths, torch.float64, X, diff, vel + w, src, ddx, dim, True)
    dF = 0.6 + 2 * 0.5 * u + 3 * -0.3 * u ** 2
    F = 0.6 * u + 0.5 * u ** 2 - 0.3 * u ** 3
    np.testing.assert_allclose(r1 - r0, -(dF * (r0 - rw) + F * divw), rtol=1e-10, atol=1e-13)
    # a linear flux with constant w is an extra velocity
    _, r2 = nlflux_ref.residual(flat, d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, ([0.3, -0.2], (2.0,), None))
    _, r3 = og.residual(flat, d_in, widths, torch.float64, X, diff, vel + 2.0 * np.array([[0.3, -0.2]]), src, ddx, dim, True)
    np.testing.assert_allclose(r2, r3, rtol=1e-12, atol=1e-14)


# ---- ADPDE ------------------------------------------------------------------------------------------------------
def _pde(**kw):
    return ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, vel=0.0, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x), **kw)


def test_adpde_nlflux_argument():
    assert _pde().nlflux is None
    p = _pde(nlflux=(1.0, [0, 0.5]))
    assert p.nlfluxCoef == [0.0, 0.5, 0.0] and p.nlfluxDivFun is None and list(p.nlfluxW) == [1.0]
    np.testing.assert_array_equal(p.nlfluxWFun(np.zeros((3, 1)), np.zeros((3, 1))), np.ones((3, 1)))
    f = lambda x, t=0: 1.0 + x ** 2
    dv = lambda x, t=0: 2.0 * x
    p = _pde(nlflux=(f, (1.0, -1.0, 0.5), dv))
    assert p.nlfluxWFun is f and p.nlfluxW is None and p.nlfluxCoef == [1.0, -1.0, 0.5] and p.nlfluxDivFun is dv
    assert _pde(nlflux=([2.0], [1.0])).nlfluxCoef == [1.0, 0.0, 0.0]
    for bad in (1.0, (1.0,), (1.0, [1, 2, 3, 4]), (1.0, []), ('fast', [1.0]), (1.0, [np.nan]), (1.0, 'abc'), (np.inf, [1.0]),
                ([1.0, 2.0], [1.0]), (1.0, [1.0], 3.0), (1.0, [1.0], None, None)):
        with pytest.raises(ValueError, match='nlflux'):
            _pde(nlflux=bad)
    assert 'div(w F(c))' in ADPDE.__doc__ and 'constant or divergence-free' in ADPDE.__doc__


def test_mor_with_nlflux_raises():
    def diffFun(x, t=0, D=0.01):
        return D * np.ones([len(x), 1])

    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    with pytest.raises(NotImplementedError, match='a parametric field w is out of scope'):
        ADPDE(Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x),
              MORvar=mor, nlflux=(1.0, [0, 0.5]))


# ---- ABI --------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_bound():
    from varnet_amd import engine as vengine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    assert re.search(r'int\s+vn_set_nlflux\s*\(\s*vn_engine\s*\*\s*h,\s*int32_t\s+batch,\s*const\s+float\s*\*\s*phi_dev,'
                     r'\s*const\s+double\s+coef\[3\]\s*\)\s*;', hdr)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr) and vengine.VN_ABI_VERSION == 7
    assert 'vn_set_nlflux' in vengine.ABI_SYMBOLS
    assert callable(getattr(vengine.VNEngine, 'set_nlflux'))
    if os.path.exists(vengine.LIB_PATH):                       # (needs the built library)
        assert hasattr(vengine.load_library(), 'vn_set_nlflux')


# ---- VarNet host layer through a stand-in engine ----------------------------------------------------------------------
class NlfluxOracleEngine(OracleEngine):
    """The oracle engine with vn_set_reaction and vn_set_nlflux: batches with a registration are evaluated by tests/nlflux_ref.py."""

    def set_interior(self, batch, *a, **kw):
        super().set_interior(batch, *a, **kw)
        self.__dict__.setdefault('react', {}).pop(batch, None)          # vn_set_interior clears both registrations
        self.__dict__.setdefault('flux', {}).pop(batch, None)

    def _register(self, table, batch, rows, coef):
        c = [] if coef is None else [float(x) for x in coef]
        if not any(c):
            table.pop(batch, None)
            return
        n = self.batches[batch][0].shape[0]
        r = None if rows is None else np.array(rows.numpy() if isinstance(rows, torch.Tensor) else rows, dtype=float).reshape(-1, 1)
        assert r is None or r.shape[0] == n
        table[batch] = (r, c + [0.0] * (3 - len(c)))

    def set_reaction(self, batch, rate=None, coef=None):
        self._register(self.__dict__.setdefault('react', {}), batch, rate, coef)

    def set_nlflux(self, batch, phi=None, coef=None):
        self._register(self.__dict__.setdefault('flux', {}), batch, phi, coef)

    def _eval(self, batch):
        fx = getattr(self, 'flux', {}).get(batch)
        rc = getattr(self, 'react', {}).get(batch)
        if fx is None and rc is None:
            return super()._eval(batch)
        Input, gcoef, src, n_k, detJ, Nr, dNtr = self.batches[batch]
        biInput, biLabel, bDof, biDimVal = self.bic
        N, dNt, W = self.fe
        n = Input.shape[0]
        kw = dict(Input=Input, gcoef=gcoef, source=None if not self.isSource else src.reshape(n, 1),
                  N=(np.tile(N, n_k) if Nr is None else Nr).reshape(n, 1), dNt=(np.tile(dNt, n_k) if dNtr is None else dNtr).reshape(n, 1),
                  integW=None if not self.integWflag else W.reshape(1, -1), intShape=[n_k, self.integNum], detJ=detJ,
                  detJvec=np.size(detJ) > 1, biInput=biInput, biLabel=biLabel.reshape(-1, 1), bDof=bDof, biDimVal=biDimVal,
                  w=self.w, dim=self.dim, time_dependent=self.td, is_source=self.isSource, integWflag=self.integWflag)
        return nlflux_ref.loss_and_grad(self.theta.astype(np.float64), self.inpDim, self.layerWidth, fx, rc, torch.float64, **kw)

    def residual(self, X, diff, vel, source=None, diff_dx=None, fp64=False, reaction=None, nlflux=None):
        n = np.shape(X)[0]
        src = np.zeros((n, 1)) if source is None else np.reshape(source, (n, 1))
        ddx = np.zeros((n, self.dim)) if diff_dx is None else np.reshape(diff_dx, (n, self.dim))
        if reaction is not None:
            reaction = (np.reshape(reaction[0], (-1, 1)), reaction[1])
        u, r = nlflux_ref.residual(self.theta, self.inpDim, self.layerWidth, torch.float64, np.asarray(X), np.reshape(diff, (n, 1)),
                                   np.reshape(vel, (n, self.dim)), src, ddx, self.dim, nlflux, reaction, self.td)
        return torch.as_tensor(u[:, 0]), torch.as_tensor(r[:, 0])


@pytest.fixture
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return NlfluxOracleEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                                  isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                                  learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


def wFun(x, t=0):
    return 1.0 + 0.5 * x + t


def divwFun(x, t=0):
    return 0.5 * np.ones([len(x), 1])


def test_phi_stream_follows_the_rows_of_every_batch(cpu_engine):
    """Periodic tables: phi of a row is w(x_r, t_r) dN_p/dx with p the row's quadrature point, whatever the mini-batch or shuffle."""
    vn = VarNet(_pde(nlflux=(wFun, [0.6, 0.5, -0.3]), reaction=(2.0, [-1.0])), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
    eng, fd = vn.engine, vn.fixData
    td = vn._build_tdata(batchNum=3)
    for shuffled in (False, True):
        if shuffled:
            np.random.seed(3)
            td.shuffleTrainData()
        seen = 0
        for bi in range(td.batchNum):
            ph, coef = eng.flux[bi]
            X = eng.batches[bi][0]
            n_k = eng.batches[bi][3]
            assert coef == [0.6, 0.5, -0.3]
            want = wFun(X[:, 0:1], X[:, 1:2]).astype(np.float64) * np.tile(fd.dNx[:, 0:1], (n_k, 1))
            np.testing.assert_allclose(ph, want, rtol=1e-13, atol=1e-13 * np.max(np.abs(want)))
            assert eng.react[bi][1] == [-2.0, 0.0, 0.0]                   # the reaction of the same batch is kept
            seen += len(ph)
        assert seen == fd.nt * fd.integNum
    # a constant w: the same stream with w = 1
    vn = VarNet(_pde(nlflux=(1.0, [0, 0.5])), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
    vn._build_tdata()
    ph, coef = vn.engine.flux[0]
    assert coef == [0.0, 0.5, 0.0]
    np.testing.assert_allclose(ph, np.tile(vn.fixData.dNx[:, 0:1], (vn.fixData.nt, 1)), rtol=1e-13)


def test_phi_stream_on_per_row_tables(cpu_engine):
    """Scaled supports (detJvec): phi = (w * dNx_rows).sum(1) with the per-row tables of fixData.rows()."""
    vn = VarNet(_pde(nlflux=(wFun, [0.6, 0.5, -0.3])), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
    fd = vn.fixData
    fd.updateOptimData(0.5, 0.5)
    assert fd.detJvec
    rng = np.random.default_rng(2)
    Input = np.hstack([rng.uniform(-1, 1, (fd.nT, 1)), rng.uniform(0, 0.5, (fd.nT, 1))])
    biInput = np.hstack([rng.uniform(-1, 1, (sum(fd.biDof), 1)), rng.uniform(0, 0.5, (sum(fd.biDof), 1))])
    d = vn._assemble(Input, biInput, fd.biDof, 0, None)
    _, dNxr, _ = fd.rows()
    assert len(np.unique(np.round(dNxr, 12))) > len(np.unique(np.round(fd.dNx, 12)))      # two families of supports
    want = (wFun(Input[:, 0:1], Input[:, 1:2]) * dNxr).sum(1)
    np.testing.assert_allclose(d['phi'].numpy().astype(np.float64), want, rtol=1e-13, atol=1e-13 * np.max(np.abs(want)))
    assert d['nlfluxCoef'] == [0.6, 0.5, -0.3] and d['N_rows'] is not None


def test_loss_and_residual_see_the_term(cpu_engine):
    out = {}
    for key, kw in (('off', {}), ('on', {'nlflux': (wFun, [0.6, 0.5, -0.3], divwFun)}), ('nodiv', {'nlflux': (wFun, [0.6, 0.5, -0.3])})):
        vn = VarNet(_pde(**kw), layerWidth=[6, 4], discNum=8, bDiscNum=None, tDiscNum=6)
        vn.engine.set_params(vn.engine.get_params() + 0.1)
        comp, _, _ = vn.splitLoss(vn._build_tdata())
        out[key] = (comp, vn.residual()[1], vn.residual()[3], vn.fixData.uniform_input)
    (c0, r0, u0, X), (c1, r1, u1, _), (c2, r2, _, _) = out['off'], out['on'], out['nodiv']
    np.testing.assert_array_equal(c0[:2], c1[:2])
    assert abs(c1[2, 0] - c0[2, 0]) > 1e-2 * abs(c0[2, 0])
    np.testing.assert_array_equal(c1, c2)                                   # div_w enters the strong residual only
    np.testing.assert_array_equal(u0, u1)
    F = 0.6 * u0 + 0.5 * u0 ** 2 - 0.3 * u0 ** 3
    np.testing.assert_allclose(r2 - r1, 0.5 * F, rtol=1e-9, atol=1e-12)     # ... as -F(u) div w
    assert np.max(np.abs(r2 - r0)) > 1e-2 * np.max(np.abs(r0))


def _case_lines(path):
    return [ln for ln in open(path).read().splitlines(True) if not ln.startswith('Simulation date')]


def test_case_file_names_the_term_only_when_present(cpu_engine, tmp_path):
    lines = {}
    for key, kw in (('default', {}), ('none', {'nlflux': None}), ('on', {'nlflux': (1.0, [0, 0.5])})):
        np.random.seed(0)
        vn = VarNet(_pde(**kw), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
        vn.train(str(tmp_path / key), epochNum=1, saveFreq=1, verbose=False)
        lines[key] = _case_lines(str(tmp_path / key / 'caseData.txt'))
    assert lines['default'] == lines['none'] and not any('Flux term' in ln for ln in lines['default'])
    extra = [ln for ln in lines['on'] if 'Flux term' in ln]
    assert extra == ['Flux term: -div(w*(f1 c + f2 c^2 + f3 c^3)), coefficients [0.0, 0.5, 0.0]\n']
