"""
CPU tier of the solution-dependent diffusivity (`ADPDE(nldiff=[d0, d1, d2])`, vn_set_nldiff): the condition on the test inputs
(each of D and psi alone moves every compared quantity by at least 100 x the bar it is compared at), the fp64 restatement of
tests/nldiff_ref.py against tests/nlflux_ref.py (D = 1 without psi: bit for bit), against central differences and against a direct
autograd divergence, the hand-derived seeds of DESIGN.md section 16 against autograd, `ADPDE` validation and the MOR refusal, the
declaration and binding of the new entry point, and the host assembly (gcoef = kappa dN/dx, the psi stream) through a stand-in
engine.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests import nldiff_ref, nlflux_ref
from tests.gradcheck import block_errors
from tests.nldiff_cases import (CASES, COEF, DEGENERATE, DIFF, FLUX, IDS, inputs, phi, psi, ref_kw, reference, reference64, terms_of,
                                theta)
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL
from tests.test_nlflux_host import NlfluxOracleEngine
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pi = np.pi


def moved(i, with_term, without):
    """How far leaving a term out moves what the parity tests compare, each on the scale its bar uses: (loss, varLoss, lossVec,
    least-moved parameter tensor of the gradient)."""
    (ra, ga), (rb, gb) = reference64(i, with_term), reference64(i, without)
    lv = np.max(np.abs(ra['lossVec'] - rb['lossVec'])) / np.max(np.abs(ra['lossVec']))
    blocks = block_errors(gb, ga, CASES[i][0], CASES[i][2], CASES[i][1], CASES[i][7])
    return (abs(ra['loss'] - rb['loss']) / abs(ra['loss']), abs(ra['varLoss'] - rb['varLoss']) / abs(ra['varLoss']), float(lv),
            min(blocks.values()))


# ---- the inputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_inputs_make_a_missing_term_fail(i):
    """A condition on the INPUTS, from the fp64 reference alone (no engine, no tolerance of one): D alone ('d' against no term) and
    psi alone ('psi' against no term) each move the loss and varLoss by >= 100 LOSS_RTOL, lossVec by >= 100 LVEC_RTOL of its
    maximum and EVERY parameter tensor of the gradient by >= 100 GRAD_RTOL of its own size.  (BCloss and ICloss do not contain
    the interior rows: no interior term can move them.)  Every gradient is finite, the degenerate D = u^2 included."""
    for alone in ('d', 'psi'):
        dl, dv, lv, blk = moved(i, alone, 'none')
        print('nldiff inputs %s, %s alone: loss %.3g varLoss %.3g lossVec %.3g least-moved gradient tensor %.3g'
              % (IDS[i], alone, dl, dv, lv, blk))
        assert dl >= 100 * LOSS_RTOL and dv >= 100 * LOSS_RTOL, (alone, dl, dv)
        assert lv >= 100 * LVEC_RTOL, (alone, lv)
        assert blk >= 100 * GRAD_RTOL, (alone, blk)
    for variant in ('dpsi', 'd', 'psi', 'all', 'pm'):
        assert np.all(np.isfinite(reference64(i, variant)[1])), variant


# ---- the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_unit_diffusivity_without_psi_is_the_flux_reference_exactly(i):
    d_in, widths = CASES[i][0], CASES[i][2]
    flat = theta(i).astype(np.float64)
    ph = phi(i).astype(np.float64)
    rate = inputs(i)[1].astype(np.float64)
    for nlflux, reaction in ((None, None), ((ph, FLUX), None), ((ph, FLUX), (rate, COEF))):
        ref, g = nlflux_ref.loss_and_grad(flat, d_in, widths, nlflux, reaction, torch.float64, **ref_kw(i))
        got, gg = nldiff_ref.loss_and_grad(flat, d_in, widths, (None, (1.0, 0.0, 0.0)), nlflux, reaction, torch.float64, **ref_kw(i))
        for k in ('loss', 'BCloss', 'ICloss', 'varLoss'):
            assert got[k] == ref[k], (k, got[k], ref[k])
        assert np.array_equal(got['lossVec'], ref['lossVec'])
        assert np.array_equal(gg, g)


@pytest.mark.parametrize('variant', ['dpsi', 'all', 'pm'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_reference_gradient_against_central_differences(i, variant):
    """6 sampled coordinates agree with central differences of the reference's own loss to 1e-7 of the gradient's largest entry,
    and each to 1e-4 of itself (the bars of tests/test_nlflux_host.py; coordinates with |g| < 1e-8 are not judged there)."""
    ref, g = reference64(i, variant)
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


def test_hand_derived_seeds_against_autograd():
    """The seeds the kernels implement: with A_r = sum_d u_{x_d} gcoef_d, the row integrand
    t_r = D(u) A - u psi - u dNt - (s + rho p(u)) N - F(u) phi and s_r = d loss / d t_r = 2 w2 detJ R_k W_p,
        d loss / d u_r = (D'(u) A - psi - dNt - rho p'(u) N - F'(u) phi) s_r,        d loss / d A_r = D(u) s_r,
    against torch autograd with u and A as independent leaves.  D = (0, 0, 1) with u = 0 at some rows: nothing divides by D."""
    rng = np.random.default_rng(21)
    n_k, q, w2, detJ = 7, 5, 5.0, 0.137
    n = n_k * q
    T = lambda a: torch.as_tensor(a, dtype=torch.float64)
    for dcoef in (DIFF, DEGENERATE):
        u0 = rng.standard_normal(n)
        u0[::6] = 0.0
        u, A = T(u0).requires_grad_(True), T(rng.standard_normal(n)).requires_grad_(True)
        ps, dNt, N, ph = (T(rng.standard_normal(n)) for _ in range(4))
        s, rho, W = T(rng.standard_normal(n)), T(rng.uniform(0.5, 2, n)), T(np.tile(rng.uniform(0.5, 1, q), n_k))
        c, f = COEF, FLUX
        D = dcoef[0] + u * (dcoef[1] + u * dcoef[2])
        t = D * A - u * ps - u * dNt - (s + rho * (c[0] * u + c[1] * u ** 2 + c[2] * u ** 3)) * N - (f[0] * u + f[1] * u ** 2 + f[2] * u ** 3) * ph
        R = (W * t).reshape(n_k, q).sum(1)
        loss = w2 * detJ * (R ** 2).sum()
        loss.backward()
        with torch.no_grad():
            seed = (2.0 * w2 * detJ * R).repeat_interleave(q) * W
            dD = dcoef[1] + 2.0 * dcoef[2] * u
            ubar = (dD * A - ps - dNt - rho * (c[0] + 2 * c[1] * u + 3 * c[2] * u ** 2) * N - (f[0] + 2 * f[1] * u + 3 * f[2] * u ** 2) * ph) * seed
            udbar = D * seed
        np.testing.assert_allclose(ubar.numpy(), u.grad.numpy(), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(udbar.numpy(), A.grad.numpy(), rtol=1e-12, atol=1e-13)
        assert np.all(np.isfinite(ubar.numpy())) and (dcoef != DEGENERATE or np.any(udbar.numpy() == 0.0))


def test_advection_on_the_value_side_is_the_same_weak_form():
    """int v . grad u N = -int u (v . grad N + N div v) for a test function that vanishes on the edge of its support: on a 1D hat
    function with a fine quadrature both sides agree, with a constant and with a variable velocity."""
    x = np.linspace(-1.0, 1.0, 200001)
    N, dN = 1.0 - np.abs(x), -np.sign(x)
    u, du = np.sin(2.0 * x + 0.3), 2.0 * np.cos(2.0 * x + 0.3)
    for v, dv in ((0.5 + 0 * x, 0 * x), (1.0 + 0.5 * x ** 2, x)):
        trap = lambda f: float(np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(x)))
        lhs = trap(v * du * N)
        rhs = -trap(u * (v * dN + N * dv))
        assert abs(lhs - rhs) < 1e-8 * max(1.0, abs(lhs)), (lhs, rhs)


def test_reference_residual_is_the_divergence_form():
    """nldiff_ref.residual against a direct autograd evaluation of -u_t + div(kappa(x) D(u) grad u) - v . grad u + s with kappa a
    smooth function of x (its gradient passed as diff_dx), in 2D+t."""
    rng = np.random.default_rng(0)
    n, d_in, dim, widths = 40, 3, 2, [10, 20]
    X = rng.uniform(-1, 1, (n, d_in))
    vel, src = rng.standard_normal((n, dim)), rng.standard_normal((n, 1))
    flat = 2.0 * og.glorot_init(d_in, widths, 3).astype(np.float64)
    kap = lambda x: 0.5 + 0.2 * x[:, 0:1] ** 2 + 0.1 * torch.sin(x[:, 1:2])
    Xt = torch.as_tensor(X).clone().requires_grad_(True)
    params = og.unflatten(flat, d_in, widths, dtype=torch.float64)
    u = og.model(params, Xt, 'sigmoid')
    gu = torch.autograd.grad(u.sum(), Xt, create_graph=True)[0]
    fluxv = kap(Xt) * nldiff_ref.dfun(u, DIFF) * gu[:, :dim]
    div = sum(torch.autograd.grad(fluxv[:, d].sum(), Xt, create_graph=True)[0][:, d:d + 1] for d in range(dim))
    want = (-gu[:, dim:dim + 1] + div - (torch.as_tensor(vel) * gu[:, :dim]).sum(1, keepdim=True) + torch.as_tensor(src)).detach().numpy()
    Xk = torch.as_tensor(X).clone().requires_grad_(True)
    kv = kap(Xk)
    dk = torch.autograd.grad(kv.sum(), Xk)[0][:, :dim].numpy()
    val, got = nldiff_ref.residual(flat, d_in, widths, torch.float64, X, kv.detach().numpy(), vel, src, dk, dim, DIFF)
    np.testing.assert_allclose(val, u.detach().numpy(), rtol=0, atol=1e-15)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-13)
    _, lin = nldiff_ref.residual(flat, d_in, widths, torch.float64, X, kv.detach().numpy(), vel, src, dk, dim, None)
    assert np.max(np.abs(got - lin)) > 1e-2 * np.max(np.abs(got))
    _, one = nldiff_ref.residual(flat, d_in, widths, torch.float64, X, kv.detach().numpy(), vel, src, dk, dim, (1.0, 0.0, 0.0))
    np.testing.assert_allclose(one, lin, rtol=1e-14, atol=1e-15)


# ---- ADPDE ----------------------------------------------------------------------------------------------------------
def _pde(**kw):
    kw.setdefault('vel', 0.0)
    return ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x), **kw)


def test_adpde_nldiff_argument():
    assert _pde().nldiff is None
    p = _pde(nldiff=[0, 2])
    assert p.nldiffCoef == [0.0, 2.0, 0.0] and p.nldiffDivFun is None and p.nldiff == [0.0, 2.0, 0.0]
    dv = lambda x, t=0: 2.0 * x
    p = _pde(nldiff=([1.0, 0.0, 2.0], dv))
    assert p.nldiffCoef == [1.0, 0.0, 2.0] and p.nldiffDivFun is dv
    assert _pde(nldiff=(0.5,)).nldiffCoef == [0.5, 0.0, 0.0]
    assert _pde(nldiff=np.array([1.0, 0.5])).nldiffCoef == [1.0, 0.5, 0.0]
    assert _pde(nldiff=[1.0, 0.5], reaction=(2.0, [-1.0]), nlflux=(1.0, [0, 0.5])).nlfluxCoef == [0.0, 0.5, 0.0]
    for bad in (1.0, 'abc', [], [1, 2, 3, 4], [np.nan], [1.0, np.inf], ['a', 'b'], ([1.0, 0.0], 3.0), ([1.0], 'fast'), ([], dv)):
        with pytest.raises(ValueError, match='nldiff'):
            _pde(nldiff=bad)
    assert 'div(diff D(c) grad c)' in ADPDE.__doc__ and 'constant\n    or divergence-free' in ADPDE.__doc__


def test_mor_with_nldiff_raises():
    def diffFun(x, t=0, D=0.01):
        return D * np.ones([len(x), 1])

    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    with pytest.raises(NotImplementedError, match='solution-dependent diffusivity with model-order reduction'):
        ADPDE(Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x),
              MORvar=mor, nldiff=[1.0, 0.0, 2.0])


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_bound():
    from varnet_amd import engine as vengine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    assert re.search(r'int\s+vn_set_nldiff\s*\(\s*vn_engine\s*\*\s*h,\s*int32_t\s+batch,\s*const\s+float\s*\*\s*psi_dev,'
                     r'\s*const\s+double\s+coef\[3\]\s*\)\s*;', hdr)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr) and vengine.VN_ABI_VERSION == 7
    assert 'vn_set_nldiff' in vengine.ABI_SYMBOLS
    assert callable(getattr(vengine.VNEngine, 'set_nldiff'))
    assert 'kappa dN/dx' in hdr[hdr.index('quasilinear diffusion'):hdr.index('int vn_set_nldiff')]     # the caller's side of the contract
    if os.path.exists(vengine.LIB_PATH):                       # (needs the built library)
        assert hasattr(vengine.load_library(), 'vn_set_nldiff')


class _Lib:
    """Records vn_set_nldiff calls in place of the library (argument handling that needs no device)."""

    def __init__(self):
        self.calls = []

    def vn_set_nldiff(self, h, batch, psi, coef):
        self.calls.append((batch, psi, None if coef is None else list(coef)))
        return 0


def test_set_nldiff_argument_handling():
    from varnet_amd.engine import VNEngine
    eng = VNEngine.__new__(VNEngine)
    eng.lib, eng.h, eng._keep, eng.torch = _Lib(), None, {('nldiff', 0): 'old'}, torch
    eng._ck = lambda rc: None
    with pytest.raises(ValueError, match='at most three coefficients'):
        eng.set_nldiff(0, None, (1.0, 2.0, 3.0, 4.0))
    assert eng.lib.calls == [] and eng._keep[('nldiff', 0)] == 'old'
    eng.set_nldiff(0)                                            # coef None clears ...
    eng.set_nldiff(0, None, (1.0,))                              # ... and so does D = 1 without psi (zero-padded)
    assert eng.lib.calls == [(0, None, None), (0, None, None)] and ('nldiff', 0) not in eng._keep
    eng.set_nldiff(3, None, [0.0, 2.0])                          # psi None with another D: a registration without advection
    assert eng.lib.calls[-1] == (3, None, [0.0, 2.0, 0.0]) and eng._keep[('nldiff', 3)] is None


# ---- VarNet host layer through a stand-in engine --------------------------------------------------------------------
class NldiffOracleEngine(NlfluxOracleEngine):
    """The stand-in engine of tests/test_nlflux_host.py with vn_set_nldiff: such batches are evaluated by tests/nldiff_ref.py."""

    def set_interior(self, batch, *a, **kw):
        super().set_interior(batch, *a, **kw)
        self.__dict__.setdefault('ndiff', {}).pop(batch, None)

    def set_nldiff(self, batch, psi=None, coef=None):
        table = self.__dict__.setdefault('ndiff', {})
        c = [] if coef is None else [float(x) for x in coef]
        c = c + [0.0] * (3 - len(c))
        if coef is None or (c == [1.0, 0.0, 0.0] and psi is None):
            table.pop(batch, None)
            return
        n = self.batches[batch][0].shape[0]
        r = None if psi is None else np.array(psi.numpy() if isinstance(psi, torch.Tensor) else psi, dtype=float).reshape(-1, 1)
        assert r is None or r.shape[0] == n
        table[batch] = (r, c)

    def _eval(self, batch):
        nd = getattr(self, 'ndiff', {}).get(batch)
        if nd is None:
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
        return nldiff_ref.loss_and_grad(self.theta.astype(np.float64), self.inpDim, self.layerWidth, nd,
                                        getattr(self, 'flux', {}).get(batch), getattr(self, 'react', {}).get(batch), torch.float64, **kw)

    def residual(self, X, diff, vel, source=None, diff_dx=None, fp64=False, reaction=None, nlflux=None, nldiff=None):
        n = np.shape(X)[0]
        src = np.zeros((n, 1)) if source is None else np.reshape(source, (n, 1))
        ddx = np.zeros((n, self.dim)) if diff_dx is None else np.reshape(diff_dx, (n, self.dim))
        if reaction is not None:
            reaction = (np.reshape(reaction[0], (-1, 1)), reaction[1])
        u, r = nldiff_ref.residual(self.theta, self.inpDim, self.layerWidth, torch.float64, np.asarray(X), np.reshape(diff, (n, 1)),
                                   np.reshape(vel, (n, self.dim)), src, ddx, self.dim, nldiff, nlflux, reaction, self.td)
        return torch.as_tensor(u[:, 0]), torch.as_tensor(r[:, 0])


@pytest.fixture
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return NldiffOracleEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                                  isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                                  learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


def kappaFun(x, t=0):
    return 0.1 + 0.05 * x ** 2 + 0.02 * t


def velFun(x, t=0):
    return 0.5 + 0.3 * x + 0.1 * t


def divvFun(x, t=0):
    return 0.3 * np.ones([len(x), 1])


def _pde2(**kw):
    return ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=kappaFun, vel=velFun, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x), **kw)


def test_assembly_moves_the_advection_to_psi(cpu_engine):
    """With the term gcoef = kappa dN/dx alone and psi = v dN/dx + N div v per row, whatever the mini-batch or shuffle; without it
    the assembled arrays are what they were (gcoef = kappa dN/dx + v N, no psi)."""
    vn = VarNet(_pde2(nldiff=([0.7, 0.4, 0.3], divvFun), reaction=(2.0, [-1.0])), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
    eng, fd = vn.engine, vn.fixData
    td = vn._build_tdata(batchNum=3)
    for shuffled in (False, True):
        if shuffled:
            np.random.seed(3)
            td.shuffleTrainData()
        seen = 0
        for bi in range(td.batchNum):
            ps, coef = eng.ndiff[bi]
            X, g, n_k = eng.batches[bi][0], eng.batches[bi][1], eng.batches[bi][3]
            assert coef == [0.7, 0.4, 0.3]
            x, t = X[:, 0:1], X[:, 1:2]
            dNx, N = np.tile(fd.dNx[:, 0:1], (n_k, 1)), np.tile(np.reshape(fd.N, (-1, 1)), (n_k, 1))
            np.testing.assert_allclose(g, kappaFun(x, t) * dNx, rtol=1e-13, atol=1e-15)
            want = velFun(x, t) * dNx + 0.3 * N
            np.testing.assert_allclose(ps, want, rtol=1e-13, atol=1e-13 * np.max(np.abs(want)))
            assert eng.react[bi][1] == [-2.0, 0.0, 0.0]                   # the reaction of the same batch is kept
            seen += len(ps)
        assert seen == fd.nt * fd.integNum
    # without div_vel the divergence is taken as zero; a zero velocity registers no psi at all
    vn = VarNet(_pde2(nldiff=[0.7, 0.4, 0.3]), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
    vn._build_tdata()
    ps, _ = vn.engine.ndiff[0]
    X = vn.engine.batches[0][0]
    np.testing.assert_allclose(ps, velFun(X[:, 0:1], X[:, 1:2]) * np.tile(vn.fixData.dNx[:, 0:1], (vn.fixData.nt, 1)), rtol=1e-13, atol=1e-14)
    vn = VarNet(_pde(nldiff=[0.0, 2.0]), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
    vn._build_tdata()
    assert vn.engine.ndiff[0] == (None, [0.0, 2.0, 0.0])
    # no term: untouched
    vn = VarNet(_pde2(), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
    td = vn._build_tdata()
    fd = vn.fixData
    assert not getattr(vn.engine, 'ndiff', {}) and td.mor[0]['psi'] is None and td.mor[0]['nldiffCoef'] is None
    X, g = vn.engine.batches[0][0], vn.engine.batches[0][1]
    dNx, N = np.tile(fd.dNx[:, 0:1], (fd.nt, 1)), np.tile(np.reshape(fd.N, (-1, 1)), (fd.nt, 1))
    np.testing.assert_array_equal(g, kappaFun(X[:, 0:1], X[:, 1:2]) * dNx + velFun(X[:, 0:1], X[:, 1:2]) * N)


def test_assembly_on_per_row_tables(cpu_engine):
    """Scaled supports (detJvec): gcoef = kappa dNx_rows and psi = (v * dNx_rows).sum(1) + N_rows div v with fixData.rows()."""
    vn = VarNet(_pde2(nldiff=([0.7, 0.4, 0.3], divvFun)), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
    fd = vn.fixData
    fd.updateOptimData(0.5, 0.5)
    assert fd.detJvec
    rng = np.random.default_rng(2)
    Input = np.hstack([rng.uniform(-1, 1, (fd.nT, 1)), rng.uniform(0, 0.5, (fd.nT, 1))])
    biInput = np.hstack([rng.uniform(-1, 1, (sum(fd.biDof), 1)), rng.uniform(0, 0.5, (sum(fd.biDof), 1))])
    d = vn._assemble(Input, biInput, fd.biDof, 0, None)
    Nr, dNxr, _ = fd.rows()
    x, t = Input[:, 0:1], Input[:, 1:2]
    want = (velFun(x, t) * dNxr).sum(1) + 0.3 * Nr.reshape(-1)
    np.testing.assert_allclose(d['psi'].numpy(), want, rtol=1e-13, atol=1e-13 * np.max(np.abs(want)))
    np.testing.assert_allclose(d['gcoef'].numpy(), kappaFun(x, t) * dNxr, rtol=1e-13, atol=1e-15)
    assert d['nldiffCoef'] == [0.7, 0.4, 0.3] and d['N_rows'] is not None


def test_weak_loss_with_unit_diffusivity_is_the_linear_problem_up_to_quadrature(cpu_engine):
    """D = 1 with the advection on the value side is the same PDE as the plain run: the two weak losses differ only by the
    quadrature error of the integration by parts, and the strong residuals agree exactly (the residual keeps v . grad u)."""
    out = {}
    for key, kw in (('plain', {}), ('unit', {'nldiff': ([1.0], divvFun)}), ('on', {'nldiff': ([0.7, 0.4, 0.3], divvFun)})):
        vn = VarNet(_pde2(**kw), layerWidth=[6, 4], discNum=8, bDiscNum=None, tDiscNum=6)
        vn.engine.set_params(vn.engine.get_params() + 0.1)
        comp, _, _ = vn.splitLoss(vn._build_tdata())
        out[key] = (comp, vn.residual()[1], vn.residual()[3])
    (c0, r0, u0), (c1, r1, u1), (c2, r2, _) = out['plain'], out['unit'], out['on']
    np.testing.assert_array_equal(c0[:2], c1[:2])
    assert abs(c1[2, 0] - c0[2, 0]) < 0.05 * abs(c0[2, 0])                  # the same weak form, two quadratures of it
    assert abs(c2[2, 0] - c0[2, 0]) > 10 * abs(c1[2, 0] - c0[2, 0])         # D(u) is a different problem
    np.testing.assert_array_equal(u0, u1)
    np.testing.assert_allclose(r1, r0, rtol=1e-12, atol=1e-14)
    assert np.max(np.abs(r2 - r0)) > 1e-2 * np.max(np.abs(r0))


def _case_lines(path):
    return [ln for ln in open(path).read().splitlines(True) if not ln.startswith('Simulation date')]


def test_case_file_names_the_term_only_when_present(cpu_engine, tmp_path):
    lines = {}
    for key, kw in (('default', {}), ('none', {'nldiff': None}), ('on', {'nldiff': [1.0, 0.0, 2.0]})):
        np.random.seed(0)
        vn = VarNet(_pde(**kw), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
        vn.train(str(tmp_path / key), epochNum=1, saveFreq=1, verbose=False)
        lines[key] = _case_lines(str(tmp_path / key / 'caseData.txt'))
    assert lines['default'] == lines['none'] and not any('diffusivity:' in ln for ln in lines['default'])
    extra = [ln for ln in lines['on'] if 'Solution-dependent diffusivity' in ln]
    assert extra == ['Solution-dependent diffusivity: div(diff*(d0 + d1 c + d2 c^2) grad c), coefficients [1.0, 0.0, 2.0]\n']
