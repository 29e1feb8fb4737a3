"""
CPU tier of the polynomial reaction term (`ADPDE(reaction=(rate, [c1, c2, c3]))`, vn_set_reaction): the fp64 restatement of
tests/reaction_ref.py against the oracle (zero coefficients: bit for bit) and against central differences, `ADPDE` validation and
the MOR refusal, the declaration and binding of the new entry point, the host assembly of the rate stream through a stand-in
engine (mini-batches and shuffles pick the same rows as the other interior arrays), and reaction-free case files.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests import reaction_ref
from tests.oracle_engine import OracleEngine
from tests.reaction_cases import CASES, COEF, IDS, inputs, ref_kw, reference, reference64, theta
from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.mor import MOR
from varnet_amd.varnet import VarNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pi = np.pi


# ---- the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_zero_coefficients_are_the_oracle_exactly(i):
    d_in, widths = CASES[i][0], CASES[i][2]
    flat = theta(i).astype(np.float64)
    ref, g = og.loss_and_grad(flat, d_in, widths, torch.float64, **ref_kw(i))
    for rate in (inputs(i)[1].astype(np.float64), None):
        got, gg = reaction_ref.loss_and_grad(flat, d_in, widths, (rate, (0.0, 0.0, 0.0)), torch.float64, **ref_kw(i))
        for k in ('loss', 'BCloss', 'ICloss', 'varLoss'):
            assert got[k] == ref[k], (k, got[k], ref[k])
        assert np.array_equal(got['lossVec'], ref['lossVec'])
        assert np.array_equal(gg, g)


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_reference_gradient_against_central_differences(i):
    """<= 1e-4 relative on 6 sampled coordinates (coordinates with |g| < 1e-8 are not judged); the term is a real part of the
    objective on these inputs."""
    ref, g = reference64(i, 'rate')
    ref0, g0 = reference64(i, 'none')
    assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss'])
    assert np.linalg.norm(g - g0) > 1e-2 * np.linalg.norm(g)
    flat = theta(i).astype(np.float64)
    rate = inputs(i)[1]
    h = 1e-5
    judged = 0
    for p in np.random.default_rng(7).choice(flat.size, 6, replace=False):
        if abs(g[p]) < 1e-8:
            continue
        e = np.zeros_like(flat)
        e[p] = h
        fp = reference(i, (rate, COEF), flat + e)[0]['loss']
        fm = reference(i, (rate, COEF), flat - e)[0]['loss']
        fd = (fp - fm) / (2 * h)
        err = abs(fd - g[p]) / abs(g[p])
        print('case %s coordinate %d: autograd %.6e, central difference %.6e, relative %.2e' % (IDS[i], p, g[p], fd, err))
        assert err <= 1e-4, (IDS[i], p, g[p], fd)
        judged += 1
    assert judged >= 3


def test_reference_residual_adds_the_term():
    rng = np.random.default_rng(0)
    n, d_in, dim, widths = 50, 3, 2, [10, 20]
    X = rng.uniform(-1, 1, (n, d_in))
    diff, vel = rng.uniform(0.1, 1, (n, 1)), rng.standard_normal((n, dim))
    src, ddx = rng.standard_normal((n, 1)), rng.standard_normal((n, dim))
    rate = rng.uniform(0.5, 2, (n, 1))
    flat = og.glorot_init(d_in, widths, 3).astype(np.float64)
    u, r0 = og.residual(flat, d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, True)
    u1, r1 = reaction_ref.residual(flat, d_in, widths, torch.float64, X, diff, vel, src, ddx, dim, (rate, COEF), True)
    assert np.array_equal(u, u1)
    np.testing.assert_allclose(r1 - r0, rate * (u - u ** 2 + 0.5 * u ** 3), rtol=1e-12, atol=1e-15)


# ---- ADPDE ------------------------------------------------------------------------------------------------------
def _pde(**kw):
    return ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, vel=0.0, tInterval=[0, 0.5], IC=lambda x: np.sin(pi * x), **kw)


def test_adpde_reaction_argument():
    assert _pde().reaction is None
    p = _pde(reaction=(2.0, [-1.0]))
    assert p.reactionCoef == [-1.0, 0.0, 0.0] and p.reactionRate == 2.0
    np.testing.assert_array_equal(p.reactionRateFun(np.zeros((3, 1)), np.zeros((3, 1))), 2.0 * np.ones((3, 1)))
    f = lambda x, t=0: 1.0 + x ** 2
    p = _pde(reaction=(f, (1.0, -1.0, 0.5)))
    assert p.reactionRateFun is f and p.reactionRate is None and p.reactionCoef == [1.0, -1.0, 0.5]
    for bad in (1.0, (1.0,), (1.0, [1, 2, 3, 4]), (1.0, []), ('fast', [1.0]), (1.0, [np.nan]), (1.0, 'abc'), (np.inf, [1.0])):
        with pytest.raises(ValueError, match='reaction'):
            _pde(reaction=bad)
    assert 'rate * (c1 c + c2 c^2 + c3 c^3)' in ADPDE.__doc__


def test_mor_with_reaction_raises():
    def diffFun(x, t=0, D=0.01):
        return D * np.ones([len(x), 1])

    mor = MOR(diffFun, ['D'], [[0.003, 0.033]])
    with pytest.raises(NotImplementedError, match='parametric reaction rates are out of scope'):
        ADPDE(Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0], IC=lambda x: -np.sin(pi * x),
              MORvar=mor, reaction=(1.0, [-1.0]))


# ---- ABI --------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_bound():
    from varnet_amd import engine as vengine
    hdr = open(os.path.join(ROOT, 'include', 'varnet_hip.h')).read()
    assert re.search(r'int\s+vn_set_reaction\s*\(\s*vn_engine\s*\*\s*h,\s*int32_t\s+batch,\s*const\s+float\s*\*\s*rate_dev,'
                     r'\s*const\s+double\s+coef\[3\]\s*\)\s*;', hdr)
    assert re.search(r'#define\s+VN_ABI_VERSION\s+7\b', hdr) and vengine.VN_ABI_VERSION == 7
    assert 'vn_set_reaction' in vengine.ABI_SYMBOLS
    assert callable(getattr(vengine.VNEngine, 'set_reaction'))
    if os.path.exists(vengine.LIB_PATH):                       # (needs the built library)
        assert hasattr(vengine.load_library(), 'vn_set_reaction')


# ---- VarNet host layer through a stand-in engine ----------------------------------------------------------------------
class ReactOracleEngine(OracleEngine):
    """The oracle engine with vn_set_reaction: batches with a registration are evaluated by tests/reaction_ref.py."""

    def set_interior(self, batch, *a, **kw):
        super().set_interior(batch, *a, **kw)
        self.__dict__.setdefault('react', {}).pop(batch, None)          # vn_set_interior clears the registration

    def set_reaction(self, batch, rate=None, coef=None):
        self.__dict__.setdefault('react', {})
        c = [] if coef is None else [float(x) for x in coef]
        if not any(c):
            self.react.pop(batch, None)
            return
        n = self.batches[batch][0].shape[0]
        r = None if rate is None else np.array(rate.numpy() if isinstance(rate, torch.Tensor) else rate, dtype=float).reshape(-1, 1)
        assert r is None or r.shape[0] == n
        self.react[batch] = (r, c + [0.0] * (3 - len(c)))

    def _eval(self, batch):
        rc = getattr(self, 'react', {}).get(batch)
        if rc is None:
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
        return reaction_ref.loss_and_grad(self.theta.astype(np.float64), self.inpDim, self.layerWidth, rc, torch.float64, **kw)

    def residual(self, X, diff, vel, source=None, diff_dx=None, fp64=False, reaction=None):
        u, r = super().residual(X, diff, vel, source, diff_dx, fp64)
        if reaction is not None:
            rate, coef = reaction
            r = r + torch.as_tensor(np.reshape(rate, -1)) * reaction_ref.poly(u, coef)
        return u, r


@pytest.fixture
def cpu_engine(monkeypatch):
    def make(self, processors):
        fd = self.fixData
        return ReactOracleEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                                 isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                                 learning_rate=self.learning_rate)
    monkeypatch.setattr(VarNet, '_make_engine', make)


def rateFun(x, t=0):
    return 1.0 + 0.5 * x ** 2 + t


def test_rate_stream_follows_the_rows_of_every_batch(cpu_engine):
    vn = VarNet(_pde(reaction=(rateFun, [1.0, -1.0, 0.5])), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
    eng = vn.engine
    td = vn._build_tdata(batchNum=3)
    for shuffled in (False, True):
        if shuffled:
            np.random.seed(3)
            td.shuffleTrainData()
        seen = 0
        for bi in range(td.batchNum):
            rate, coef = eng.react[bi]
            X = eng.batches[bi][0]
            assert coef == [1.0, -1.0, 0.5]
            np.testing.assert_allclose(rate, rateFun(X[:, 0:1], X[:, 1:2]).astype(np.float64), rtol=1e-15)
            seen += len(rate)
        assert seen == vn.fixData.nt * vn.fixData.integNum
    # a constant rate is folded into the coefficients: no stream
    vn = VarNet(_pde(reaction=(2.0, [-1.0, 0.25])), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
    vn._build_tdata()
    assert vn.engine.react[0][0] is None and vn.engine.react[0][1] == [-2.0, 0.5, 0.0]


def test_loss_and_residual_see_the_term(cpu_engine):
    out = {}
    for key, kw in (('off', {}), ('on', {'reaction': (rateFun, [1.0, -1.0, 0.5])})):
        vn = VarNet(_pde(**kw), layerWidth=[6, 4], discNum=8, bDiscNum=None, tDiscNum=6)
        vn.engine.set_params(vn.engine.get_params() + 0.1)
        comp, _, _ = vn.splitLoss(vn._build_tdata())
        out[key] = (comp, vn.residual()[1], vn.residual()[3], vn.fixData.uniform_input)
    (c0, r0, u0, X), (c1, r1, u1, _) = out['off'], out['on']
    np.testing.assert_array_equal(c0[:2], c1[:2])
    assert abs(c1[2, 0] - c0[2, 0]) > 1e-2 * abs(c0[2, 0])
    np.testing.assert_array_equal(u0, u1)
    np.testing.assert_allclose(r1 - r0, rateFun(X[:, 0:1], X[:, 1:2]) * (u0 - u0 ** 2 + 0.5 * u0 ** 3), rtol=1e-9, atol=1e-12)


def _case_lines(path):
    return [ln for ln in open(path).read().splitlines(True) if not ln.startswith('Simulation date')]


def test_case_file_names_the_term_only_when_present(cpu_engine, tmp_path):
    lines = {}
    for key, kw in (('default', {}), ('none', {'reaction': None}), ('on', {'reaction': (2.0, [1.0, -1.0])})):
        np.random.seed(0)
        vn = VarNet(_pde(**kw), layerWidth=[5], discNum=8, bDiscNum=None, tDiscNum=6)
        vn.train(str(tmp_path / key), epochNum=1, saveFreq=1, verbose=False)
        lines[key] = _case_lines(str(tmp_path / key / 'caseData.txt'))
    assert lines['default'] == lines['none'] and not any('Reaction' in ln for ln in lines['default'])
    extra = [ln for ln in lines['on'] if 'Reaction' in ln]
    assert extra == ['Reaction term: rate*(c1 c + c2 c^2 + c3 c^3), coefficients [1.0, -1.0, 0.0]\n']
