"""
The 8-wave fused kernel's hidden-layer sweeps as bf16-piece products (vn_fused16.hip, bf_sweeps: hidden widths 33..50, 2..5 hidden
layers): loss, loss terms, loss field and every gradient block against the fp64 oracle at the bars of the f32 route, for sigmoid and
tanh, full, narrow and mixed widths; the same inputs through the 4-wave f32 kernel (cross-check library) and the generic kernels;
the forward-only and reverse-with-seeds modes (two-pass route); bitwise repeatability; and the per-workgroup weight-gradient stash
in global memory across grids, batches and engines.
"""
import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests.gradcheck import assert_grad_close
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL, synth

pytestmark = pytest.mark.gpu

FUSED16, FUSED32, GENERIC = 3, 2, 1

# (widths, integNum, n_k): 50 wide (the headline net), 40 and 33 wide (padding inside the second K fragment), mixed widths
NETS = [([50] * 5, 64, 40), ([40] * 5, 64, 30), ([33, 50, 40, 50, 33], 16, 50),
        ([50] * 4, 64, 30), ([33] * 4, 32, 40), ([50, 35, 48, 50], 64, 20),
        ([50] * 3, 64, 30), ([40, 50, 34], 16, 60),
        ([50] * 2, 64, 30), ([33, 49], 32, 40)]


def make(widths, q, kernel, act):
    from varnet_amd.engine import VNEngine
    return VNEngine(2, 3, widths, True, q, kernel=kernel, activationFun=act)


def load(eng, d, n_k, bDof, flat, batch=0):
    eng.set_params(flat)
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_interior(batch, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
    eng.set_weights(d['w'])


def oracle(flat, d, widths, q, n_k, bDof, act, dtype=torch.float64):
    f = np.float64 if dtype == torch.float64 else np.float32
    c = lambda a: None if a is None else a.astype(f)
    return og.loss_and_grad(
        flat.astype(f), 3, widths, dtype, Input=c(d['Input']), gcoef=c(d['gcoef']), source=c(d['source']), N=c(d['N']),
        dNt=c(d['dNt']), integW=c(d['integW']), intShape=[n_k, q], detJ=float(d['detJ']), detJvec=False,
        biInput=c(d['biInput']), biLabel=c(d['biLabel']), bDof=bDof, biDimVal=2.0, w=d['w'], dim=2, time_dependent=True,
        is_source=False, integWflag=False, activation=act)


def grad(eng, batch=0):
    gb = eng.bind_grad_buffer()
    eng.grad(batch)
    torch.cuda.synchronize()
    return gb.cpu().numpy().copy()


def check(eng, flat, d, widths, q, n_k, bDof, act, what):
    ref, gref = oracle(flat, d, widths, q, n_k, bDof, act)
    out, lv = eng.eval_loss(0, lossVec=True)
    for got, key in zip(out, ['loss', 'BCloss', 'ICloss', 'varLoss']):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (what, key, got, ref[key])
    lref = ref['lossVec'].reshape(-1)
    assert np.max(np.abs(lv.cpu().numpy() - lref)) <= LVEC_RTOL * np.max(np.abs(lref)), what
    g = grad(eng)
    assert abs(g[eng.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']), what
    assert np.max(np.abs(g[:eng.P] - gref)) / np.max(np.abs(gref)) <= GRAD_RTOL, what
    assert_grad_close(g, gref, 3, widths, GRAD_RTOL, dim=2, what=what,
                      g32=lambda: oracle(flat, d, widths, q, n_k, bDof, act, torch.float32)[1])
    return g


@pytest.mark.parametrize('act', ['sigmoid', 'tanh'])
@pytest.mark.parametrize('net', NETS, ids=['-'.join(map(str, n[0])) for n in NETS])
def test_bf16_sweeps_against_oracle_and_other_kernels(net, act):
    widths, q, n_k = net
    nB, bDof = 200, 120
    d = synth(11, 3, 2, widths, q, n_k, nB, bDof, False, False, False)
    eng = make(widths, q, FUSED16, act)
    assert eng.kernel_path()[0] == 3                                 # the 8-wave fused kernel serves the step
    eng.init_params(seed=4)
    flat = eng.get_params() + 0.05 * np.random.default_rng(6).standard_normal(eng.P).astype(np.float32)
    load(eng, d, n_k, bDof, flat)
    g = check(eng, flat, d, widths, q, n_k, bDof, act, 'fused16 %s %s' % (widths, act))
    assert np.array_equal(grad(eng), g)                              # fixed summation order: bitwise repeatable
    eng.close()
    # the 4-wave kernel (sigmoid only) has no 2-layer instantiation beyond 32 wide
    others = [GENERIC] + ([FUSED32] if len(widths) >= 3 and act == 'sigmoid' else [])
    for k in others:
        e = make(widths, q, k, act)
        load(e, d, n_k, bDof, flat)
        check(e, flat, d, widths, q, n_k, bDof, act, 'kernel %d %s %s' % (k, widths, act))
        e.close()


@pytest.mark.parametrize('act', ['sigmoid', 'tanh'])
def test_bf16_sweeps_forward_only_and_seeded_reverse(act):
    """integNum 216 does not fit a tile: the two-pass route runs the kernel's forward-only mode (1) and its reverse pass with
    external seeds (2)."""
    widths, q, n_k, nB, bDof = [50] * 5, 216, 12, 150, 100
    d = synth(12, 3, 2, widths, q, n_k, nB, bDof, False, False, False)
    eng = make(widths, q, FUSED16, act)
    eng.init_params(seed=5)
    flat = eng.get_params() + 0.05 * np.random.default_rng(7).standard_normal(eng.P).astype(np.float32)
    load(eng, d, n_k, bDof, flat)
    g = check(eng, flat, d, widths, q, n_k, bDof, act, 'two-pass %s' % act)
    assert np.array_equal(grad(eng), g)
    eng.close()


def test_stash_across_grids_batches_and_engines():
    """The weight-gradient stash is per workgroup in global memory, sized by the engine for the grid of each launch: a small
    batch (few workgroups), then a large one (one per CU), then the small one again must give the small batch's bits; a second
    engine in the same process gives the same bits on the same data."""
    widths, q = [50] * 5, 64
    nB, bDof = 200, 120
    small, large = 12, 1500
    dl = synth(13, 3, 2, widths, q, large, nB, bDof, False, False, False)
    ds = dict(dl, Input=dl['Input'][:small * q], gcoef=dl['gcoef'][:small * q], N=dl['N'][:small * q], dNt=dl['dNt'][:small * q])
    eng = make(widths, q, FUSED16, 'sigmoid')
    eng.init_params(seed=6)
    flat = eng.get_params()
    load(eng, ds, small, bDof, flat, batch=0)
    eng.set_interior(1, dl['Input'], dl['gcoef'], dl['source'], n_k=large, detJ=dl['detJ'])
    g_small = check(eng, flat, ds, widths, q, small, bDof, 'sigmoid', 'small batch')
    g_large = grad(eng, 1)
    ref, gref = oracle(flat, dl, widths, q, large, bDof, 'sigmoid')
    assert abs(g_large[eng.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
    assert_grad_close(g_large, gref, 3, widths, GRAD_RTOL, dim=2, what='large batch')
    assert np.array_equal(grad(eng, 0), g_small)
    other = make(widths, q, FUSED16, 'sigmoid')
    load(other, ds, small, bDof, flat)
    assert np.array_equal(grad(other), g_small)
    assert np.array_equal(grad(eng, 1), g_large)
    other.close()
    eng.close()
