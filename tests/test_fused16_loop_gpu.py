"""
The tile loop of the 8-wave fused kernel's bf16-piece instantiations (vn_fused16.hip, hidden widths 33..50, 2..5 hidden layers)
after its bookkeeping was cut down: fragment reads that reach their (piece, q, row tile) block through an immediate offset from
one lane base per 48 KB window of the weight images, launch-uniform predicates tested as bits of one scalar, border reads of the
weight-gradient rounds from lane bases that carry the image's own address.  What such a change can break -- a wrong block
offset, a wrong window base, a guard turned into an unconditional store, state carried from one tile to the next -- shows as a
wrong loss or gradient block against the fp64 oracle, at the bars of tests/parity_cases.py:

  * every depth (windows 1 and 1 + 2), narrow widths (zero padding inside the second K fragment and the fourth row tile),
    sigmoid and tanh;
  * one tile per workgroup (a single half-filled interior tile plus the BC/IC tiles) and several tiles per workgroup on every CU;
  * the forward-only and the seeded-reverse modes (integNum 216 does not fit a tile: two-pass route).
"""
import numpy as np
import pytest

from tests.gradcheck import assert_grad_close
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, synth
from tests.test_fused16_bf16_gpu import FUSED16, check, grad, load, make, oracle

pytestmark = pytest.mark.gpu

# (widths, integNum, n_k)
NETS = [([50] * 5, 64, 30), ([50] * 4, 64, 30), ([50] * 3, 64, 30), ([50] * 2, 64, 30),
        ([33, 50, 40, 50, 33], 16, 50), ([33, 49], 32, 30)]
NB, BDOF = 200, 120


def perturbed(eng, seed):
    return eng.get_params() + 0.05 * np.random.default_rng(seed).standard_normal(eng.P).astype(np.float32)


@pytest.mark.parametrize('act', ['sigmoid', 'tanh'])
@pytest.mark.parametrize('net', NETS, ids=['-'.join(map(str, n[0])) for n in NETS])
def test_every_block_of_every_layer_against_the_oracle(net, act):
    widths, q, n_k = net
    d = synth(21, 3, 2, widths, q, n_k, NB, BDOF, False, False, False)
    eng = make(widths, q, FUSED16, act)
    assert eng.kernel_path()[0] == 3                                 # the 8-wave fused kernel serves the step
    eng.init_params(seed=8)
    flat = perturbed(eng, 9)
    load(eng, d, n_k, BDOF, flat)
    g = check(eng, flat, d, widths, q, n_k, BDOF, act, 'loop %s %s' % (widths, act))
    assert np.array_equal(grad(eng), g)
    eng.close()


def test_one_tile_and_many_tiles_per_workgroup():
    """n_k = 1: a single interior tile, half filled (64 of 128 points), then the BC/IC tiles -- every workgroup runs the loop body
    at most once.  n_k = 1500: 750 interior tiles, several per workgroup on every CU -- accumulators, stash and lane bases
    carried across tiles.  Both against the fp64 oracle, each bitwise repeatable; the large batch's data is a superset of the
    small one's."""
    widths, q = [50] * 5, 64
    small, large = 1, 1500
    dl = synth(22, 3, 2, widths, q, large, NB, BDOF, False, False, False)
    ds = dict(dl, Input=dl['Input'][:small * q], gcoef=dl['gcoef'][:small * q], N=dl['N'][:small * q], dNt=dl['dNt'][:small * q])
    one = make(widths, q, FUSED16, 'sigmoid')
    one.init_params(seed=10)
    flat = perturbed(one, 11)
    load(one, ds, small, BDOF, flat)
    g_one = check(one, flat, ds, widths, q, small, BDOF, 'sigmoid', 'n_k = 1')
    assert np.array_equal(grad(one), g_one)
    many = make(widths, q, FUSED16, 'sigmoid')
    load(many, dl, large, BDOF, flat)
    g_many = grad(many)
    ref, gref = oracle(flat, dl, widths, q, large, BDOF, 'sigmoid')
    assert abs(g_many[many.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])
    assert np.max(np.abs(g_many[:many.P] - gref)) / np.max(np.abs(gref)) <= GRAD_RTOL
    assert_grad_close(g_many, gref, 3, widths, GRAD_RTOL, dim=2, what='n_k = 1500')
    assert np.array_equal(grad(many), g_many)
    assert np.array_equal(grad(one), g_one)                          # the other engine's launches left this one's state alone
    many.close()
    one.close()


@pytest.mark.parametrize('act', ['sigmoid', 'tanh'])
def test_forward_only_and_seeded_reverse_modes(act):
    widths, q, n_k, nB, bDof = [50] * 5, 216, 12, NB, BDOF
    d = synth(23, 3, 2, widths, q, n_k, nB, bDof, False, False, False)
    eng = make(widths, q, FUSED16, act)
    eng.init_params(seed=12)
    flat = perturbed(eng, 13)
    load(eng, d, n_k, bDof, flat)
    g = check(eng, flat, d, widths, q, n_k, bDof, act, 'two-pass %s' % act)
    assert np.array_equal(grad(eng), g)
    eng.close()
