"""
The folded edge tile of the 8-wave fused kernel's bf16-piece sweeps (vn_fused16.hip, stage_split_hidden<L, FOLD13>): features 48
and 49 of a 50-wide layer keep their m- and l-pieces in the idle rows (forward sweep) and the idle in-slots (sweep back) of the
piece-0 blocks, and one MFMA per B piece replaces the six of the other row tiles.  Loss, loss terms, loss field and every gradient
block against the fp64 oracle at the bars of the f32 route, and bitwise repeatability, for: both edge features at every depth, one
edge feature (49 wide), none (48 wide: the fourth tile is all padding), mixed edge content from layer to layer; several tiles per
workgroup with a boundary tile behind an interior one; the two-pass route (forward-only and seeded reverse launches).
"""
import numpy as np
import pytest

from tests.parity_cases import synth
from tests.test_fused16_bf16_gpu import FUSED16, GENERIC, check, grad, load, make

pytestmark = pytest.mark.gpu

# (widths, integNum, n_k)
EDGE_NETS = [([50] * 2, 64, 30), ([50] * 3, 64, 30), ([50] * 4, 64, 30), ([50] * 5, 64, 30),      # (a) both edge features, every depth
             ([49] * 4, 64, 30),                                                                   # (b) one edge feature
             ([48] * 4, 64, 30),                                                                   # (c) tile 3 all padding
             ([50, 49, 48, 50, 33], 64, 30)]                                                       # (d) mixed edge content


def run(widths, q, n_k, nB, bDof, act, seed, others=()):
    d = synth(seed, 3, 2, widths, q, n_k, nB, bDof, False, False, False)
    eng = make(widths, q, FUSED16, act)
    assert eng.kernel_path()[0] == 3                                 # the 8-wave fused kernel serves the step
    eng.init_params(seed=seed + 1)
    flat = eng.get_params() + 0.05 * np.random.default_rng(seed + 2).standard_normal(eng.P).astype(np.float32)
    load(eng, d, n_k, bDof, flat)
    g = check(eng, flat, d, widths, q, n_k, bDof, act, 'fused16 %s %s' % (widths, act))
    assert np.array_equal(grad(eng), g)                              # fixed summation order: bitwise repeatable
    eng.close()
    for k in others:
        e = make(widths, q, k, act)
        load(e, d, n_k, bDof, flat)
        check(e, flat, d, widths, q, n_k, bDof, act, 'kernel %d %s %s' % (k, widths, act))
        e.close()


@pytest.mark.parametrize('act', ['sigmoid', 'tanh'])
@pytest.mark.parametrize('net', EDGE_NETS, ids=['-'.join(map(str, n[0])) for n in EDGE_NETS])
def test_folded_edge_tile_against_oracle_and_generic_kernel(net, act):
    widths, q, n_k = net
    run(widths, q, n_k, 200, 120, act, 21, others=[GENERIC])


def test_folded_edge_tile_over_several_tiles_per_workgroup():
    """(e) 750 interior tiles + 2 boundary tiles: every workgroup of a 256-workgroup grid walks two or three tiles, and workgroups
    238 and 239 end on a boundary tile behind their interior ones."""
    run([50] * 5, 64, 1500, 200, 120, 'sigmoid', 31)


def test_folded_edge_tile_on_the_two_pass_route():
    """(f) integNum 216 does not fit a tile: 338 tiles through the forward-only mode (1) and the reverse pass with external seeds
    (2), two tiles on some workgroups."""
    run([50] * 5, 216, 200, 200, 120, 'sigmoid', 41)
