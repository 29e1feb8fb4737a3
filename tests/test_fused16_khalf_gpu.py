"""
The paired K halves of the 8-wave fused kernel's bf16 sweeps (vn_fused16_common.h: five_khalf / three_khalf, the 20-block image of
stage_split_hidden<L, FOLD13>): in the second K fragment of both sweeps the three full K halves and the edge halves of the three pieces
share MFMAs, 11 per row tile and stream instead of 12, and the stashed layer of weight-gradient accumulators lives in the LDS the
smaller image frees.  Loss, loss terms, loss field and every gradient block against the fp64 oracle at the bars of the f32 route, bitwise
repeatability, and the generic kernel on the same data, for: both edge features at depths 2..5 (L = 2: no stash; 3..5: the LDS stash),
one edge feature (49 wide), none (48), a layer that ends inside the first half of the second fragment (33), mixed widths; several tiles
per workgroup with a boundary tile last; the two-pass route.  tests/test_fused16_khalf_host.py checks the arrangement itself, product
by product.
"""
import pytest

from tests.test_fused16_bf16_gpu import GENERIC
from tests.test_fused16_fold_gpu import run

pytestmark = pytest.mark.gpu

# (widths, integNum, n_k)
KHALF_NETS = [([50] * 2, 64, 30), ([50] * 3, 64, 30), ([50] * 4, 64, 30), ([50] * 5, 64, 30),
              ([49] * 4, 64, 30), ([48] * 4, 64, 30), ([33] * 3, 64, 30), ([50, 49, 48, 50, 33], 64, 30)]


@pytest.mark.parametrize('act', ['sigmoid', 'tanh'])
@pytest.mark.parametrize('net', KHALF_NETS, ids=['-'.join(map(str, n[0])) for n in KHALF_NETS])
def test_khalf_sweeps_against_oracle_and_generic_kernel(net, act):
    widths, q, n_k = net
    run(widths, q, n_k, 200, 120, act, 51, others=[GENERIC])


def test_khalf_sweeps_over_several_tiles_per_workgroup():
    """1 500 test functions: 750 interior tiles + 2 boundary tiles, two or three tiles per workgroup of a 256-workgroup grid -- the LDS
    stash carries layer 2's accumulators from tile to tile -- and a boundary tile last on two of them."""
    run([50] * 5, 64, 1500, 200, 120, 'sigmoid', 61)


def test_khalf_sweeps_on_the_two_pass_route():
    """integNum 216 does not fit a tile: the forward-only launch and the seeded reverse launch, 338 tiles"""
    run([50] * 5, 216, 200, 200, 120, 'tanh', 71)
