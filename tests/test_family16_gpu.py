"""
Reachability of the 8-wave kernel family: every (hidden layers, k-steps) pair of the table in varnet_amd/csrc/vn_fused16_common.h
(VN16_TABLE) that the engine's route accepts has every point kernel -- vn_forward, vn_forward_grad, vn_residual, their fp64 forms
and one gradient of a small weak-form batch return for it, with finite outputs -- and the widest shapes just outside the table go
layer by layer.

No accuracy bar on purpose: accuracy is what the parity and fuzz tests assert, bit-equality of a refactor with its parent is what
tools/family16_ab.py compares (profiles/family16_ab.json).  The cases (networks, parameters, points, batch) are that tool's.
"""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    'family16_ab', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'family16_ab.py'))
ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab)

N = 17          # one full 16-point chunk and a chunk of one point


@pytest.mark.parametrize('act', ['sigmoid', 'tanh'])
@pytest.mark.parametrize('L,KS', ab.family_table(), ids=lambda v: str(v))
def test_every_pair_of_the_table_has_every_kernel(L, KS, act):
    from varnet_amd.engine import VN_KERNEL_FUSED16
    case = ab.make_case(L, KS, act)
    eng = ab.make_engine(case)
    assert eng.kernel_path()[0] == VN_KERNEL_FUSED16
    outs = ab.point_outputs(eng, case, N)            # a missing instantiation raises VNError (hipErrorInvalidValue)
    outs.update(ab.grad_output(eng, case))
    assert tuple(outs['forward'][0].shape) == (N,)
    for name, tensors in outs.items():
        for t in tensors:
            assert bool(torch.isfinite(t).all()), name
    eng.close()


@pytest.mark.parametrize('L', [7, 8])
def test_shapes_just_outside_the_table_run_layer_by_layer(L):
    from varnet_amd.engine import VNEngine, VN_KERNEL_LAYERED
    assert (L, 16) not in ab.family_table()
    eng = VNEngine(ab.DIM, ab.D_IN, [64] * L, True, ab.INTEG_NUM)
    assert eng.kernel_path()[0] == VN_KERNEL_LAYERED
    eng.close()
