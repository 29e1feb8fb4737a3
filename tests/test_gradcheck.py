"""CPU tests of the per-block gradient check (tests/gradcheck.py): its partition of the parameter vector, negative controls
(perturbed input-layer gradients that the old global metric lets through and the per-block check must catch, naming the
block), and a positive control (the oracle's own fp32 evaluation passes against fp64 on every engine case)."""
import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests.gradcheck import (assert_grad_close, assert_pair_close, block_errors, column_errors, global_error,
                             input_names, param_blocks)
from tests.parity_cases import CASES, GRAD_RTOL, STEADY, oracle_eval, steady_inputs, steady_oracle, synth


@pytest.mark.parametrize('d_in,widths', [(d, w) for d in range(1, 33) for w in ([20], [50] * 5)] +
                         [(3, [7, 128, 3]), (5, [33, 50, 41, 17, 50, 50, 50, 50]), (8, [60, 64, 51, 64, 56, 63]),
                          (32, [300, 1, 2])])
def test_blocks_partition_the_parameter_vector(d_in, widths):
    blocks = param_blocks(d_in, widths)
    P = og.param_count(d_in, widths)
    cover = np.zeros(P, dtype=np.int64)
    for _, s in blocks:
        assert s.stop > s.start
        cover[s] += 1
    assert np.all(cover == 1)
    names = [n for n, _ in blocks]
    assert len(set(names)) == len(names)
    assert len(blocks) == d_in + 2 * len(widths) + 1
    # every block is one tensor (or one input row of W1) of og.unflatten's layout
    flat = np.arange(P, dtype=np.float64)
    params = og.unflatten(flat, d_in, widths)
    byname = dict(blocks)
    for k in range(d_in):
        assert np.array_equal(flat[byname['W1.in%d' % k]], params[0][0][k].numpy())
    assert np.array_equal(flat[byname['b1']], params[0][1].numpy())
    for l in range(1, len(widths)):
        assert np.array_equal(flat[byname['W%d' % (l + 1)]], params[l][0].numpy().reshape(-1))
        assert np.array_equal(flat[byname['b%d' % (l + 1)]], params[l][1].numpy())
    assert np.array_equal(flat[byname['Wo']], params[-1][0].numpy().reshape(-1))
    assert np.array_equal(flat[byname['bo']], params[-1][1].numpy())


def test_input_columns_are_named_by_what_they_carry():
    assert input_names(2, 1) == ['x0', 't']
    assert input_names(3, 2) == ['x0', 'x1', 't']
    assert input_names(6, 2) == ['x0', 'x1', 't', 'p0', 'p1', 'p2']
    assert input_names(8, 3) == ['x0', 'x1', 'x2', 't', 'p0', 'p1', 'p2', 'p3']
    assert input_names(3, 2, td=False) == ['x0', 'x1', 'p0']          # steady: the extra column is not time
    assert input_names(1, 1, td=False) == ['x0']
    assert input_names(4) == ['in0', 'in1', 'in2', 'in3']
    assert [n for n, _ in param_blocks(3, [5, 6], dim=2)] == ['W1.x0', 'W1.x1', 'W1.t', 'b1', 'W2', 'b2', 'Wo', 'bo']


def test_zero_reference_block_uses_the_floor():
    g = np.array([1.0, 0.0, 0.0, 0.0, 0.0])              # d_in 1, widths [1]: W1, b1, Wo, bo
    gref = g.copy()
    gref[1] = 0.0
    g[1] = 1e-8
    e = block_errors(g, gref, 1, [1])
    assert e['b1'] == pytest.approx(1e-8 / 1e-7)          # relative to 1e-7 |gref|_inf, not to zero
    assert e['W1.in0'] == 0.0


def _case_gradients(i):
    d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec = CASES[i]
    d = synth(1, d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec)
    flat = og.glorot_init(d_in, widths, 3)                # the engine's init_params(seed=3), bit for bit
    flat = flat + 0.05 * np.random.default_rng(5).standard_normal(flat.size).astype(np.float32)
    _, g64 = oracle_eval(flat, d, d_in, dim, widths, q, n_k, bDof, source, integW, detJvec)
    return d_in, dim, widths, np.asarray(g64, dtype=np.float64)


def _w1(d_in, widths):
    return slice(0, d_in * widths[0])


@pytest.mark.parametrize('i', [6, 22, 26, 27])
@pytest.mark.parametrize('perturb', ['W1_scaled_1.05', 'W1_rows_0_1_swapped', 'b1_scaled_1.1'])
def test_negative_controls_pass_the_old_metric_and_fail_per_block(i, perturb):
    d_in, dim, widths, gref = _case_gradients(i)
    g = gref.copy()
    H = widths[0]
    if perturb == 'W1_scaled_1.05':
        g[_w1(d_in, widths)] *= 1.05
        expect = ('W1.',)
    elif perturb == 'W1_rows_0_1_swapped':
        g[0:H], g[H:2 * H] = gref[H:2 * H].copy(), gref[0:H].copy()
        expect = ('W1.x0', 'W1.x1')
    else:
        b1 = slice(d_in * H, d_in * H + H)
        g[b1] *= 1.1
        expect = ('b1',)
    old = global_error(g, gref)
    assert old <= GRAD_RTOL, old                          # the gap: the suite's old metric lets it through
    with pytest.raises(AssertionError) as ei:
        assert_grad_close(g, gref, d_in, widths, GRAD_RTOL, dim=dim, global_bar=1.0)
    msg = str(ei.value)
    named = msg.split('gradient block ')[1].split(' ')[0]
    assert named.startswith(expect), msg
    assert 'of |g_ref|_inf' in msg and 'bar 1.0e-04' in msg
    # the pairwise form catches it too (route against route)
    with pytest.raises(AssertionError, match='gradient block (%s)' % '|'.join(expect)):
        assert_pair_close(g, gref, d_in, widths, 3e-4, dim=dim, global_bar=1.0)


def test_conditioning_rule_is_per_block_and_only_where_fp32_itself_deviates():
    d_in, widths = 2, [3]
    P = og.param_count(d_in, widths)
    rng = np.random.default_rng(0)
    gref = rng.uniform(1, 2, P)
    g = gref.copy()
    g[0] *= 1 + 5e-4                                      # W1.x0 misses the bar
    g32_ok = gref.copy()
    g32_ok[0] *= 1 + 3e-4                                 # the fp32 oracle deviates there as much: conditioned, passes
    rec = assert_grad_close(g, gref, d_in, widths, 1e-4, g32=lambda: g32_ok, dim=1, global_bar=1e-3)
    assert list(rec['conditioned']) == ['W1.x0']
    g32_other = gref.copy()
    g32_other[P - 1] *= 1 + 3e-4                          # fp32 deviates on ANOTHER block: no allowance for W1.x0
    with pytest.raises(AssertionError, match='W1.x0'):
        assert_grad_close(g, gref, d_in, widths, 1e-4, g32=lambda: g32_other, dim=1, global_bar=1e-3)
    calls = []
    assert_grad_close(gref, gref, d_in, widths, 1e-4, g32=lambda: calls.append(1), dim=1)
    assert not calls                                      # the fp32 oracle runs only when a block misses the bar


def test_column_errors_judge_each_direction_on_its_own_scale():
    ref = np.stack([np.linspace(1, 2, 50), 1e-5 * np.linspace(-1, 1, 50)], axis=1)
    v = ref.copy()
    v[:, 1] *= -1                                         # wrong sign in the small direction
    assert np.max(np.abs(v - ref)) / np.max(np.abs(ref)) < 1e-4
    assert column_errors(v, ref)[1] == pytest.approx(2.0)


@pytest.mark.parametrize('i', range(len(CASES)))
def test_fp32_oracle_passes_per_block_on_every_case(i):
    """Positive control: a correct fp32 evaluation (the oracle's own) reaches the per-block bar on every engine case."""
    d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec = CASES[i]
    d = synth(1, d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec)
    flat = og.glorot_init(d_in, widths, 3)
    flat = flat + 0.05 * np.random.default_rng(5).standard_normal(flat.size).astype(np.float32)
    _, g64 = oracle_eval(flat, d, d_in, dim, widths, q, n_k, bDof, source, integW, detJvec)
    _, g32 = oracle_eval(flat, d, d_in, dim, widths, q, n_k, bDof, source, integW, detJvec, dtype=torch.float32)
    assert_grad_close(g32, g64, d_in, widths, GRAD_RTOL, dim=dim)


@pytest.mark.parametrize('i', range(len(STEADY)))
def test_fp32_oracle_passes_per_block_on_every_steady_case(i):
    case = STEADY[i]
    d, flat = steady_inputs(case)
    _, g64 = steady_oracle(flat, d, case)
    _, g32 = steady_oracle(flat, d, case, torch.float32)
    assert_grad_close(g32, g64, case[0], case[2], GRAD_RTOL, dim=case[1], td=False)
