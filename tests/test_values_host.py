"""CPU tier of the value-regime parity suite (tests/value_cases.py): assertions on the references alone, which make the GPU tier
(tests/test_values_gpu.py) meaningful -- the bars need no widening on these cases, the transforms reach the regime they are
named after, and a route that ignored a transform would miss the bars.  The kernels' activation formula restated in float32
(value_cases.formula_loss_and_grad) is measured against the fp64 oracle here: the yardstick of the GPU tier's miss rule."""
import numpy as np
import pytest

from tests import value_cases as vc
from tests.gradcheck import block_errors, fp32_deviation
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL

KEYS = ('loss', 'BCloss', 'ICloss', 'varLoss')
CASES = [(n, a) for n in vc.NETS for a in vc.ACTS]


def loss_dev(res, ref):
    return max(abs(res[k] - ref[k]) / abs(ref[k]) for k in KEYS if ref[k] != 0.0)


@pytest.mark.parametrize('net,act', CASES)
def test_the_bars_need_no_widening(net, act):
    """The fp32 oracle stays within a quarter of the GPU bars of the fp64 oracle, on every gradient block and on the loss and
    each of its components, under every transform (and under `tiny` of the optimizer-step tests)."""
    d_in, dim, widths, q, n_k, td = vc.NETS[net]
    for tr in vc.TRANSFORMS + ('tiny',):
        r64, g64 = vc.oracle(net, tr, act)
        r32, g32 = vc.oracle(net, tr, act, False)
        dev = fp32_deviation(g32, g64, d_in, widths, dim, td)
        worst = max(dev, key=dev.get)
        print('%s %s %s: fp32 oracle gradient %.2e (%s), loss %.2e' % (net, tr, act, dev[worst], worst, loss_dev(r32, r64)))
        assert np.all(np.isfinite(g64)) and np.all(np.isfinite(g32))
        assert dev[worst] <= GRAD_RTOL / 4, (tr, worst, dev[worst])
        assert loss_dev(r32, r64) <= LOSS_RTOL / 4, (tr, loss_dev(r32, r64))


@pytest.mark.parametrize('net,act', CASES)
def test_planted_units_saturate_and_the_others_do_not(net, act):
    d_in, dim, widths, q, n_k, td = vc.NETS[net]
    c = abs(vc.act_const(act))
    for (z, a), wd in zip(vc.hidden_preacts(net, 'planted', act), widths):
        units = list(vc.planted_units(wd))
        rest = np.setdiff1d(np.arange(wd), units)
        assert np.all(c * np.abs(z[:, units]) > 128.0)
        lo = -1.0 if act == 'tanh' else 0.0
        assert np.array_equal(a[:, units], np.broadcast_to(np.where(np.array(vc.PLANT) > 0, 1.0, lo).astype(np.float32), (len(a), 4)))
        assert np.all(c * np.abs(z[:, rest]) < 64.0)


@pytest.mark.parametrize('net,act', CASES)
def test_offset_is_compensated_and_cancels(net, act):
    """The fp64 loss is the plain one within 1e-5 (the fp32 rounding of b1 is all that differs), and the first layer's terms are
    50 times its result in the median at offset 100 (half the offset where a net runs a smaller one: the same ratio)."""
    d_in, dim, widths, q, n_k, td = vc.NETS[net]
    plain, off = vc.oracle(net, 'plain', act)[0], vc.oracle(net, 'offset100', act)[0]
    assert abs(off['loss'] - plain['loss']) <= 1e-5 * abs(plain['loss'])
    d = vc.inputs(net, 'offset100')[0]
    flat = vc.theta(net, 'offset100').astype(np.float64)
    W1 = flat[:d_in * widths[0]].reshape(d_in, widths[0])
    b1 = flat[vc.bias_slices(d_in, widths)[0]]
    X = np.concatenate([d['Input'], d['biInput']]).astype(np.float64)
    terms = np.abs(X) @ np.abs(W1) + np.abs(b1)
    ratio = float(np.median(terms / np.abs(X @ W1 + b1)))
    print('%s %s: median cancellation %.1f at offset %g' % (net, act, ratio, vc.scale(net, 'offset100')))
    assert ratio >= 0.5 * vc.scale(net, 'offset100')


@pytest.mark.parametrize('net,act', CASES)
def test_shrunk_is_small(net, act):
    assert max(float(np.abs(z).max()) for z, _ in vc.hidden_preacts(net, 'shrunk', act)) < 2e-2


@pytest.mark.parametrize('net,act', CASES)
def test_transforms_are_visible_at_the_bars(net, act):
    """Each transform that changes the function or the data moves the fp64 loss or some gradient block by more than 100 bars."""
    d_in, dim, widths, q, n_k, td = vc.NETS[net]
    r0, g0 = vc.oracle(net, 'plain', act)
    for tr in ('planted', 'steep4', 'scaled_down', 'scaled_up', 'mixed', 'shrunk'):
        r, g = vc.oracle(net, tr, act)
        moved = max(abs(r['loss'] - r0['loss']) / abs(r0['loss']) / LOSS_RTOL,
                    max(block_errors(g, g0, d_in, widths, dim, td).values()) / GRAD_RTOL)
        assert moved > 100.0, (tr, moved)


def test_planted800_overflows_exp_in_double():
    for net in vc.NETS:
        d_in, dim, widths, q, n_k, td = vc.NETS[net]
        flat = vc.theta(net, 'planted800')
        for s, wd in zip(vc.bias_slices(d_in, widths), widths):
            assert np.array_equal(flat[s][list(vc.planted_units(wd))], 8 * np.array(vc.PLANT, dtype=np.float32))
    with np.errstate(over='ignore'):
        assert np.isinf(np.exp(np.float64(800.0) - 5.0))
    r, g = vc.oracle('5x50', 'planted800', 'tanh')
    assert np.isfinite(r['loss']) and np.all(np.isfinite(g))


def test_the_formula_restatement_is_the_loss_and_its_gradient():
    """With the exact activation in double the restatement is the oracle (1e-11: two fp64 evaluations of one function)."""
    for net, tr, act in (('3x20', 'plain', 'sigmoid'), ('40_50_34', 'mixed', 'tanh'), ('5x50_steady', 'scaled_down', 'tanh'),
                         ('4x50_mor', 'planted', 'sigmoid')):
        d_in, dim, widths, q, n_k, td = vc.NETS[net]
        r64, g64 = vc.oracle(net, tr, act)
        r, g = vc.formula_loss_and_grad(net, tr, act, dt=np.float64, actf=vc.exact_act)
        assert loss_dev(r, r64) <= 1e-11
        assert np.max(np.abs(r['lossVec'] - r64['lossVec'].reshape(-1))) <= 1e-11 * np.max(np.abs(r64['lossVec']))
        assert max(block_errors(g, g64, d_in, widths, dim, td).values()) <= 1e-11


@pytest.mark.parametrize('tr', vc.TRANSFORMS)
def test_kernel_formula_yardstick(tr):
    """The float32 restatement with a = rcp(1 + exp2(c z)), tanh = 2a - 1 against the fp64 oracle, printed per case: finite
    under every transform (saturated units included), inside the bars wherever the fp32 oracle is, except where tanh's
    pre-activations are all small -- there its gradient leaves the bar on the CPU already, by the formula alone."""
    worst = {}
    for net in vc.NETS:
        d_in, dim, widths, q, n_k, td = vc.NETS[net]
        for act in vc.ACTS:
            r64, g64 = vc.oracle(net, tr, act)
            r, g = vc.kernel_formula(net, tr, act)
            dev = block_errors(g, g64, d_in, widths, dim, td)
            b = max(dev, key=dev.get)
            print('%s %s %s: kernel formula gradient %.2e (%s), loss %.2e' % (net, tr, act, dev[b], b, loss_dev(r, r64)))
            assert np.all(np.isfinite(g)) and np.isfinite(r['loss'])
            assert loss_dev(r, r64) <= LOSS_RTOL
            worst[act] = max(worst.get(act, 0.0), dev[b])
    print('%s: worst kernel-formula gradient deviation %s' % (tr, worst))
    assert worst['sigmoid'] <= GRAD_RTOL
    if tr == 'shrunk':
        assert worst['tanh'] > GRAD_RTOL            # the cancellation of 2 sigmoid(2z) - 1: an ulp of 0.5 on a value near 0
    else:
        assert worst['tanh'] <= GRAD_RTOL
