"""
Host tier of the learnt weight scales (vn_set_reparam): the restatement tests/reparam_ref.py against torch autograd of the oracle
loss as a function of (V, s), against central differences, and against oracle.tf1_graph.TF1Adam at f == 1; MEASURED_C of the joint
step measured over every sequence of tests/reparam_cases.py; every named mutant shown to leave the bar in NumPy alone; the argument
checks of the Python layer that need no device.
"""
import numpy as np
import pytest
import torch

from oracle import tf1_graph as og
from tests import reparam_cases as rc
from tests import reparam_ref as rr

AUTOGRAD_RTOL = 1e-12          # the bar of tests/test_ansatz_host.py
FD_RTOL = 1e-7                 # of the gradient's scale
SMALL = [0, 1, 2, 3, 5]        # cases whose fp64 autograd takes well under a second


def test_group_counts_and_membership():
    for i, c in enumerate(rc.CASES):
        widths = c[2]
        for k, (mode, per, n) in enumerate(rc.MODES):
            lay = rc.layout(i, k)
            want = sum(widths) + 1 if mode == 'rwf' else (len(widths) if per == 'layer' else sum(widths))
            assert lay.S == want and lay.P == og.param_count(c[0], widths)
            dims = rr.layer_dims(c[0], widths)
            off = 0
            for l, (fi, fo) in enumerate(dims):
                wg, bg = lay.group[off:off + fi * fo].reshape(fi, fo), lay.group[off + fi * fo:off + fi * fo + fo]
                out = l == len(dims) - 1
                if mode == 'rwf':
                    assert np.all(bg == -1) and np.all(wg == wg[0]) and len(set(wg[0])) == fo          # weights only, one per column
                elif out:
                    assert np.all(wg == -1) and np.all(bg == -1)                                      # hidden layers only
                elif per == 'layer':
                    assert len(set(wg.ravel()) | set(bg)) == 1 and wg[0, 0] >= 0
                else:
                    assert np.all(wg == wg[0]) and np.array_equal(bg, wg[0]) and len(set(bg)) == fo
                off += fi * fo + fo
            # every scale owns at least one entry, in layer order
            assert np.array_equal(np.unique(lay.group[lay.group >= 0]), np.arange(lay.S))


@pytest.mark.parametrize('k', range(len(rc.MODES)), ids=rc.MODE_IDS)
@pytest.mark.parametrize('i', SMALL, ids=[rc.IDS[i] for i in SMALL])
def test_chain_rule_is_autograd(i, k):
    """g_V = f g and g_s = f' sum V g, with g the plain oracle gradient at theta_eff, against autograd through theta_eff(V, s)."""
    lay = rc.layout(i, k)
    s = rc.scales(i, k).astype(np.float64)
    V = lay.factorise(rc.theta(i), s)
    res, gV_ad, gs_ad = rc.autograd_of(i, lay, V, s)
    ref, g = rc.oracle_grad(i, lay.effective(V, s))
    gV, gs = lay.chain(V, s, g)
    assert abs(res['loss'] - ref['loss']) <= AUTOGRAD_RTOL * abs(ref['loss'])
    assert np.max(np.abs(gV - gV_ad)) <= AUTOGRAD_RTOL * np.max(np.abs(gV_ad))
    assert np.max(np.abs(gs - gs_ad)) <= AUTOGRAD_RTOL * max(np.max(np.abs(gs_ad)), np.max(lay.fprime(s) * lay.abs_sums(V, g)))
    assert np.max(np.abs(gs_ad)) > 0.0


@pytest.mark.parametrize('k', [0, 4, 8], ids=[rc.MODE_IDS[k] for k in (0, 4, 8)])
@pytest.mark.parametrize('i', [1, 2], ids=[rc.IDS[1], rc.IDS[2]])
def test_chain_rule_is_central_differences(i, k):
    lay = rc.layout(i, k)
    s = rc.scales(i, k).astype(np.float64)
    V = lay.factorise(rc.theta(i), s)
    _, g = rc.oracle_grad(i, lay.effective(V, s))
    gV, gs = lay.chain(V, s, g)
    loss = lambda V_, s_: rc.oracle_grad(i, lay.effective(V_, s_))[0]['loss']
    rng = np.random.default_rng(9)
    h = 1e-5
    scale = max(np.max(np.abs(gV)), np.max(np.abs(gs)))
    for j in list(rng.choice(lay.P, 6, replace=False)):
        e = np.zeros(lay.P); e[j] = h
        assert abs((loss(V + e, s) - loss(V - e, s)) / (2 * h) - gV[j]) <= FD_RTOL * scale
    for j in range(min(lay.S, 6)):
        e = np.zeros(lay.S); e[j] = h
        assert abs((loss(V, s + e) - loss(V, s - e)) / (2 * h) - gs[j]) <= FD_RTOL * scale


@pytest.mark.parametrize('k', [0, 1, 5], ids=[rc.MODE_IDS[k] for k in (0, 1, 5)])
def test_unit_scale_is_the_plain_tf1_step(k):
    """slope with n = 1 (s = 1) and rwf with s = 0: f == 1 and, as long as s is held there, V takes oracle.tf1_graph.TF1Adam's
    step.  The scales' rate is 0 so that they stay."""
    i = 2
    lay, V0, _, gs = rc.sequence(i, k)
    assert rc.MODES[k][2] == 1.0
    s = np.zeros(lay.S) if lay.mode == 'rwf' else np.ones(lay.S)
    V = np.asarray(rc.theta(i), dtype=np.float64)
    tf = og.TF1Adam(lay.P, lr=rc.LR, dtype=np.float64)
    j = rr.Joint64(lay, rc.LR, 0.0, rounded=False)
    Vt = V.copy()
    for t, g in enumerate(gs, 1):
        V, s, th = j.step(V, s, g.astype(np.float64), t)
        Vt = tf.step(Vt, g.astype(np.float64))
        assert np.max(np.abs(V - Vt)) <= 1e-15 and np.array_equal(th, V)
        assert np.array_equal(s, np.zeros(lay.S) if lay.mode == 'rwf' else np.ones(lay.S))


def run32(i, k):
    """Joint32 over the case's sequence; the state of before every step and Joint64's step from it."""
    lay, V, s, gs = rc.sequence(i, k)
    a = rr.Joint32(lay, rc.LR, rc.LR_S)
    steps = []
    for t, g in enumerate(gs, 1):
        st = dict(t=t, V=V, s=s, g=g, m=a.m, v=a.v, ms=a.ms, vs=a.vs)
        V, s, th = a.step(V, s, g, t)
        st.update(V1=V, s1=s, th1=th, m1=a.m, v1=a.v, ms1=a.ms, vs1=a.vs)
        steps.append(st)
    return lay, steps


def measure(lay, steps):
    """Largest (|Joint32 - Joint64| - ulp / 2) / lr_t over V and s, and the largest slot error over slot_bar."""
    ref = rr.Joint64(lay, rc.LR, rc.LR_S)
    c = slot = 0.0
    for st in steps:
        ref.load(st['m'], st['v'], st['ms'], st['vs'])
        V, s, _ = ref.step(st['V'], st['s'], st['g'], st['t'])
        for got, want, before, lr in ((st['V1'], V, st['V'], rc.LR), (st['s1'], s, st['s'], rc.LR_S)):
            lr_t = rr.lr_t_of(lr, st['t'])
            c = max(c, float(np.max((np.abs(got - want) - rr.bar(before, want, lr_t, c=0.0)) / lr_t)))
        for got, want, before, term in ((st['m1'], ref.m, st['m'], (1 - ref.b1) * ref.gV), (st['v1'], ref.v, st['v'], (1 - ref.b2) * ref.gV ** 2),
                                        (st['ms1'], ref.ms, st['ms'], (1 - ref.b1) * ref.gs), (st['vs1'], ref.vs, st['vs'], (1 - ref.b2) * ref.gs ** 2)):
            slot = max(slot, float(np.max(np.abs(got - want) / rr.slot_bar(before, want, term))))
    return c, slot


def test_measured_c_is_current():
    worst, where, slot = 0.0, None, 0.0
    for i in range(len(rc.CASES)):
        for k in range(len(rc.MODES)):
            c, sl = measure(*run32(i, k))
            slot = max(slot, sl)
            if c > worst:
                worst, where = c, (rc.IDS[i], rc.MODE_IDS[k])
    print('reparam MEASURED_C = %r at %s; worst slot error / slot_bar = %.3f' % (worst, where, slot))
    assert worst > 0.0
    assert abs(worst - rr.MEASURED_C) <= 1e-3 * rr.MEASURED_C, 'tests/reparam_ref.py: MEASURED_C is stale, measured %r' % worst
    assert slot <= 1.0            # the fp32 twin keeps the slots' own bar


@pytest.mark.parametrize('name', rr.MUTANTS)
def test_every_mutant_leaves_the_bar(name):
    """On the sequences the GPU trajectory test runs (tests/reparam_cases.py: TRAJECTORIES), fed Joint32's states: every
    mutant misses the bar somewhere on every sequence it applies to, and applies to at least one."""
    hit = 0
    for i, k in rc.TRAJECTORIES:
        lay, steps = run32(i, k)
        r = rr.replay(name, lay, steps, rc.LR, rc.LR_S)
        if r is None:
            continue
        hit += 1
        assert r > 1.0, (name, rc.IDS[i], rc.MODE_IDS[k], r)
    assert hit > 0


def test_unmutated_replay_keeps_the_bar():
    for i, k in rc.TRAJECTORIES:
        lay, steps = run32(i, k)
        assert rr.replay(None, lay, steps, rc.LR, rc.LR_S) == 0.0


# ---- the Python layer: what needs no device ------------------------------------------------------------------------------
def test_binding_counts_the_scales():
    from varnet_amd.engine import ABI_SYMBOLS, reparam_count, reparam_layers
    for i, c in enumerate(rc.CASES):
        for k, (mode, per, n) in enumerate(rc.MODES):
            lay = rc.layout(i, k)
            assert reparam_count(mode, per, c[0], c[2]) == lay.S
            assert reparam_layers(mode, per, c[2]) == [sl.stop - sl.start for sl in lay.layer_s if sl.stop > sl.start]
    for name in ('vn_set_reparam', 'vn_get_reparam', 'vn_set_reparam_state', 'vn_reparam_grad'):
        assert name in ABI_SYMBOLS


def test_header_declares_the_symbols():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'varnet_hip.h')).read()
    for name in ('vn_set_reparam(', 'vn_get_reparam(', 'vn_set_reparam_state(', 'vn_reparam_grad(', 'VN_REPARAM_RWF = 1', 'VN_REPARAM_SLOPE = 2',
                 'VN_REPARAM_PER_LAYER = 1'):
        assert name in hdr, name
    assert '#define VN_ABI_VERSION 7' in hdr


def test_varnet_argument_checks():
    from varnet_amd.varnet import parse_reparam
    assert parse_reparam(None) is None
    assert parse_reparam('rwf') == dict(kind='rwf', mean=1.0, std=0.1, per='neuron', n=1.0)
    assert parse_reparam({'kind': 'slope', 'n': 10.0, 'per': 'layer'}) == dict(kind='slope', n=10.0, per='layer', mean=None, std=None)
    assert parse_reparam('slope')['n'] == 1.0
    for bad in ('rfw', 3, {'n': 2}, {'kind': 'slope', 'n': 0.5}, {'kind': 'slope', 'per': 'entry'}, {'kind': 'rwf', 'std': -1.0},
                {'kind': 'rwf', 'mean': float('nan')}, {'kind': 'slope', 'n': float('inf')}, {'kind': 'rwf', 'colour': 1}):
        with pytest.raises(ValueError):
            parse_reparam(bad)


def test_varnet_refusals_need_no_device():
    """What VarNet refuses before it builds an engine: another optimizer, towers, a network of the layer-by-layer route, a
    reparamLr without a reparam, a negative reparamLr."""
    from varnet_amd.adpde import ADPDE
    from varnet_amd.domain import Domain1D
    from varnet_amd.varnet import VarNet
    pde = ADPDE(Domain1D(), diff=0.1, vel=1.0, tInterval=[0, 1.0], IC=lambda x: -np.sin(np.pi * x))
    kw = dict(discNum=4, bDiscNum=None, tDiscNum=3)
    for bad, exc in ((dict(reparam='rwf', optimizer='rmsprop'), NotImplementedError), (dict(reparam='rwf', optimizer='lbfgs'), NotImplementedError),
                     (dict(reparam='slope', processors=[0, 1]), NotImplementedError), (dict(reparam='rwf', layerWidth=[128, 128]), NotImplementedError),
                     (dict(reparam='rwf', layerWidth=[20] * 9), NotImplementedError), (dict(reparamLr=1e-3), ValueError),
                     (dict(reparam='rwf', reparamLr=-1.0), ValueError), (dict(reparam='rfw'), ValueError)):
        with pytest.raises(exc):
            VarNet(pde, **dict(kw, **bad))
