"""
GPU tier of the self-adaptive test-function weights (vn_set_tf_adapt, vn_get_tf_adapt, vn_set_tf_adapt_state,
`VarNet(tfAdapt=...)`):

    var = sum_k omega_k l_k,  omega_k = m(lambda_k) / Z of the COMMITTED state, constant for the gradient;
    the update of lambda is formed from the step's own l_k and committed by the optimizer step: omega lags one step.

1. Weights in use are the committed ones: loss components, the unweighted loss field and the gradient against the fp64
   restatement (tests/causal_ref.py) evaluated with the engine's OWN omega (read through vn_get_tf_adapt) as static weights, at the
   project's unchanged bars (tests/parity_cases.py: LOSS_RTOL, LVEC_RTOL, GRAD_RTOL through tests/gradcheck.assert_grad_close with
   its fp32 conditioning callback; `check_parity` of tests/test_causal_gpu.py, restated), on every case and route, on the
   de-duplicated step, with the three polynomial terms, and again after the state has moved.
2. Single update: lambda', slots', omega', Z' and the statistics after a step against tests/adapt_ref.py in fp64 on the engine's
   own state and loss field before it, at the bar tests/adapt_cases.single_update_bar measures (never read from the engine).
3. Bitwise contracts, 4. non-mutation by the loss-only calls and probes, 5. a zero loss field, 6. alignment, 7. refusals and
   replacement, 8. the `VarNet` layer.  Also under 1: a hard-constraint ansatz on one case (tests/ansatz_cases.py).

The figures are written to adapt_parity.json in the directory VN_RECORD_DIR names (default: profile_out/ beside tests/; the
committed copy: profiles/adapt_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import adapt_ref, causal_ref, dedup_map_cases as mc, nldiff_cases, nlflux_cases
from tests.adapt_cases import (BASE, CASES, IDS, RULES, SINGLE_CASES, inputs, lambda0, omega0, parity_spec, reference, rel_dev,
                               single_update_bar, spec_of, theta, weights_are_real)
from tests.gradcheck import assert_grad_close, block_errors
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL
from varnet_amd.engine import VN_KERNEL_AUTO, VN_KERNEL_FUSED, VN_KERNEL_GENERIC, VNEngine, VNError

pytestmark = pytest.mark.gpu

KEYS = ['loss', 'BCloss', 'ICloss', 'varLoss']
RECORD = {}
KNAME = {VN_KERNEL_AUTO: 'auto', VN_KERNEL_GENERIC: 'generic'}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        RECORD['single_update_bar'] = {r: single_update_bar(r) for r in RULES}
        with open(os.path.join(out, 'adapt_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def register_interior(eng, i, batch=0):
    d = inputs(i)
    eng.set_interior(batch, d['Input'], d['gcoef'], d['source'], n_k=CASES[i][4], detJ=d['detJ'], N_rows=d['N_rows'],
                     dNt_rows=d['dNt_rows'])


def register_terms(eng, i, batch=0):
    (phi, fcoef), (rate, coef) = nlflux_cases.terms_of(i, 'both')
    eng.set_reaction(batch, rate, coef)
    eng.set_nlflux(batch, phi, fcoef)
    eng.set_nldiff(batch, nldiff_cases.psi(i), nldiff_cases.DIFF)


def make_engine(i, kernel=VN_KERNEL_AUTO, spec=None, variant='plain', xcheck=False, optimizer='adam', lam=True):
    """An engine of CASES[i]; spec: the adaptive registration of batch 0 (None: none), started from lambda0(i) (lam=False: from
    the spec's init)."""
    d_in, dim, widths, q, n_k, nB, bDof, td, act, source, integW, detJvec, rows = CASES[i]
    d = inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW, kernel=kernel, activationFun=act, xcheck=xcheck,
                   optimizer_name=optimizer)
    eng.set_params(theta(i))
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    register_interior(eng, i)
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
    eng.set_weights(d['w'])
    if variant == 'terms':
        register_terms(eng, i)
    if spec is not None:
        eng.set_tf_adapt(0, spec, lambda0(i) if lam else None)
    return eng


def grad_of(eng, batch=0):
    gb = eng.bind_grad_buffer()
    eng.grad(batch)
    torch.cuda.synchronize()
    return gb.cpu().numpy().astype(np.float64)


def state_of(eng, batch=0):
    """The committed state as a list of arrays, for bitwise comparison."""
    s = eng.tf_adapt(batch)
    st = s['stats']
    out = [s['lambda'], s['omega'], np.array([st[k] for k in ('min', 'max', 'mean', 'share', 'Z', 'tau')])]
    if s['slots'] is not None:
        out.append(s['slots'])
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def outside_generic(i, kernel):
    """The 128-wide case lies outside the generic kernels: the engine refuses the request (as it does without weights)."""
    if max(CASES[i][2]) > 64 and kernel == VN_KERNEL_GENERIC:
        with pytest.raises(VNError, match='error 5'):
            make_engine(i, kernel)
        return True
    return False


def check_parity(net, eng, ref, tag, g32):
    """eval_loss (with the unweighted lossVec) and grad of batch 0 against ref = (result, gradient); prints and records every
    figure, then asserts.  net = (d_in, dim, widths, td)."""
    d_in, dim, widths, td = net
    ref, gref = ref
    out, lv = eng.eval_loss(0, lossVec=True)
    g = grad_of(eng)
    P = eng.P
    rel = lambda got, want: abs(got - want) / max(abs(want), 1e-300) if want != 0.0 else abs(got)
    rec = {'eval_' + k: rel(got, ref[k]) for got, k in zip(out, KEYS)}
    rec.update({'grad_' + k: rel(got, ref[k]) for got, k in zip(g[P:], KEYS)})
    lref = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1)
    rec['lossVec'] = float(np.max(np.abs(lv.cpu().numpy() - lref)) / np.max(np.abs(lref)))
    errs = block_errors(g, gref, d_in, widths, dim, td)
    rec['worst_block'] = max(errs, key=errs.get)
    rec['worst_block_err'] = errs[rec['worst_block']]
    rec['kernel_path'] = list(eng.kernel_path())
    RECORD[tag] = rec
    print('adapt %s: %s' % (tag, json.dumps(rec, sort_keys=True)))
    for got, key in zip(out, KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'eval', key, got, ref[key])
    for got, key in zip(g[P:], KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'grad', key, got, ref[key])
    assert rec['lossVec'] <= LVEC_RTOL, (tag, rec['lossVec'])             # lossVec is the UNWEIGHTED field of the reference
    assert_grad_close(g[:P], gref, d_in, widths, GRAD_RTOL, dim=dim, td=td, what=tag, g32=g32)
    return g


def net_of(i):
    return CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][7]


def check_in_use(i, eng, tag, variant='plain'):
    """The reference evaluated at the engine's parameters with the engine's own committed omega as static weights."""
    om = eng.tf_adapt(0)['omega'].astype(np.float64)
    flat = eng.get_params()
    return check_parity(net_of(i), eng, reference(i, om, variant, flat), tag,
                        lambda: reference(i, om, variant, flat, dtype=torch.float32)[1])


# ---- 1. weights in use -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_weights_in_use_parity(i, kernel):
    weights_are_real(i)
    if outside_generic(i, kernel):
        return
    eng = make_engine(i, kernel, parity_spec('rba'))
    try:
        s = eng.tf_adapt(0)
        assert np.array_equal(s['lambda'], lambda0(i)) and s['stats']['tau'] == 0.0 and s['stats']['Z'] == 1.0
        assert rel_dev(s['omega'], omega0(i)) <= 2.0 ** -23               # lambda^2 in fp32, one rounding more to omega
        g1 = check_in_use(i, eng, '%s/%s' % (IDS[i], KNAME[kernel]))
        assert np.array_equal(g1, grad_of(eng))                           # two calls: the same bits
    finally:
        eng.close()


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('i', [1, 3], ids=[IDS[1], IDS[3]])
def test_weights_in_use_after_the_state_has_moved(i, rule):
    """Three steps at a large rate, then the same comparison: the weights in use are those of the committed state."""
    kw = dict(eta=0.5, gamma=0.9) if rule == 'rba' else dict(lr=0.1)
    eng = make_engine(i, spec=parity_spec(rule, **kw))
    try:
        om0 = eng.tf_adapt(0)['omega']
        for _ in range(3):
            eng.train_step(0)
        s = eng.tf_adapt(0)
        assert s['stats']['tau'] == 3.0 and rel_dev(s['omega'], om0) > 1e-2
        check_in_use(i, eng, '%s/%s/moved' % (IDS[i], rule))
    finally:
        eng.close()


def test_weights_in_use_with_all_three_terms():
    i = 3
    weights_are_real(i, 'terms')
    eng = make_engine(i, spec=parity_spec('rba'), variant='terms')
    try:
        check_in_use(i, eng, '%s/auto/terms' % IDS[i], 'terms')
    finally:
        eng.close()


def test_weights_in_use_with_an_ansatz():
    """Case 2 of tests/ansatz_cases.py (5x50 net, n_k = 257: two seed blocks) with its ansatz on the interior and the BC/IC rows.
    The reference is tests/ansatz_ref.py with the weights carried by its per-test-function detJ (detJ omega_k: the same sum);
    its loss field divided by omega is the unweighted one."""
    from tests import ansatz_cases as az, ansatz_ref
    from tests.test_ansatz_gpu import make_engine as ansatz_engine
    i = 2
    n_k = az.CASES[i][4]
    net = (az.CASES[i][0], az.CASES[i][1], az.CASES[i][2], az.CASES[i][7])
    lam = np.random.default_rng(31).uniform(0.5, 2.0, n_k).astype(np.float32)
    eng = ansatz_engine(i)
    try:
        eng.set_tf_adapt(0, parity_spec('rba'), lam)
        om = eng.tf_adapt(0)['omega'].astype(np.float64)
        detJ = float(az.inputs(i)['detJ'])

        def ev(dtype, omega):
            f = np.float64 if dtype == torch.float64 else np.float32
            if omega is None:
                return az.reference(i, dtype=dtype)
            kw = az.ref_kw(i, dtype)
            kw['detJ'], kw['detJvec'] = (detJ * omega).reshape(-1, 1).astype(f), True
            ref, g = ansatz_ref.loss_and_grad(az.theta(i).astype(f), net[0], net[2], az.cast(az.ansatz(i), f), dtype=dtype, **kw)
            ref['lossVec'] = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1) / omega
            return ref, g
        ref, gref = ev(torch.float64, om)
        ref0, g0 = ev(torch.float64, None)
        assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss'])
        assert np.linalg.norm(gref - g0) > 1e-2 * np.linalg.norm(gref)
        assert rel_dev(ref['lossVec'], np.asarray(ref0['lossVec']).reshape(-1)) <= 1e-12
        check_parity(net, eng, (ref, gref), 'ansatz/%s' % az.IDS[i], lambda: ev(torch.float32, om)[1])
        eng.train_step(0)
        assert eng.tf_adapt(0, arrays=False)['stats']['tau'] == 1.0
    finally:
        eng.close()


def test_weights_in_use_dedup_identity_map():
    i = 3
    eng = make_engine(i, spec=parity_spec('sa'))
    try:
        g_row = grad_of(eng)
        nT = inputs(i)['Input'].shape[0]
        idx = torch.arange(nT, dtype=torch.int32)
        eng.set_dedup(0, inputs(i)['Input'], idx, torch.arange(nT + 1, dtype=torch.int32), idx)        # keeps the registration
        g1 = check_in_use(i, eng, '%s/dedup_identity' % IDS[i])
        assert np.array_equal(g1, grad_of(eng)) and not np.array_equal(g1, g_row)                    # another formulation ran
        eng.train_step(0)                                                 # ... whose step moves the state, too
        assert eng.tf_adapt(0, arrays=False)['stats']['tau'] == 1.0
        check_in_use(i, eng, '%s/dedup_identity/moved' % IDS[i])
    finally:
        eng.close()


def test_weights_in_use_dedup_shared_point_map():
    """The 'hot_point' map of tests/dedup_map_cases.py (7680 rows on 300 points, n_k = 120: four 32-function partials)."""
    name = 'hot_point'
    d_in, dim, widths, q, act, source, integW = mc.config(name)[:7]
    d = mc.inputs(name)
    n_k = d['n_k']
    lam = np.random.default_rng(31).uniform(0.5, 2.0, n_k).astype(np.float32)
    eng = VNEngine(dim, d_in, widths, True, q, isSource=source, integWflag=integW, activationFun=act)
    try:
        eng.set_params(mc.theta(name))
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        eng.set_bic(d['biInput'], d['biLabel'], d['bDof'], mc.BIDIMVAL)
        eng.set_weights(d['w'])
        eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=mc.DETJ)
        eng.set_dedup(0, d['Xu'], d['uid'], d['rowptr'], d['rowidx'])
        eng.set_tf_adapt(0, parity_spec('rba'), lam)
        om = eng.tf_adapt(0)['omega'].astype(np.float64)
        ev = lambda dt, f, o: causal_ref.loss_and_grad(mc.theta(name).astype(f), d_in, widths, o, None, dtype=dt, **mc.ref_kw(name, dt))
        ref, gref = ev(torch.float64, np.float64, om)
        ref0, g0 = ev(torch.float64, np.float64, None)
        assert abs(ref['varLoss'] - ref0['varLoss']) > 1e-2 * abs(ref['varLoss'])
        assert np.linalg.norm(gref - g0) > 1e-2 * np.linalg.norm(gref)
        check_parity((d_in, dim, widths, True), eng, (ref, gref), 'dedup_map/%s' % name, lambda: ev(torch.float32, np.float32, om)[1])
        eng.train_step(0)
        assert eng.tf_adapt(0, arrays=False)['stats']['tau'] == 1.0
    finally:
        eng.close()


# ---- 2. single update ------------------------------------------------------------------------------------------------
def predict_and_compare(i, eng, spec, bar, tag, rec):
    """One train_step of batch 0: the state and the loss field before it, the fp64 prediction, the comparison.
    The field is that of a vn_eval_loss at the same parameters, NOT the one the step's own vn_grad wrote: the engine-owned
    buffer of a gradient evaluation has no entry point that reads it back, and the loss-only call runs other kernels on some
    routes (the forward-only launch or the de-duplicated loss-only sequence), so the two fields need not agree bit for bit.
    What the comparison can still tell: lambda' and omega' see a deviation delta of l_k damped (eta delta / 2 for rba, the
    rate for sa), but the sa slots do not -- m1 moves by (1 - beta1) delta relative, m2 by twice that -- and they are compared
    at the same bar, so on the sa runs the two fields agree to a few ulps or the slots would miss it."""
    before = eng.tf_adapt(0)
    _, lv = eng.eval_loss(0, lossVec=True)
    want = adapt_ref.step(before['lambda'].astype(np.float64), None if before['slots'] is None else before['slots'].astype(np.float64),
                          int(before['stats']['tau']), lv.cpu().numpy().astype(np.float64), spec)
    eng.train_step(0)
    after = eng.tf_adapt(0)
    dev = {'lambda': rel_dev(after['lambda'], want['lam']), 'omega': rel_dev(after['omega'], want['omega']),
           'slots': 0.0 if want['slots'] is None else rel_dev(after['slots'], want['slots']),
           'stats': max(rel_dev(after['stats'][k], want['stats'][k]) for k in ('min', 'max', 'mean', 'share', 'Z'))}
    for k, v in dev.items():
        rec[k] = max(rec.get(k, 0.0), v)
    assert after['stats']['tau'] == want['stats']['tau'], (tag, after['stats'], want['stats'])
    assert max(dev.values()) <= bar, (tag, dev, bar)
    return before, after


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('i', SINGLE_CASES, ids=[IDS[k] for k in SINGLE_CASES])
def test_single_update_chained_over_eight_steps(i, rule):
    bar = single_update_bar(rule)['bar']
    spec = spec_of(i, rule)
    eng = make_engine(i, spec=spec)
    rec = {'bar': bar}
    tag = '%s/%s/single_update' % (IDS[i], rule)
    try:
        for s in range(8):
            before, after = predict_and_compare(i, eng, spec, bar, tag, rec)
            assert after['stats']['tau'] == s + 1
            assert not np.array_equal(after['lambda'], before['lambda'])
    finally:
        RECORD[tag] = rec
        print('adapt %s: %s' % (tag, json.dumps(rec, sort_keys=True)))
        eng.close()


@pytest.mark.parametrize('rule', RULES)
def test_every_three_updates_on_every_third_step(rule):
    i = 1
    spec = spec_of(i, rule, every=3)
    bar = single_update_bar(rule)['bar']
    eng = make_engine(i, spec=spec)
    static = make_engine(i)
    try:
        taus = []
        for s in range(8):
            if s % 3 == 0:
                predict_and_compare(i, eng, spec, bar, 'every3', {})
            else:                                                         # a static-weights step: the state stays, bit for bit
                st = state_of(eng)
                static.set_params(eng.get_params())
                static.set_tf_weights(0, eng.tf_adapt(0)['omega'])
                g = grad_of(static)
                assert np.array_equal(grad_of(eng), g)
                eng.apply()
                assert same(state_of(eng), st)
            taus.append(eng.tf_adapt(0, arrays=False)['stats']['tau'])
        assert taus == [1, 1, 1, 2, 2, 2, 3, 3]
    finally:
        eng.close()
        static.close()


# ---- 3. bitwise contracts ----------------------------------------------------------------------------------------------
BITWISE = [(3, 'rba'), (3, 'sa'), (BASE + 2, 'sa'), (1, 'rba')]
BITWISE_IDS = ['%s-%s' % (IDS[i], r) for i, r in BITWISE]


def run_steps(eng, n, batch=0):
    for _ in range(n):
        eng.train_step(batch)
    torch.cuda.synchronize()
    return [eng.get_params()] + state_of(eng)


@pytest.mark.parametrize('i,rule', BITWISE, ids=BITWISE_IDS)
def test_two_engines_and_step_is_grad_plus_apply(i, rule):
    """Two engines on the same sequence give the same bits.  train_step against grad + apply: the two forms of the optimizer step
    (folded into the reduction, or a kernel of its own) differ in theta by an ulp here and there without any weights
    (tests/test_periodic_gpu.py measures that gap), so the contract is pinned where it can hold bit for bit: from one exported
    state, both forms leave the SAME adaptive state, and each leaves the theta its own form leaves on a static registration of
    the committed omega."""
    a, b, c = (make_engine(i, spec=spec_of(i, rule)) for _ in range(3))
    s1, s2 = make_engine(i), make_engine(i)
    try:
        ra = run_steps(a, 4)
        assert same(ra, run_steps(b, 4))                                  # two engines, the same sequence: the same bits
        assert a.step == 4 and ra[3][5] == 4.0
        plain_bytes = s1.export_state().size
        for _ in range(3):
            buf = a.export_state()
            om = a.tf_adapt(0)['omega']
            c.import_state(buf)
            for twin in (s1, s2):
                twin.import_state(buf[:plain_bytes])                      # step, theta and both slots: the prefix of the layout
                twin.set_tf_weights(0, om)
            a.train_step(0)
            s1.train_step(0)
            for e in (c, s2):
                e.grad(0)
                e.apply()
            torch.cuda.synchronize()
            assert same(state_of(a), state_of(c))                         # one pending state, committed by either form
            assert np.array_equal(a.get_params(), s1.get_params())        # the folded step: that of static weights
            assert np.array_equal(c.get_params(), s2.get_params())        # grad + apply: likewise
            assert a.step == c.step == s1.step
    finally:
        for e in (a, b, c, s1, s2):
            e.close()


@pytest.mark.parametrize('i,rule', BITWISE[:2], ids=BITWISE_IDS[:2])
def test_grad_twice_without_apply(i, rule):
    eng, once = make_engine(i, spec=spec_of(i, rule)), make_engine(i, spec=spec_of(i, rule))
    try:
        st = state_of(eng)
        g1 = grad_of(eng).copy()
        assert same(state_of(eng), st)                                    # a pending state is not the committed one
        g2 = grad_of(eng).copy()
        assert np.array_equal(g1, g2) and same(state_of(eng), st)
        eng.apply()
        once.grad(0)
        once.apply()
        torch.cuda.synchronize()
        assert same([eng.get_params()] + state_of(eng), [once.get_params()] + state_of(once))      # the same pending bits
        assert eng.tf_adapt(0, arrays=False)['stats']['tau'] == 1.0
    finally:
        eng.close()
        once.close()


@pytest.mark.parametrize('rule', RULES)
def test_train_epoch_over_two_batches_one_adaptive(rule):
    i = 3
    a, b = make_engine(i, spec=spec_of(i, rule)), make_engine(i, spec=spec_of(i, rule))
    plain = make_engine(i)
    try:
        for e in (a, b):
            register_interior(e, i, batch=1)                              # batch 1: the same rows, no registration
        assert np.array_equal(grad_of(a, 1), grad_of(plain))              # ... bit for bit the step of a plain engine
        a.apply()
        b.grad(1)
        b.apply()
        acc = torch.zeros(1, device='cuda')
        a.train_epoch((0, 1, 0), acc)
        for k in (0, 1, 0):
            b.train_step(k)
        torch.cuda.synchronize()
        assert same([a.get_params()] + state_of(a), [b.get_params()] + state_of(b))
        assert a.step == 4 and a.tf_adapt(0, arrays=False)['stats']['tau'] == 2.0
        assert np.isfinite(acc.item())
    finally:
        for e in (a, b, plain):
            e.close()


@pytest.mark.parametrize('i,rule', BITWISE[:3], ids=BITWISE_IDS[:3])
def test_snapshot_rollback_replay_and_export_import(i, rule):
    spec = spec_of(i, rule)
    eng, fresh = make_engine(i, spec=spec), make_engine(i, spec=spec, lam=False)
    plain = make_engine(i)
    try:
        assert eng.export_state().size > plain.export_state().size         # the state travels
        run_steps(eng, 2)
        eng.state_snapshot()
        s2 = state_of(eng)
        r5 = run_steps(eng, 5)
        eng.state_rollback()
        assert same(state_of(eng), s2) and eng.step == 2
        assert same(run_steps(eng, 5), r5)                                # replay: the same bits
        buf = eng.export_state()
        fresh.import_state(buf)
        assert same(state_of(fresh), state_of(eng)) and fresh.step == eng.step
        assert same(run_steps(fresh, 3), run_steps(eng, 3))
        # vn_set_tf_adapt_state: lambda, slots and tau put back, omega and the statistics rebuilt to the same bits
        s = eng.tf_adapt(0)
        fresh.set_tf_adapt_state(0, np.ones_like(s['lambda']), None, 0)
        assert not same(state_of(fresh), state_of(eng))
        fresh.set_tf_adapt_state(0, s['lambda'], s['slots'], int(s['stats']['tau']))
        assert same(state_of(fresh), state_of(eng))
        # vn_params_init returns to the registered initial state
        eng.init_params(seed=1)
        s0 = eng.tf_adapt(0)
        assert np.array_equal(s0['lambda'], lambda0(i)) and s0['stats']['tau'] == 0.0
        assert s0['slots'] is None or not s0['slots'].any()
    finally:
        for e in (eng, fresh, plain):
            e.close()


def _snapshot(eng):
    out, lv = eng.eval_loss(0, lossVec=True)
    g = grad_of(eng).copy()
    for _ in range(3):
        eng.train_step(0)
    torch.cuda.synchronize()
    return [np.array(out), lv.cpu().numpy(), g, eng.get_params(), eng.export_state()]


@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('i', [2, 3], ids=[IDS[2], IDS[3]])
def test_register_then_clear_is_bitwise_untouched(i, kernel):
    """Loss, loss field, gradient, three steps and the exported state (vn_state_size with it) of an engine that registered and
    cleared, or registered and re-registered its interior, against one that never registered."""
    def run(how):
        eng = make_engine(i, kernel, None if how == 'never' else spec_of(i, 'sa'))
        try:
            if how != 'never':
                eng.grad(0)                                               # an evaluation with the weights, a pending state ...
                if how == 'cleared':
                    eng.set_tf_adapt(0)                                   # ... then cleared
                else:
                    register_interior(eng, i)                             # a new vn_set_interior clears the registration
            return _snapshot(eng)
        finally:
            eng.close()
    never = run('never')
    for how in ('cleared', 'reregistered'):
        assert same(never, run(how)), how


@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
def test_identity_rule_is_a_static_registration_of_ones(kernel):
    """rba with gamma = 1, eta = 0, init = 1, normalize = False: omega = 1 bit for bit, over three steps."""
    i = 1
    eng = make_engine(i, kernel, adapt_ref.spec_of('rba', gamma=1.0, eta=0.0, init=1.0, normalize=False), lam=False)
    static = make_engine(i, kernel)
    try:
        static.set_tf_weights(0, np.ones(CASES[i][4], dtype=np.float32))
        assert np.array_equal(grad_of(eng), grad_of(static))
        for e in (eng, static):
            for _ in range(3):
                e.train_step(0)
        torch.cuda.synchronize()
        assert np.array_equal(eng.get_params(), static.get_params())
        s = eng.tf_adapt(0)
        assert np.all(s['omega'] == 1.0) and np.all(s['lambda'] == 1.0) and s['stats']['tau'] == 3.0
    finally:
        eng.close()
        static.close()


# ---- 4. non-mutation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rule', RULES)
def test_loss_only_calls_and_probes_leave_the_state_alone(rule):
    i = 1
    spec = spec_of(i, rule)
    eng, quiet = make_engine(i, spec=spec), make_engine(i, spec=spec)
    try:
        for e in (eng, quiet):
            e.train_step(0)
        eng.grad(0)                                                       # a pending state, which the calls below must keep as well
        quiet.grad(0)
        st = state_of(eng)
        out, _ = eng.eval_loss(0, lossVec=True)
        assert same(state_of(eng), st)
        o64, g64, lv64 = eng.objective64(0, grad=True, lossVec=True)      # parity at its own bar with omega widened
        om = eng.tf_adapt(0)['omega'].astype(np.float64)
        ref, gref = reference(i, om, flat=eng.get_params())
        for got, key in zip(o64, KEYS):
            assert abs(got - ref[key]) <= 1e-12 * abs(ref[key]) + 1e-300, (key, got, ref[key])
        d_in, dim, widths, td = net_of(i)
        errs = block_errors(g64.cpu().numpy(), gref, d_in, widths, dim, td)
        assert max(errs.values()) <= 1e-11, errs
        assert same(state_of(eng), st)
        tg = eng.term_grads([0])                                          # what a balance probe runs
        assert np.all(np.isfinite(tg['norm2']))
        assert same(state_of(eng), st)
        eng.grad(0)                                                       # (a probe leaves its own sums in the gradient buffer)
        eng.apply()                                                       # commits the pending state: one update, not two
        quiet.apply()
        torch.cuda.synchronize()
        assert same([eng.get_params()] + state_of(eng), [quiet.get_params()] + state_of(quiet))
        # between two steps, with nothing pending
        eng.eval_loss(0)
        eng.term_grads([0])
        assert same(run_steps(eng, 1), run_steps(quiet, 1))
    finally:
        eng.close()
        quiet.close()


# ---- 5. zero field -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rule', RULES)
def test_zero_loss_field_does_not_move_the_state(rule):
    """theta = 0 on a source-free case: u = 0, every residual and l_k vanish (the BC / IC terms do not)."""
    i = 1
    spec = spec_of(i, rule)
    eng, static = make_engine(i, spec=spec), make_engine(i)
    try:
        zero = np.zeros(eng.P, dtype=np.float32)
        eng.set_params(zero)
        static.set_params(zero)
        out, lv = eng.eval_loss(0, lossVec=True)
        assert not lv.cpu().numpy().any() and out[0] > 0.0
        st = state_of(eng)
        static.set_tf_weights(0, eng.tf_adapt(0)['omega'])
        eng.train_step(0)
        static.train_step(0)
        torch.cuda.synchronize()
        s = eng.tf_adapt(0)
        assert same(state_of(eng), st) and s['stats']['tau'] == 0.0 and np.all(np.isfinite(s['omega']))
        assert np.array_equal(eng.get_params(), static.get_params()) and eng.get_params().any()
    finally:
        eng.close()
        static.close()


# ---- 6. alignment ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rule', RULES)
def test_views_off_the_16_byte_grid(rule):
    """Case 1 cut to 39 test functions (n_k % 4 = 3): lambda_init_dev one float off the 16-byte grid (validated and copied by
    a one-entry-per-thread kernel); the update's own accesses, all on engine-owned aligned buffers -- the loss field of a
    gradient evaluation included, vn_grad takes no caller's array --, end in a scalar tail."""
    i, n_k = 1, 39
    d_in, dim, widths, q, _, nB, bDof, td, act, source, integW, detJvec, rows = CASES[i]
    d = {k: (v[:n_k * q] if k in ('Input', 'gcoef') else v) for k, v in inputs(i).items()}
    spec = adapt_ref.spec_of(rule)
    lam = lambda0(i)[:n_k]
    eng = VNEngine(dim, d_in, widths, td, q, activationFun=act)
    try:
        eng.set_params(theta(i))
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=n_k, detJ=d['detJ'])
        eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
        eng.set_weights(d['w'])
        buf = torch.zeros(n_k + 5, dtype=torch.float32, device='cuda')
        view = buf[1:1 + n_k]
        view.copy_(torch.as_tensor(lam))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
        eng.set_tf_adapt(0, spec, view)
        buf.zero_()                                                       # copied by the call
        s = eng.tf_adapt(0)
        assert np.array_equal(s['lambda'], lam)
        want = adapt_ref.weights(lam, spec, dtype=np.float32)             # m = lambda^2 in fp32, sums in fp64, as in the kernel
        assert rel_dev(s['omega'], want[0]) <= 2.0 ** -23 and rel_dev(s['stats']['Z'], want[1]) <= 1e-13
        predict_and_compare(i, eng, spec, single_update_bar(rule)['bar'], 'misaligned_39/%s' % rule, {})
    finally:
        eng.close()


# ---- 7. refusals and replacement -----------------------------------------------------------------------------------------
def test_refusals():
    i = 2
    eng = make_engine(i, VN_KERNEL_FUSED, xcheck=True)                    # the 4-wave cross-check geometry
    try:
        with pytest.raises(VNError, match='error 5: vn_set_tf_adapt is not built for VN_KERNEL_FUSED'):
            eng.set_tf_adapt(0, 'rba')
        eng.set_tf_adapt(0)                                               # clearing is always accepted
    finally:
        eng.close()
    eng = make_engine(i)
    plain = make_engine(i)
    try:
        import ctypes as C
        raw = lambda rule, par, lam=None, batch=0: eng._ck(eng.lib.vn_set_tf_adapt(eng.h, batch, rule, (C.c_double * 10)(*par), lam))
        rba = [0.999, 0.01, 0, 0, 0, 2, 1, 1, 1, 0]
        sa = [0.005, 1e3, 0.9, 0.999, 1e-8, 2, 1, 1, 1, 0]
        bad = [(1, 0, -0.1), (1, 0, 1.5), (1, 1, -1.0), (1, 5, 3.0), (1, 5, 0.0), (1, 8, 0.0), (1, 8, 1.5), (1, 7, 2.0), (1, 6, -1.0),
               (1, 0, float('nan')), (1, 9, float('inf')),
               (2, 0, -1.0), (2, 1, 0.0), (2, 2, 1.0), (2, 2, -0.1), (2, 3, 1.0), (2, 4, 0.0), (2, 5, 0.0), (2, 8, 0.5), (2, 4, float('nan'))]
        for rule, k, v in bad:
            par = list(rba if rule == 1 else sa)
            par[k] = v
            with pytest.raises(VNError, match='error 1: vn_set_tf_adapt'):
                raw(rule, par)
        with pytest.raises(VNError, match='error 1: vn_set_tf_adapt: rule'):
            raw(3, rba)
        n_k = CASES[i][4]
        for v in (-1.0, float('nan'), float('inf')):                      # lambda_init_dev is validated on the device
            lam = torch.ones(n_k, device='cuda')
            lam[n_k // 2] = v
            with pytest.raises(VNError, match=r'error 1: vn_set_tf_adapt: 1 initial lambda\(s\)'):
                eng.set_tf_adapt(0, 'rba', lam)
        with pytest.raises(AssertionError, match='one entry per test function'):
            eng.set_tf_adapt(0, 'rba', np.ones(n_k - 1, dtype=np.float32))
        with pytest.raises(VNError, match='error 3'):
            eng.set_tf_adapt(5, 'rba')                                    # an unregistered batch
        with pytest.raises(VNError, match='error 3: vn_get_tf_adapt: batch 0 has no adaptive registration'):
            eng.tf_adapt(0)
        with pytest.raises(VNError, match='error 3: vn_set_tf_adapt_state: batch 0 has no adaptive registration'):
            eng.set_tf_adapt_state(0, np.ones(n_k, dtype=np.float32))
        d_in, dim = CASES[i][0], CASES[i][1]
        eng.set_interior(1, torch.zeros(0, d_in, device='cuda'), torch.zeros(0, dim, device='cuda'), None, n_k=0, detJ=0.1)
        with pytest.raises(VNError, match='error 1: batch 1 has no interior rows'):
            raw(1, rba, batch=1)
        # none of the refused calls left a registration behind
        assert np.array_equal(grad_of(eng), grad_of(plain))
        assert eng.export_state().size == plain.export_state().size
        # state calls on a registered batch
        eng.set_tf_adapt(0, 'rba')
        with pytest.raises(VNError, match='error 1: vn_set_tf_adapt_state: lambda'):
            eng.set_tf_adapt_state(0, np.full(n_k, -1.0, dtype=np.float32))
        with pytest.raises(VNError, match='error 1: vn_set_tf_adapt_state: tau'):
            eng.set_tf_adapt_state(0, np.ones(n_k, dtype=np.float32), None, -1)
        with pytest.raises(VNError, match='error 1: vn_set_tf_adapt_state: batch 0 runs the rba rule'):
            eng.set_tf_adapt_state(0, np.ones(n_k, dtype=np.float32), np.zeros((2, n_k), dtype=np.float32))
        lam_h, slots_h = np.full(n_k, -7.0, np.float32), np.zeros(2 * n_k, np.float32)
        with pytest.raises(VNError, match='error 1: vn_get_tf_adapt: batch 0 runs the rba rule'):
            eng._ck(eng.lib.vn_get_tf_adapt(eng.h, 0, lam_h.ctypes.data, None, slots_h.ctypes.data, None))
        torch.cuda.synchronize()
        assert np.all(lam_h == -7.0)                                      # refused before any copy was enqueued
        st = (C.c_double * 6)()
        eng._ck(eng.lib.vn_get_tf_adapt(eng.h, 0, None, None, None, st))  # stats alone
        assert list(st)[2] == 1.0 and list(st)[5] == 0.0
    finally:
        eng.close()
        plain.close()


def test_registrations_replace_each_other():
    from tests.causal_cases import n_slabs, slabs, static_weights
    i = 3
    spec = spec_of(i, 'rba')
    eng, ref_a, ref_s = make_engine(i, spec=spec), make_engine(i, spec=spec), make_engine(i)
    try:
        ref_s.set_tf_weights(0, static_weights(i))
        g_a, g_s = grad_of(ref_a).copy(), grad_of(ref_s).copy()
        assert not np.array_equal(g_a, g_s)
        assert np.array_equal(grad_of(eng), g_a)
        eng.set_tf_weights(0, static_weights(i))                          # replaces the adaptive registration ...
        assert np.array_equal(grad_of(eng), g_s)
        with pytest.raises(VNError, match='error 3'):
            eng.tf_adapt(0)
        eng.set_tf_adapt(0, spec, lambda0(i))                             # ... and back
        assert np.array_equal(grad_of(eng), g_a)
        eng.set_causal(0, slabs(i), n_slabs(i), 1.0)                      # a causal registration replaces it as well
        with pytest.raises(VNError, match='error 3'):
            eng.tf_adapt(0)
        eng.set_tf_adapt(0, spec, lambda0(i))
        with pytest.raises(VNError, match='error 3: batch 0 has no causal registration'):
            eng.causal_weights(0)
        assert np.array_equal(grad_of(eng), g_a)
    finally:
        for e in (eng, ref_a, ref_s):
            e.close()


def test_lbfgs_refuses_an_adaptive_batch():
    i = 2
    eng = make_engine(i, spec=spec_of(i, 'rba'), optimizer='lbfgs')
    try:
        with pytest.raises(VNError, match='error 5: vn_lbfgs_step on batch 0, which has an adaptive registration'):
            eng.lbfgs_step(0)
        eng.set_tf_adapt(0)
        assert eng.lbfgs_step(0)['status'] == 0
    finally:
        eng.close()


def test_comm_init_is_refused_on_a_handle_with_an_adaptive_batch():
    """vn_comm_init checks the batches before it touches the collective library: the refusal needs none."""
    from varnet_amd.engine import VN_COMM_ID_BYTES
    i = 2
    spec = spec_of(i, 'rba')
    eng, ref = make_engine(i, spec=spec), make_engine(i, spec=spec)
    try:
        with pytest.raises(VNError, match='error 5: vn_comm_init: batch 0 has an adaptive registration'):
            eng.comm_init(0, 1, bytes(VN_COMM_ID_BYTES))
        assert same(run_steps(eng, 2), run_steps(ref, 2))                 # the registration is still there and in use
        eng.set_tf_adapt(0)
        assert eng.export_state().size < ref.export_state().size
    finally:
        eng.close()
        ref.close()


def test_set_tf_adapt_is_refused_under_a_communicator():
    """A one-rank communicator on this card, then the registration: error 5; clearing (rule 0) is still accepted; after
    vn_comm_destroy the registration goes through."""
    assert VNEngine.comm_available(), 'the one-rank communicator of tests/test_multi_gpu.py needs the collective library'
    i = 2
    eng = make_engine(i)
    try:
        eng.comm_init(0, 1, VNEngine.comm_unique_id())
        assert eng.comm_size() == (1, 0)
        for rule in RULES:
            with pytest.raises(VNError, match='error 5: vn_set_tf_adapt under a communicator'):
                eng.set_tf_adapt(0, rule)
        eng.set_tf_adapt(0)                                               # rule 0 is always accepted
        with pytest.raises(VNError, match='error 3'):
            eng.tf_adapt(0)                                               # nothing was registered
        eng.comm_destroy()
        eng.set_tf_adapt(0, 'rba')
        assert eng.tf_adapt(0, arrays=False)['stats']['tau'] == 0.0
    finally:
        eng.close()


@pytest.mark.parametrize('rule', RULES)
def test_rmsprop_commits_through_the_same_path(rule):
    """RMSProp is not refused: its folded step and its vn_apply commit the pending state like Adam's.  Three steps of each form
    against the fp64 prediction, tau counting every one."""
    i = 1
    spec = spec_of(i, rule)
    bar = single_update_bar(rule)['bar']
    eng, sep = make_engine(i, spec=spec, optimizer='rmsprop'), make_engine(i, spec=spec, optimizer='rmsprop')
    try:
        for s in range(3):
            predict_and_compare(i, eng, spec, bar, 'rmsprop/%s' % rule, {})
        before = state_of(sep)
        sep.grad(0)
        assert same(state_of(sep), before)                                # pending until the optimizer step
        sep.apply()
        assert sep.tf_adapt(0, arrays=False)['stats']['tau'] == 1.0 and not same(state_of(sep), before)
        assert eng.tf_adapt(0, arrays=False)['stats']['tau'] == 3.0 and eng.step == 3 and sep.step == 1
    finally:
        eng.close()
        sep.close()


@pytest.mark.parametrize('rule', RULES)
def test_beyond_the_block_cap_every_thread_strides(rule):
    """n_k = 263 173: 258 spans of 1024 on the 256-block cap of the three kernels, so the first blocks' threads run a second
    strided pass (the last one partial, n_k % 4 = 1).  Two updates against the fp64 prediction, elementwise, at the measured
    bar; the (1, 1, [20], q = 4) net of case 0 on synth's inputs."""
    from tests.parity_cases import synth
    n_k = 256 * 1024 + 1029
    assert n_k % 4 == 1 and n_k > 256 * 1024
    d_in, dim, widths, q, _, nB, bDof, td, act = CASES[0][:9]
    d = synth(11, d_in, dim, widths, q, n_k, nB, bDof)
    spec = adapt_ref.spec_of(rule)
    eng = VNEngine(dim, d_in, widths, td, q, activationFun=act)
    try:
        eng.set_params(theta(0))
        eng.set_fe_table(d['N1'], d['dNt1'], None)
        eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=n_k, detJ=d['detJ'])
        eng.set_bic(d['biInput'][:bDof], d['biLabel'][:bDof], bDof, 2.0)
        eng.set_weights(d['w'])
        eng.set_tf_adapt(0, spec, np.random.default_rng(31).uniform(0.5, 2.0, n_k).astype(np.float32))
        rec = {}
        for s in range(2):
            predict_and_compare(0, eng, spec, single_update_bar(rule)['bar'], 'n_k_263173/%s' % rule, rec)
        RECORD['n_k_263173/%s/single_update' % rule] = rec
    finally:
        eng.close()


# ---- 8. through VarNet -------------------------------------------------------------------------------------------------
def _varnet(**kw):
    from varnet_amd.adpde import ADPDE
    from varnet_amd.domain import Domain1D
    from varnet_amd.varnet import VarNet
    pde = ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=0.1, vel=0.5, tInterval=[0, 0.5], IC=lambda x: np.sin(np.pi * x))
    return VarNet(pde, tDiscNum=10, discNum=12, bDiscNum=None, layerWidth=[20, 20], **kw)


@pytest.mark.parametrize('dedup', [False, True], ids=['rowwise', 'dedup'])
def test_through_varnet_train_records_and_checkpoint(tmp_path, dedup):
    """`VarNet(pde, tfAdapt='rba')` on a 12 x 10 1D+t grid, row-wise and de-duplicated: train() registers the batch, the state
    moves once per epoch, tfWeights() and trainRes.tfAdaptHist report it, the case file names the rule, and a checkpoint restored
    into a fresh model continues bit for bit."""
    np.random.seed(0)
    vn = _varnet(tfAdapt={'rule': 'rba', 'eta': 0.05})
    res = vn.train(str(tmp_path / 'run'), epochNum=40, tol=0.0, saveFreq=10, verbose=False, dedup=dedup)
    try:
        assert vn.dedup_state['on'] == dedup, vn.dedup_state
        nt = vn.fixData.nt
        w = vn.tfWeights()
        assert len(w) == 1 and w[0]['omega'].shape == w[0]['lambda'].shape == (nt,)
        st = w[0]['stats']
        assert st['tau'] == 40.0 and abs(st['mean'] - 1.0) <= 1e-12 and st['min'] < 1.0 < st['max'] and 0.0 < st['share'] < 1.0
        assert [e for e, _ in res.tfAdaptHist] == [10, 20, 30, 40]
        assert [h[0]['tau'] for _, h in res.tfAdaptHist] == [10.0, 20.0, 30.0, 40.0]
        case = open(os.path.join(str(tmp_path / 'run'), 'caseData.txt')).read()
        assert 'Self-adaptive test-function weights: rule rba' in case and 'eta = 0.05' in case
        # checkpoint round trip into a fresh model
        arrays = vn.checkpoint_arrays()
        np.random.seed(0)
        vn2 = _varnet(tfAdapt={'rule': 'rba', 'eta': 0.05})
        try:
            td2 = vn2.tData = vn2._build_tdata()
            if dedup:
                td2.enable_dedup()
            vn2.restore_arrays(arrays)
            vn2.engine.set_weights(res.trainWeight)
            w2 = vn2.tfWeights(td2)
            assert np.array_equal(w2[0]['lambda'], w[0]['lambda']) and np.array_equal(w2[0]['omega'], w[0]['omega'])
            assert w2[0]['stats'] == st
            vn.tData.select_mor(0)
            td2.select_mor(0)
            assert same(run_steps(vn.engine, 3), run_steps(vn2.engine, 3))
        finally:
            vn2.engine.close()
    finally:
        vn.engine.close()


def test_through_varnet_loss_lag_is_only_a_readback_schedule(tmp_path):
    """lossLag = 8 against lossLag = 0 with tfAdapt='rba', the stop inside a block: snapshot, rollback and replay carry the state."""
    np.random.seed(0)
    vn = _varnet(tfAdapt='rba')
    probe = np.array(vn.train(str(tmp_path / 'probe'), epochNum=12, tol=0.0, saveFreq=100, verbose=False, lossLag=0).lossAll)
    vn.engine.close()
    assert probe[10] < probe[:10].min()                                   # the loss falls: epoch 11 is the first below tol
    tol = 0.5 * (probe[10] + probe[:10].min())
    runs = []
    for lag in (0, 8):
        np.random.seed(0)
        vn = _varnet(tfAdapt='rba')
        res = vn.train(str(tmp_path / ('lag%d' % lag)), epochNum=40, tol=tol, saveFreq=100, verbose=False, lossLag=lag)
        w = vn.tfWeights()[0]
        runs.append([np.array(res.lossAll), vn.engine.get_params(), w['lambda'], w['omega'], np.array(list(w['stats'].values()))])
        assert vn.engine.step == 11 and w['stats']['tau'] == 11.0         # not one step, not one update beyond the stop
        vn.engine.close()
    assert same(runs[0], runs[1])


def test_through_varnet_set_tf_adapt_and_balance(tmp_path):
    """setTfAdapt re-registers from the initial state or clears; a balance probe between the epochs does not move the state."""
    np.random.seed(0)
    vn = _varnet(tfAdapt='sa')
    try:
        vn.train(str(tmp_path / 'a'), epochNum=6, tol=0.0, saveFreq=100, verbose=False, balance={'rule': 'gradnorm', 'freq': 2})
        st = vn.tfWeights()[0]['stats']
        assert st['tau'] == 6.0 and abs(st['mean'] - 1.0) <= 1e-12       # three probes in between: one update per epoch, no more
        vn.setTfAdapt({'rule': 'rba', 'normalize': False})
        w = vn.tfWeights()[0]
        assert w['stats']['tau'] == 0.0 and np.all(w['lambda'] == 1.0) and np.all(w['omega'] == 1.0)
        vn.setTfAdapt(None)
        with pytest.raises(ValueError, match='self-adaptive weights are off'):
            vn.tfWeights()
        with pytest.raises(VNError, match='error 3'):
            vn.engine.tf_adapt(0)
    finally:
        vn.engine.close()
