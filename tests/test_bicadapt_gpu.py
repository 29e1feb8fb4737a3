"""
GPU tier of the weights on the Dirichlet and initial rows (vn_set_bic_weights, vn_set_bic_adapt, vn_get_bic_adapt,
vn_set_bic_adapt_state, `VarNet(bicWeights=..., bicAdapt=...)`):

    BC = biDimVal (1 / bDof) sum_{i < bDof} omega_i e_i^2, IC likewise over its part; omega_i = m(lambda_i) / Z_s of the COMMITTED
    state of the row's part, constant for the gradient; an adaptive part moves from its own l_i = e_i^2 and the optimizer step
    commits it: omega lags one step.

1. Weights in use: loss components, the unweighted loss field and the gradient against the fp64 restatement
   (tests/bicadapt_ref.py) evaluated with the engine's OWN omega (read through vn_get_bic_adapt), at the project's unchanged
   bars (tests/parity_cases.py: LOSS_RTOL, LVEC_RTOL, GRAD_RTOL through tests/gradcheck.assert_grad_close with its fp32
   conditioning callback) -- the single launch, the two-pass sequence (integNum 216), the de-duplicated step on an identity and on
   a shared-point map, VN_KERNEL_GENERIC, the three polynomial terms, flux rows and observations (which stay unweighted), after
   the state has moved, and static weights with and without normalisation.  vn_eval_loss reports the same numbers.
2. Single update and eight chained steps per rule and part against tests/adapt_ref.py on the engine's own state and loss field,
   at the bar tests/adapt_cases.single_update_bar measures on the CPU (never read from the engine).
3. Bitwise contracts, 4. non-mutation, 5. degenerate fields, 6. every = 3, 7. refusals and replacement in both orders,
8. the `VarNet` layer.

vn_objective_f64 carries the same weights, widened exactly: wherever the restatement itself is the reference (check_in_use) its
loss scalars and gradient are compared in fp64, at FP64_LOSS_RTOL / FP64_GRAD_RTOL.

The figures are written to bicadapt_parity.json in the directory VN_RECORD_DIR names (default: profile_out/ beside tests/; the
committed copy: profiles/bicadapt_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import adapt_cases, adapt_ref, bicadapt_ref, dedup_map_cases as mc, flux_ref, obs_ref
from tests.adapt_cases import rel_dev, single_update_bar
from tests.bicadapt_cases import (BIDIMVAL, BIG, CASES, IDS, IDX, RULES, inputs, lambda0, omega_rows, parity_spec, parts_of, reference,
                                  rows, theta, weights_are_real)
from tests.gradcheck import assert_grad_close, assert_pair_close, block_errors
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL
from varnet_amd.engine import VN_KERNEL_AUTO, VN_KERNEL_FUSED, VN_KERNEL_GENERIC, VN_KERNEL_LAYERED, VNEngine, VNError

pytestmark = pytest.mark.gpu

KEYS = ['loss', 'BCloss', 'ICloss', 'varLoss']
# fp64 on both sides, the sums in another order: n eps with n up to 2.6e5 rows is 6e-11 at worst and sqrt(n) eps = 1e-13 typically;
# the bars tests/test_adapt_gpu.py uses for the same entry point
FP64_LOSS_RTOL = 1e-12
FP64_GRAD_RTOL = 1e-11
RECORD = {}
KNAME = {VN_KERNEL_AUTO: 'auto', VN_KERNEL_GENERIC: 'generic'}
PART = ('bc', 'ic')


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        RECORD['single_update_bar'] = {r: single_update_bar(r) for r in RULES}
        with open(os.path.join(out, 'bicadapt_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def register_interior(eng, i, batch=0):
    d = inputs(i)
    eng.set_interior(batch, d['Input'], d['gcoef'], None, n_k=CASES[i][5], detJ=d['detJ'])


def make_engine(i, kernel=VN_KERNEL_AUTO, spec=None, parts=None, optimizer='adam', lam=True, xcheck=False):
    """An engine of CASES[i]; spec: the adaptive registration of `parts` (default: every part that has rows), started from
    lambda0 (lam=False: from the spec's init)."""
    name, d_in, dim, widths, q, n_k, nB, bDof, td = CASES[i]
    d = inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, kernel=kernel, optimizer_name=optimizer, xcheck=xcheck)
    eng.set_params(theta(i))
    eng.set_fe_table(d['N1'], d['dNt1'], None)
    register_interior(eng, i)
    eng.set_bic(d['biInput'], d['biLabel'], bDof, BIDIMVAL)
    eng.set_weights(d['w'])
    if spec is not None:
        for s in (parts_of(i) if parts is None else parts):
            eng.set_bic_adapt(s, spec, lambda0(i, s) if lam else None)
    return eng


def grad_of(eng, batch=0):
    gb = eng.bind_grad_buffer()
    eng.grad(batch)
    torch.cuda.synchronize()
    return gb.cpu().numpy().astype(np.float64)


def state_of(eng):
    """The committed state of every registered part as a list of arrays, for bitwise comparison."""
    out = []
    for p in sorted(eng.bic_parts()):
        s = eng.bic_adapt(p)
        st = s['stats']
        out += [s['lambda'], s['omega'], np.array([st[k] for k in ('min', 'max', 'mean', 'share', 'Z', 'tau')])]
        if s['slots'] is not None:
            out.append(s['slots'])
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def engine_omega(i, eng):
    """One weight per row from the engine's own committed state (an unregistered part: 1), fp64."""
    return omega_rows(i, {IDX_PART[p]: eng.bic_adapt(p)['omega'].astype(np.float64) for p in eng.bic_parts()})


IDX_PART = {'bc': 0, 'ic': 1}


def check_parity(net, eng, ref, tag, g32, fields=None):
    """eval_loss (with the unweighted interior lossVec) and grad of batch 0 against ref = (result, gradient); the rows' own
    loss field (read back after the gradient evaluation) against ref['field']; prints and records every figure, then asserts."""
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
    for p in eng.bic_parts():
        f = np.asarray((fields or ref['field'])[IDX_PART[p]], dtype=np.float64)
        rec['field_' + p] = float(np.max(np.abs(eng.bic_adapt(p)['lossfield'] - f)) / np.max(np.abs(f)))
    errs = block_errors(g, gref, d_in, widths, dim, td)
    rec['worst_block'] = max(errs, key=errs.get)
    rec['worst_block_err'] = errs[rec['worst_block']]
    rec['kernel_path'] = list(eng.kernel_path())
    RECORD[tag] = rec
    print('bicadapt %s: %s' % (tag, json.dumps(rec, sort_keys=True)))
    for got, key in zip(out, KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'eval', key, got, ref[key])
    for got, key in zip(g[P:], KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'grad', key, got, ref[key])
    assert rec['lossVec'] <= LVEC_RTOL, (tag, rec['lossVec'])
    for p in eng.bic_parts():
        assert rec['field_' + p] <= LVEC_RTOL, (tag, p, rec['field_' + p])  # the field is the UNWEIGHTED one of the reference
    assert_grad_close(g[:P], gref, d_in, widths, GRAD_RTOL, dim=dim, td=td, what=tag, g32=g32)
    return g


def net_of(i):
    return CASES[i][1], CASES[i][2], CASES[i][3], CASES[i][8]


def check_fp64(net, eng, ref, tag):
    """vn_objective_f64 against ref = (result, gradient) in fp64; it leaves the committed and the pending state alone."""
    d_in, dim, widths, td = net
    ref, gref = ref
    st = state_of(eng)
    o64, g64, _ = eng.objective64(0, grad=True)
    assert same(state_of(eng), st)
    rec = {'f64_' + k: abs(got - ref[k]) / max(abs(ref[k]), 1e-300) for got, k in zip(o64, KEYS)}
    errs = block_errors(g64.cpu().numpy(), gref, d_in, widths, dim, td)
    rec['f64_worst_block_err'] = max(errs.values())
    RECORD.setdefault(tag, {}).update(rec)
    print('bicadapt %s fp64: %s' % (tag, json.dumps(rec, sort_keys=True)))
    for got, key in zip(o64, KEYS):
        assert abs(got - ref[key]) <= FP64_LOSS_RTOL * abs(ref[key]) + 1e-300, (tag, 'f64', key, got, ref[key])
    assert max(errs.values()) <= FP64_GRAD_RTOL, (tag, errs)


def check_in_use(i, eng, tag):
    """The restatement evaluated at the engine's parameters with the engine's own committed omega, in fp32 and in fp64."""
    om = engine_omega(i, eng)
    flat = eng.get_params()
    ref = reference(i, om, flat)
    g = check_parity(net_of(i), eng, ref, tag, lambda: reference(i, om, flat, dtype=np.float32)[1])
    check_fp64(net_of(i), eng, ref, tag)
    return g


# ---- 1. weights in use -----------------------------------------------------------------------------------------------
IN_USE = [(i, VN_KERNEL_AUTO) for i in range(len(CASES))] + [(IDX['n33_21'], VN_KERNEL_GENERIC), (IDX['n300_257'], VN_KERNEL_GENERIC)]


@pytest.mark.parametrize('i,kernel', IN_USE, ids=['%s-%s' % (IDS[i], KNAME[k]) for i, k in IN_USE])
def test_weights_in_use_parity(i, kernel):
    """Every (nB, bDof) of the issue on its route: the single launch, the two-pass sequence (twopass33_21) and the generic kernels."""
    weights_are_real(i)
    eng = make_engine(i, kernel, parity_spec('rba'))
    try:
        assert sorted(eng.bic_parts()) == [PART[s] for s in parts_of(i)]
        for s in parts_of(i):
            st = eng.bic_adapt(s)
            assert np.array_equal(st['lambda'], lambda0(i, s)) and st['stats']['tau'] == 0.0 and st['stats']['Z'] == 1.0
            assert rel_dev(st['omega'], lambda0(i, s).astype(np.float64) ** 2) <= 2.0 ** -23
        if CASES[i][0] == 'twopass33_21':
            assert eng.kernel_path()[1] == 1
        g1 = check_in_use(i, eng, '%s/%s' % (IDS[i], KNAME[kernel]))
        assert np.array_equal(g1, grad_of(eng))                           # two calls: the same bits
    finally:
        eng.close()


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('i', [IDX['n33_21'], IDX['n77_40']], ids=['n33_21', 'n77_40'])
def test_weights_in_use_after_the_state_has_moved(i, rule):
    """Three steps at a large rate, then the same comparison: the weights in use are those of the committed state."""
    kw = dict(eta=0.5, gamma=0.9) if rule == 'rba' else dict(lr=0.1)
    eng = make_engine(i, spec=parity_spec(rule, **kw))
    try:
        om0 = {p: eng.bic_adapt(p)['omega'] for p in eng.bic_parts()}
        for _ in range(3):
            eng.train_step(0)
        for p in eng.bic_parts():
            s = eng.bic_adapt(p)
            assert s['stats']['tau'] == 3.0 and rel_dev(s['omega'], om0[p]) > 1e-2
        check_in_use(i, eng, '%s/%s/moved' % (IDS[i], rule))
    finally:
        eng.close()


@pytest.mark.parametrize('normalize', [False, True], ids=['raw', 'normalized'])
def test_static_weights_in_use(normalize):
    """vn_set_bic_weights: the weights as given, or divided per part by their mean; then an adaptive 'ic' part replaces the static
    one of that part only."""
    i = IDX['n33_21']
    om = np.concatenate([lambda0(i, 0), lambda0(i, 1)]).astype(np.float32)
    eng = make_engine(i)
    try:
        eng.set_bic_weights(om, normalize=normalize)
        assert eng.bic_parts() == {'bc': 'static', 'ic': 'static'}
        want = bicadapt_ref.static_weights(om.astype(np.float64), CASES[i][7], normalize)
        assert rel_dev(engine_omega(i, eng), want) <= 2.0 ** -23
        assert np.array_equal(eng.bic_adapt('bc')['lambda'], lambda0(i, 0))
        check_in_use(i, eng, 'static/%s' % ('normalized' if normalize else 'raw'))
        st = state_of(eng)
        eng.train_step(0)
        assert same(state_of(eng), st)                                    # a static part never moves
        eng.set_bic_adapt('ic', parity_spec('sa'), lambda0(i, 1))
        assert eng.bic_parts()['bc'] == 'static' and eng.bic_parts()['ic']['rule'] == 'sa'
        check_in_use(i, eng, 'static_bc_adaptive_ic/%s' % ('normalized' if normalize else 'raw'))
    finally:
        eng.close()


@pytest.mark.parametrize('i', [IDX['n50_30'], IDX['n33_21']], ids=['n50_30', 'n33_21'])
def test_weights_in_use_dedup_identity_map(i):
    eng = make_engine(i, spec=parity_spec('sa'))
    try:
        g_row = grad_of(eng)
        nT = inputs(i)['Input'].shape[0]
        idx = torch.arange(nT, dtype=torch.int32)
        eng.set_dedup(0, inputs(i)['Input'], idx, torch.arange(nT + 1, dtype=torch.int32), idx)
        g1 = check_in_use(i, eng, '%s/dedup_identity' % IDS[i])
        assert np.array_equal(g1, grad_of(eng)) and not np.array_equal(g1, g_row)                    # another formulation ran
        eng.train_step(0)                                                 # ... whose step moves the state, too
        assert all(eng.bic_adapt(p, arrays=False)['stats']['tau'] == 1.0 for p in eng.bic_parts())
        check_in_use(i, eng, '%s/dedup_identity/moved' % IDS[i])
    finally:
        eng.close()


def _delta_reference(base, d_in, widths, biInput, biLabel, bDof, w, omega, flat, f=np.float64):
    """An unweighted reference of any problem on these rows plus what the weights add (tests/bicadapt_ref.bic_delta)."""
    ref, g = base
    dl, dg = bicadapt_ref.bic_delta(np.asarray(flat).astype(f), d_in, widths, np.asarray(biInput).astype(f), np.asarray(biLabel).astype(f),
                                    bDof, f(BIDIMVAL), np.asarray(w, dtype=f), True, np.asarray(omega, dtype=f))
    out = dict(ref)
    for k in ('loss', 'BCloss', 'ICloss'):
        out[k] = float(ref[k]) + float(dl[k])
    out['field'] = dl['field']
    return out, np.asarray(g, dtype=np.float64) + dg


def test_weights_in_use_dedup_shared_point_map():
    """The 'hot_point' map of tests/dedup_map_cases.py (7680 rows on 300 points), its own BC/IC rows weighted."""
    name = 'hot_point'
    d_in, dim, widths, q, act, source, integW = mc.config(name)[:7]
    assert act == 'sigmoid'
    d = mc.inputs(name)
    n_k, bDof, nB = d['n_k'], d['bDof'], d['biInput'].shape[0]
    lam = [np.random.default_rng(31 + s).uniform(0.5, 2.0, n).astype(np.float32) for s, n in enumerate((bDof, nB - bDof))]
    eng = VNEngine(dim, d_in, widths, True, q, isSource=source, integWflag=integW, activationFun=act)
    try:
        eng.set_params(mc.theta(name))
        eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
        eng.set_bic(d['biInput'], d['biLabel'], bDof, mc.BIDIMVAL)
        eng.set_weights(d['w'])
        eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=mc.DETJ)
        eng.set_dedup(0, d['Xu'], d['uid'], d['rowptr'], d['rowidx'])
        for s in (0, 1):
            eng.set_bic_adapt(s, parity_spec('rba'), lam[s])
        om = np.concatenate([eng.bic_adapt(s)['omega'].astype(np.float64) for s in (0, 1)])
        assert mc.BIDIMVAL == BIDIMVAL
        ev = lambda dt, f: _delta_reference(mc.oracle(name, dt), d_in, widths, d['biInput'], d['biLabel'], bDof, d['w'], om, mc.theta(name), f)
        ref, gref = ev(torch.float64, np.float64)
        ref0, g0 = mc.oracle(name)
        assert abs(ref['BCloss'] - ref0['BCloss']) > 1e-2 * abs(ref['BCloss']) and np.linalg.norm(gref - g0) > 1e-2 * np.linalg.norm(gref)
        check_parity((d_in, dim, widths, True), eng, (ref, gref), 'dedup_map/%s' % name, lambda: ev(torch.float32, np.float32)[1])
        eng.train_step(0)
        assert eng.bic_adapt('ic', arrays=False)['stats']['tau'] == 1.0
    finally:
        eng.close()


def test_weights_in_use_with_all_three_terms():
    """Case 3 of tests/adapt_cases.py (the 5 x 50 network, (nB, bDof) = (77, 40)) with reaction, flux term and diffusivity D(u):
    their reference, unweighted, plus what the rows' weights add."""
    from tests.test_adapt_gpu import make_engine as adapt_engine
    i = 3
    c = adapt_cases.CASES[i]
    d_in, dim, widths, nB, bDof, td, act = c[0], c[1], c[2], c[5], c[6], c[7], c[8]
    assert act == 'sigmoid' and td
    d = adapt_cases.inputs(i)
    lam = [np.random.default_rng(31 + s).uniform(0.5, 2.0, n).astype(np.float32) for s, n in enumerate((bDof, nB - bDof))]
    eng = adapt_engine(i, variant='terms')
    try:
        for s in (0, 1):
            eng.set_bic_adapt(s, parity_spec('rba'), lam[s])
        om = np.concatenate([eng.bic_adapt(s)['omega'].astype(np.float64) for s in (0, 1)])
        flat = adapt_cases.theta(i)
        ev = lambda dt, f: _delta_reference(adapt_cases.reference(i, None, 'terms', flat, dt), d_in, widths, d['biInput'], d['biLabel'],
                                            bDof, d['w'], om, flat, f)
        check_parity((d_in, dim, widths, td), eng, ev(torch.float64, np.float64), 'terms/%s' % adapt_cases.IDS[i],
                     lambda: ev(torch.float32, np.float32)[1])
    finally:
        eng.close()


def test_flux_rows_and_observations_stay_unweighted():
    """n33_21 with boundary-flux rows and observations registered: both terms enter as they do without the weights."""
    i = IDX['n33_21']
    name, d_in, dim, widths, q, n_k, nB, bDof, td = CASES[i]
    rng = np.random.default_rng(51)
    nF, nO = 19, 13
    nrm = rng.standard_normal((nF, dim))
    flux = dict(X=rng.uniform(-1, 1, (nF, d_in)).astype(np.float32), normal=(nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32),
                coef=rng.uniform(0.5, 1.5, nF).astype(np.float32), label=rng.standard_normal(nF).astype(np.float32))
    obs = dict(X=rng.uniform(-1, 1, (nO, d_in)).astype(np.float32), value=rng.standard_normal(nO).astype(np.float32))
    lam_obs = 0.75
    w = inputs(i)['w']
    eng = make_engine(i, spec=parity_spec('rba'))
    try:
        eng.set_flux_bc(flux['X'], flux['normal'], flux['coef'], flux['label'], BIDIMVAL)
        eng.set_observations(obs['X'], obs['value'], weight=lam_obs)
        om = engine_omega(i, eng)
        flat = eng.get_params()

        def ev(f):
            dt = torch.float64 if f == np.float64 else torch.float32
            ref, g = reference(i, om, flat, dtype=f)
            F, gF, _ = flux_ref.flux_term(flat.astype(f), d_in, widths, dim, flux['X'].astype(f), flux['normal'].astype(f),
                                          flux['coef'].astype(f), flux['label'].astype(f), BIDIMVAL, dtype=dt)
            O, gO, _ = obs_ref.obs_term(flat.astype(f), d_in, widths, dim, obs['X'].astype(f), obs['value'].astype(f), dtype=dt)
            ref = dict(ref)
            ref['BCloss'] = float(ref['BCloss']) + F
            ref['loss'] = float(ref['loss']) + w[0] * F + lam_obs * O
            return ref, np.asarray(g, dtype=np.float64) + w[0] * gF + lam_obs * gO
        ref, gref = ev(np.float64)
        plain, gplain = reference(i, om, flat)
        assert np.linalg.norm(gref - gplain) > 1e-2 * np.linalg.norm(gref)       # the two terms are a real part of the gradient
        check_parity(net_of(i), eng, (ref, gref), 'flux_obs/%s' % IDS[i], lambda: ev(np.float32)[1])
        check_fp64(net_of(i), eng, (ref, gref), 'flux_obs/%s' % IDS[i])
    finally:
        eng.close()


# ---- 2. single update ------------------------------------------------------------------------------------------------
def predict_and_compare(eng, part, spec, bar, tag, rec):
    """One step: the part's state before it, the loss field the step's own gradient evaluation wrote (read back through
    vn_get_bic_adapt before the optimizer step commits), the fp64 prediction, the comparison."""
    before = eng.bic_adapt(part)
    eng.grad(0)
    field = eng.bic_adapt(part)['lossfield'].astype(np.float64)
    eng.apply()
    want = adapt_ref.step(before['lambda'].astype(np.float64), None if before['slots'] is None else before['slots'].astype(np.float64),
                          int(before['stats']['tau']), field, spec)
    after = eng.bic_adapt(part)
    dev = {'lambda': rel_dev(after['lambda'], want['lam']), 'omega': rel_dev(after['omega'], want['omega']),
           'slots': 0.0 if want['slots'] is None else rel_dev(after['slots'], want['slots']),
           'stats': max(rel_dev(after['stats'][k], want['stats'][k]) for k in ('min', 'max', 'mean', 'share', 'Z'))}
    for k, v in dev.items():
        rec[k] = max(rec.get(k, 0.0), v)
    assert after['stats']['tau'] == want['stats']['tau'], (tag, after['stats'], want['stats'])
    assert max(dev.values()) <= bar, (tag, dev, bar)
    return before, after


SINGLE = [(i, s) for i in (IDX['n50_30'], IDX['n33_21'], IDX['n77_40'], IDX['n5_4'], IDX['steady40'], IDX['n300_257'], BIG) for s in parts_of(i)]


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('i,part', SINGLE, ids=['%s-%s' % (IDS[i], PART[s]) for i, s in SINGLE])
def test_single_update_chained_over_eight_steps(i, part, rule):
    """Both parts registered, each compared on its own field.  The one-row 'ic' part of n5_4 runs without normalisation (its
    normalised weight is 1 whatever lambda is)."""
    bar = single_update_bar(rule)['bar']
    spec = adapt_ref.spec_of(rule, **({'normalize': False} if rows(i)[part] == 1 else {}))
    eng = make_engine(i, spec=spec)
    rec = {'bar': bar}
    tag = '%s/%s/%s/single_update' % (IDS[i], PART[part], rule)
    try:
        for s in range(8 if i != BIG else 2):
            before, after = predict_and_compare(eng, part, spec, bar, tag, rec)
            assert after['stats']['tau'] == s + 1
            assert not np.array_equal(after['lambda'], before['lambda'])
    finally:
        RECORD[tag] = rec
        print('bicadapt %s: %s' % (tag, json.dumps(rec, sort_keys=True)))
        eng.close()


@pytest.mark.parametrize('rule', RULES)
def test_the_parts_run_their_own_rules(rule):
    """bc under one rule, ic under the other, other parameters each: every part follows its own."""
    i = IDX['n77_40']
    other = 'sa' if rule == 'rba' else 'rba'
    specs = {0: adapt_ref.spec_of(rule, power=1), 1: adapt_ref.spec_of(other, every=1, normalize=False)}
    eng = make_engine(i)
    try:
        for s in (0, 1):
            eng.set_bic_adapt(s, specs[s], lambda0(i, s))
        for step in range(3):
            b0, b1 = eng.bic_adapt(0), eng.bic_adapt(1)
            eng.grad(0)
            f = [eng.bic_adapt(s)['lossfield'].astype(np.float64) for s in (0, 1)]
            eng.apply()
            for s, b in ((0, b0), (1, b1)):
                want = adapt_ref.step(b['lambda'].astype(np.float64), None if b['slots'] is None else b['slots'].astype(np.float64),
                                      int(b['stats']['tau']), f[s], specs[s])
                got = eng.bic_adapt(s)
                assert rel_dev(got['lambda'], want['lam']) <= single_update_bar(specs[s]['rule'])['bar']
                assert rel_dev(got['omega'], want['omega']) <= single_update_bar(specs[s]['rule'])['bar']
                assert got['stats']['tau'] == step + 1
    finally:
        eng.close()


# ---- 6. every = 3 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rule', RULES)
def test_every_three_updates_on_every_third_step(rule):
    i = IDX['n33_21']
    spec = adapt_ref.spec_of(rule, every=3)
    eng = make_engine(i, spec=spec, parts=[1])
    try:
        taus = []
        for s in range(8):
            st = state_of(eng)
            eng.train_step(0)
            assert same(state_of(eng), st) == (s % 3 != 0)
            taus.append(eng.bic_adapt('ic', arrays=False)['stats']['tau'])
        assert taus == [1, 1, 1, 2, 2, 2, 3, 3]
    finally:
        eng.close()


# ---- 3. bitwise contracts ----------------------------------------------------------------------------------------------
BITWISE = [(IDX['n33_21'], 'rba'), (IDX['n33_21'], 'sa'), (IDX['n300_257'], 'sa'), (IDX['twopass33_21'], 'rba')]
BITWISE_IDS = ['%s-%s' % (IDS[i], r) for i, r in BITWISE]


def run_steps(eng, n, batch=0):
    for _ in range(n):
        eng.train_step(batch)
    torch.cuda.synchronize()
    return [eng.get_params()] + state_of(eng)


def static_twin(i, eng):
    """An engine with the committed omega of `eng` as a static registration (lambda = omega, m(x) = x, Z = 1: the same bits)."""
    twin = make_engine(i)
    twin.set_bic_weights(engine_omega(i, eng).astype(np.float32), normalize=False)
    return twin


@pytest.mark.parametrize('i,rule', BITWISE, ids=BITWISE_IDS)
def test_two_engines_and_step_is_grad_plus_apply(i, rule):
    """Two engines on the same sequence give the same bits.  train_step against grad + apply: the two forms of the optimizer step
    differ in theta by an ulp here and there without any weights (tests/test_periodic_gpu.py measures that gap), so the contract
    is pinned where it can hold bit for bit: from one exported state both forms leave the SAME adaptive state, and each leaves
    the theta its own form leaves on a static registration of the committed omega."""
    spec = adapt_ref.spec_of(rule)
    a, b, c = (make_engine(i, spec=spec) for _ in range(3))
    twins = []
    try:
        ra = run_steps(a, 4)
        assert same(ra, run_steps(b, 4))
        assert a.step == 4 and a.bic_adapt('bc', arrays=False)['stats']['tau'] == 4.0
        plain_bytes = make_engine_bytes(i)
        for _ in range(2):
            buf = a.export_state()
            c.import_state(buf)
            s1, s2 = static_twin(i, a), static_twin(i, a)
            twins += [s1, s2]
            for twin in (s1, s2):
                head = np.concatenate([buf[:plain_bytes], twin.export_state()[plain_bytes:]])
                twin.import_state(head)                                   # step, theta and both slots: the prefix of the layout
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
        for e in [a, b, c] + twins:
            e.close()


def make_engine_bytes(i):
    eng = make_engine(i)
    try:
        return eng.export_state().size
    finally:
        eng.close()


@pytest.mark.parametrize('i,rule', BITWISE[:2], ids=BITWISE_IDS[:2])
def test_grad_twice_without_apply(i, rule):
    spec = adapt_ref.spec_of(rule)
    eng, once = make_engine(i, spec=spec), make_engine(i, spec=spec)
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
        assert eng.bic_adapt('ic', arrays=False)['stats']['tau'] == 1.0
    finally:
        eng.close()
        once.close()


@pytest.mark.parametrize('rule', RULES)
def test_train_epoch_over_two_batches_that_share_the_rows(rule):
    """The state belongs to the row set: a step of either batch applies it and moves it, once per step."""
    i = IDX['n33_21']
    spec = adapt_ref.spec_of(rule)
    a, b = make_engine(i, spec=spec), make_engine(i, spec=spec)
    try:
        for e in (a, b):
            register_interior(e, i, batch=1)
        acc = torch.zeros(1, device='cuda')
        a.train_epoch((0, 1, 0), acc)
        for k in (0, 1, 0):
            b.train_step(k)
        torch.cuda.synchronize()
        assert same([a.get_params()] + state_of(a), [b.get_params()] + state_of(b))
        assert a.step == 3 and all(a.bic_adapt(p, arrays=False)['stats']['tau'] == 3.0 for p in ('bc', 'ic'))
        assert np.isfinite(acc.item())
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('i,rule', BITWISE[:3], ids=BITWISE_IDS[:3])
def test_snapshot_rollback_replay_and_export_import(i, rule):
    spec = adapt_ref.spec_of(rule)
    eng, fresh = make_engine(i, spec=spec), make_engine(i, spec=spec, lam=False)
    plain = make_engine(i)
    try:
        n = rows(i)
        per = lambda m: 8 * 8 + (4 if rule == 'sa' else 2) * 4 * m      # scalars, then lambda, omega[, m1, m2] of a part
        assert eng.export_state().size == plain.export_state().size + per(n[0]) + per(n[1])
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
        # vn_set_bic_adapt_state: lambda, slots and tau put back, omega and the statistics rebuilt to the same bits
        s = eng.bic_adapt('ic')
        fresh.set_bic_adapt_state('ic', np.ones_like(s['lambda']), None, 0)
        assert not same(state_of(fresh), state_of(eng))
        fresh.set_bic_adapt_state('ic', s['lambda'], s['slots'], int(s['stats']['tau']))
        assert same(state_of(fresh), state_of(eng))
        # vn_params_init returns to the registered initial state
        eng.init_params(seed=1)
        for p in (0, 1):
            s0 = eng.bic_adapt(p)
            assert np.array_equal(s0['lambda'], lambda0(i, p)) and s0['stats']['tau'] == 0.0
            assert s0['slots'] is None or not s0['slots'].any()
    finally:
        for e in (eng, fresh, plain):
            e.close()


def both_kinds_engine(i, lam_tf=None):
    """A batch state and both part states on one engine: batch 0 'sa', bc 'rba' on every second step, ic 'sa', each from
    non-uniform initial lambdas (lam_tf None: each from its spec's init) -- states without and with slots interleaved, one of
    them not pending on every second step."""
    eng = make_engine(i)
    eng.set_tf_adapt(0, adapt_ref.spec_of('sa'), lam_tf)
    eng.set_bic_adapt('bc', adapt_ref.spec_of('rba', every=2), None if lam_tf is None else lambda0(i, 0))
    eng.set_bic_adapt('ic', adapt_ref.spec_of('sa'), None if lam_tf is None else lambda0(i, 1))
    return eng


def both_kinds_state(eng):
    s = eng.tf_adapt(0)
    return [s['lambda'], s['omega'], s['slots'], np.array([s['stats'][k] for k in STATS])] + state_of(eng)


STATS = ('min', 'max', 'mean', 'share', 'Z', 'tau')


def test_batch_and_part_states_on_one_engine_share_one_layout():
    """vn_set_tf_adapt next to vn_set_bic_adapt: the exported state holds the batch's, then bc's, then ic's; snapshot, rollback,
    import and vn_params_init reach all three.  n33_21: n_k = 9 and the parts' 21 and 12 rows are no multiples of 4, so every
    piece's 16-byte stride on the device differs from its length in the exported bytes."""
    i = IDX['n33_21']
    n_k, n = CASES[i][5], rows(i)
    lam_tf = np.random.default_rng(29).uniform(0.5, 2.0, n_k).astype(np.float32)
    eng, twin, plain = both_kinds_engine(i, lam_tf), both_kinds_engine(i), make_engine(i)
    try:
        assert (n_k, n) == (9, (21, 12))
        plain_bytes = plain.export_state().size
        assert eng.export_state().size == plain_bytes + (64 + 4 * 4 * 9) + (64 + 2 * 4 * 21) + (64 + 4 * 4 * 12)
        run_steps(eng, 3)                                                 # an odd count: bc has skipped a step, the others none
        assert eng.bic_adapt('bc', arrays=False)['stats']['tau'] < 3.0 == eng.bic_adapt('ic', arrays=False)['stats']['tau']
        assert eng.tf_adapt(0, arrays=False)['stats']['tau'] == 3.0
        # the bytes behind the optimizer block: per state the scalars, then lambda, omega[, m1, m2], unpadded
        buf = eng.export_state()
        at = plain_bytes
        for s, m in ((eng.tf_adapt(0), n_k), (eng.bic_adapt('bc'), n[0]), (eng.bic_adapt('ic'), n[1])):
            scal = np.frombuffer(buf[at:at + 64].tobytes(), np.float64)
            assert np.array_equal(scal[:6], np.array([s['stats'][k] for k in STATS]))
            at += 64
            pieces = [s['lambda'], s['omega']] + ([] if s['slots'] is None else [s['slots'][0], s['slots'][1]])
            for piece in pieces:
                assert piece.shape == (m,) and np.array_equal(np.frombuffer(buf[at:at + 4 * m].tobytes(), np.float32), piece)
                at += 4 * m
        assert at == buf.size and eng.bic_adapt('bc')['slots'] is None and eng.tf_adapt(0)['slots'] is not None
        # snapshot / rollback
        eng.state_snapshot()
        s3, p3 = both_kinds_state(eng), eng.get_params()
        r5 = run_steps(eng, 5) + both_kinds_state(eng)
        assert not same(both_kinds_state(eng), s3)
        eng.state_rollback()
        assert same(both_kinds_state(eng), s3) and eng.step == 3 and np.array_equal(eng.get_params(), p3)
        assert same(run_steps(eng, 5) + both_kinds_state(eng), r5)       # replay: the same bits
        # import into an engine registered the same way from the specs' init
        twin.import_state(eng.export_state())
        assert same(both_kinds_state(twin), both_kinds_state(eng)) and twin.step == eng.step == 8
        assert same(run_steps(twin, 3) + both_kinds_state(twin), run_steps(eng, 3) + both_kinds_state(eng))
        # vn_params_init returns all three to their registered initial lambdas
        eng.init_params(seed=1)
        for s, lam in ((eng.tf_adapt(0), lam_tf), (eng.bic_adapt('bc'), lambda0(i, 0)), (eng.bic_adapt('ic'), lambda0(i, 1))):
            assert np.array_equal(s['lambda'], lam) and s['stats']['tau'] == 0.0
            assert s['slots'] is None or not s['slots'].any()
    finally:
        for e in (eng, twin, plain):
            e.close()


def _snapshot(eng):
    out, lv = eng.eval_loss(0, lossVec=True)
    g = grad_of(eng).copy()
    for _ in range(3):
        eng.train_step(0)
    torch.cuda.synchronize()
    return [np.array(out), lv.cpu().numpy(), g, eng.get_params(), eng.export_state()]


CLEAR = [(IDX['n33_21'], VN_KERNEL_AUTO), (IDX['n33_21'], VN_KERNEL_GENERIC), (IDX['twopass33_21'], VN_KERNEL_AUTO)]


@pytest.mark.parametrize('i,kernel', CLEAR, ids=['%s-%s' % (IDS[i], KNAME[k]) for i, k in CLEAR])
def test_register_then_clear_is_bitwise_untouched(i, kernel):
    """Loss, loss field, gradient, three steps and the exported state (vn_state_size with it) of an engine that registered and
    cleared -- part by part, through vn_set_bic_weights(NULL), or by a new vn_set_bic -- against one that never registered."""
    def run(how):
        eng = make_engine(i, kernel, None if how == 'never' else adapt_ref.spec_of('sa'))
        try:
            if how != 'never':
                eng.grad(0)                                               # an evaluation with the weights, a pending state ...
                if how == 'parts':
                    eng.set_bic_adapt('bc')
                    eng.set_bic_adapt('ic')
                elif how == 'weights_null':
                    eng.set_bic_weights(None)
                else:
                    d = inputs(i)
                    eng.set_bic(d['biInput'], d['biLabel'], CASES[i][7], BIDIMVAL)
                assert eng.bic_parts() == {}
            return _snapshot(eng)
        finally:
            eng.close()
    never = run('never')
    for how in ('parts', 'weights_null', 'set_bic'):
        assert same(never, run(how)), how


@pytest.mark.parametrize('i,kernel', CLEAR + [(IDX['n300_257'], VN_KERNEL_AUTO)],
                         ids=['%s-%s' % (IDS[i], KNAME[k]) for i, k in CLEAR] + ['n300_257-auto'])
def test_identity_registration_agrees_with_the_unregistered_step(i, kernel):
    """omega = 1, static: the rows' own pass against the step's main launch, another path, so within GRAD_RTOL, not bitwise."""
    eng, plain = make_engine(i, kernel), make_engine(i, kernel)
    try:
        eng.set_bic_weights(np.ones(sum(rows(i)), dtype=np.float32))
        assert np.all(engine_omega(i, eng) == 1.0)
        g, g0 = grad_of(eng), grad_of(plain)
        d_in, dim, widths, td = net_of(i)
        for a, b in zip(g[eng.P:], g0[eng.P:]):
            assert abs(a - b) <= LOSS_RTOL * abs(b) + 1e-7
        om = np.ones(sum(rows(i)))
        dev32 = lambda: block_errors(reference(i, om, dtype=np.float32)[1], reference(i, om)[1], d_in, widths, dim, td)
        assert_pair_close(g[:eng.P], g0[:eng.P], d_in, widths, GRAD_RTOL, dev32=dev32, dim=dim, td=td, what='identity/%s' % IDS[i])
    finally:
        eng.close()
        plain.close()


# ---- 4. non-mutation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rule', RULES)
def test_loss_only_calls_and_probes_leave_the_state_alone(rule):
    i = IDX['n33_21']
    spec = adapt_ref.spec_of(rule)
    eng, quiet = make_engine(i, spec=spec), make_engine(i, spec=spec)
    try:
        for e in (eng, quiet):
            e.train_step(0)
        eng.grad(0)                                                       # a pending state, which the calls below must keep as well
        quiet.grad(0)
        st = state_of(eng)
        out, _ = eng.eval_loss(0, lossVec=True)
        assert same(state_of(eng), st)
        ref, _ = reference(i, engine_omega(i, eng), eng.get_params())
        for got, key in zip(out, KEYS):
            assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7  # the committed omega, not the pending one
        check_fp64(net_of(i), eng, reference(i, engine_omega(i, eng), eng.get_params()), 'non_mutation/%s' % rule)
        assert same(state_of(eng), st)                                    # the committed omega, widened; nothing moved
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


# ---- 5. degenerate fields ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['zero', 'nan'])
@pytest.mark.parametrize('dead', [0, 1], ids=['bc', 'ic'])
@pytest.mark.parametrize('rule', RULES)
def test_a_degenerate_field_leaves_its_part_alone_while_the_other_moves(rule, dead, how):
    """theta = 0 makes the network's output exactly 0; labels of one part set to that output give l = 0 on it ('zero'), or one
    label of the part is NaN ('nan').  That part's state, slots and tau stay bit for bit; the other part moves."""
    i = IDX['n33_21']
    name, d_in, dim, widths, q, n_k, nB, bDof, td = CASES[i]
    d = inputs(i)
    lab = d['biLabel'].copy()
    sl = slice(0, bDof) if dead == 0 else slice(bDof, nB)
    if how == 'zero':
        lab[sl] = 0.0
    else:
        lab[sl.start + 3] = np.nan
    spec = adapt_ref.spec_of(rule)
    eng = make_engine(i)
    try:
        eng.set_params(np.zeros(eng.P, dtype=np.float32))
        assert not eng.forward(d['biInput']).cpu().numpy().any()
        eng.set_bic(d['biInput'], lab, bDof, BIDIMVAL)
        for s in (0, 1):
            eng.set_bic_adapt(s, spec, lambda0(i, s))
        before = {s: eng.bic_adapt(s) for s in (0, 1)}
        eng.grad(0)
        eng.apply()
        after = {s: eng.bic_adapt(s) for s in (0, 1)}
        a, b = after[dead], before[dead]
        assert np.array_equal(a['lambda'], b['lambda']) and np.array_equal(a['omega'], b['omega']) and a['stats'] == b['stats']
        assert a['slots'] is None or np.array_equal(a['slots'], b['slots'])
        live = 1 - dead
        assert after[live]['stats']['tau'] == 1.0 and not np.array_equal(after[live]['lambda'], before[live]['lambda'])
        f = eng.bic_adapt(dead)['lossfield']
        assert (not f.any()) if how == 'zero' else np.isnan(f[3])
    finally:
        eng.close()


# ---- 7. refusals and replacement -----------------------------------------------------------------------------------------
def test_registration_errors_and_replacement():
    i = IDX['n33_21']
    eng = make_engine(i)
    steady = make_engine(IDX['steady40'])
    try:
        with pytest.raises(VNError, match='error 3: vn_get_bic_adapt: the ic part has no registration'):
            eng.bic_adapt('ic')
        with pytest.raises(VNError, match='error 1: vn_set_bic_adapt: part = 2'):
            eng._ck(eng.lib.vn_set_bic_adapt(eng.h, 2, 1, None, None))
        with pytest.raises(VNError, match='error 1: vn_set_bic_adapt: rba gamma'):
            rule, par = 1, [1.5, 0.01, 0, 0, 0, 2, 1, 1, 1, 0]
            import ctypes as C
            eng._ck(eng.lib.vn_set_bic_adapt(eng.h, 1, rule, (C.c_double * 10)(*par), None))
        bad = lambda0(i, 1).copy()
        bad[2] = -1.0
        with pytest.raises(VNError, match=r'error 1: vn_set_bic_adapt: 1 initial lambda\(s\) of the ic part negative or not finite'):
            eng.set_bic_adapt('ic', 'rba', bad)
        om = np.ones(sum(rows(i)), dtype=np.float32)
        om[5] = np.inf
        with pytest.raises(VNError, match=r'error 1: vn_set_bic_weights: 1 weight\(s\) of the bc part negative or not finite'):
            eng.set_bic_weights(om)
        assert eng.bic_parts() == {}                                      # a failed registration keeps what the rows had: nothing
        with pytest.raises(VNError, match='error 3: vn_set_bic_adapt: the ic part has no rows'):
            steady.set_bic_adapt('ic', 'rba')
        steady.set_bic_adapt('bc', 'sa')
        # replacement: static <-> adaptive, per part
        eng.set_bic_weights(np.full(sum(rows(i)), 2.0, dtype=np.float32))
        eng.set_bic_adapt('ic', 'sa')
        assert eng.bic_parts()['bc'] == 'static' and eng.bic_parts()['ic']['rule'] == 'sa'
        assert eng.bic_adapt('ic')['slots'] is not None
        with pytest.raises(VNError, match='error 3: vn_set_bic_adapt_state: the bc part holds static weights'):
            eng.set_bic_adapt_state('bc', np.ones(rows(i)[0], dtype=np.float32))
        with pytest.raises(VNError, match='error 1: vn_get_bic_adapt: the bc part runs no sa rule'):
            import ctypes as C
            buf = np.empty(2 * rows(i)[0], np.float32)
            eng._ck(eng.lib.vn_get_bic_adapt(eng.h, 0, None, None, buf.ctypes.data, None, (C.c_double * 6)()))
        eng.set_bic_adapt('ic', 'rba')
        assert eng.bic_adapt('ic')['slots'] is None
        eng.set_bic_weights(np.ones(sum(rows(i)), dtype=np.float32))      # static again, both parts
        assert eng.bic_parts() == {'bc': 'static', 'ic': 'static'}
    finally:
        eng.close()
        steady.close()


def test_refusals_in_both_orders():
    """An ansatz on the rows, learnt vectors, a batch's own copy of the rows: refused whichever is registered first."""
    i = IDX['n33_21']
    d = inputs(i)
    nB = CASES[i][6]
    A, B = np.zeros(nB, np.float32), np.ones(nB, np.float32)
    nine = [0.0] * 9
    for first in ('weights', 'other'):
        for what in ('ansatz', 'learnt', 'batch_bic'):
            eng = make_engine(i)
            try:
                def other():
                    if what == 'ansatz':
                        eng.set_ansatz_rows('bic', A, B)
                    elif what == 'learnt':
                        eng.set_coef_learn([True] + [False] * 8, nine, None, None, 1e-3)
                    else:
                        eng.set_batch_bic(0, d['biInput'], d['biLabel'])
                if first == 'weights':
                    eng.set_bic_adapt('ic', 'rba')
                    with pytest.raises(VNError, match='error 5: .*next to weights on the BC/IC rows'):
                        other()
                else:
                    other()
                    with pytest.raises(VNError, match='error 5: vn_set_bic_adapt next to'):
                        eng.set_bic_adapt('ic', 'rba')
                    with pytest.raises(VNError, match='error 5: vn_set_bic_weights next to'):
                        eng.set_bic_weights(np.ones(sum(rows(i)), dtype=np.float32))
            finally:
                eng.close()


def test_comm_init_is_refused_on_a_handle_with_weighted_rows():
    """vn_comm_init checks the registration before it touches the collective library: the refusal needs none.  Static and
    adaptive alike; the registration stays in use, and once it is cleared the refusal is gone."""
    from varnet_amd.engine import VN_COMM_ID_BYTES
    i = IDX['n33_21']
    spec = adapt_ref.spec_of('rba')
    eng, ref = make_engine(i, spec=spec), make_engine(i, spec=spec)
    static = make_engine(i)
    try:
        static.set_bic_weights(np.ones(sum(rows(i)), dtype=np.float32))
        for e in (eng, static):
            with pytest.raises(VNError, match='error 5: vn_comm_init next to weights on the BC/IC rows'):
                e.comm_init(0, 1, bytes(VN_COMM_ID_BYTES))
        assert same(run_steps(eng, 2), run_steps(ref, 2))                 # the registration is still there and in use
    finally:
        for e in (eng, ref, static):
            e.close()


def test_row_weights_are_refused_under_a_communicator():
    """A one-rank communicator on this card, then either registration: error 5; clearing is still accepted; after
    vn_comm_destroy the registrations go through."""
    assert VNEngine.comm_available(), 'the one-rank communicator of tests/test_multi_gpu.py needs the collective library'
    i = IDX['n33_21']
    eng = make_engine(i)
    try:
        eng.comm_init(0, 1, VNEngine.comm_unique_id())
        assert eng.comm_size() == (1, 0)
        for rule in RULES:
            with pytest.raises(VNError, match='error 5: vn_set_bic_adapt under a communicator'):
                eng.set_bic_adapt('ic', rule)
        with pytest.raises(VNError, match='error 5: vn_set_bic_weights under a communicator'):
            eng.set_bic_weights(np.ones(sum(rows(i)), dtype=np.float32))
        eng.set_bic_adapt('ic')                                           # clearing is always accepted
        eng.set_bic_weights(None)
        assert eng.bic_parts() == {}
        with pytest.raises(VNError, match='error 3'):
            eng.bic_adapt('ic')                                           # nothing was registered
        eng.comm_destroy()
        eng.set_bic_adapt('ic', 'rba')
        eng.set_bic_weights(np.ones(sum(rows(i)), dtype=np.float32))
        assert eng.bic_parts() == {'bc': 'static', 'ic': 'static'}
    finally:
        eng.close()


def test_refused_routes_and_optimizers():
    i = IDX['n33_21']
    for kernel, xcheck, msg in ((VN_KERNEL_LAYERED, False, 'needs a network of the hand-written kernels'),
                                (VN_KERNEL_FUSED, True, 'is not built for VN_KERNEL_FUSED')):
        eng = make_engine(i, kernel, xcheck=xcheck)
        try:
            with pytest.raises(VNError, match='error 5: vn_set_bic_adapt ' + msg):
                eng.set_bic_adapt('ic', 'rba')
            with pytest.raises(VNError, match='error 5: vn_set_bic_weights ' + msg):
                eng.set_bic_weights(np.ones(sum(rows(i)), dtype=np.float32))
        finally:
            eng.close()
    eng = make_engine(i, optimizer='lbfgs')
    try:
        with pytest.raises(VNError, match='error 5: vn_set_bic_adapt on an L-BFGS engine'):
            eng.set_bic_adapt('ic', 'rba')
        eng.set_bic_weights(np.concatenate([lambda0(i, 0), lambda0(i, 1)]))          # static weights are fine with L-BFGS
        f0 = eng.eval_loss(0)[0][0]
        info = eng.lbfgs_step(0)
        assert info['status'] == 0 and info['f_next'] < f0
        eng.lbfgs_loss64(True)                                            # ... also with the line search on the fp64 objective
        info2 = eng.lbfgs_step(0)
        assert info2['status'] == 0 and info2['f_next'] < info['f_next']
    finally:
        eng.close()


def test_rmsprop_commits_through_the_same_path():
    i = IDX['n33_21']
    spec = adapt_ref.spec_of('rba')
    eng = make_engine(i, spec=spec, optimizer='rmsprop')
    try:
        for s in range(2):
            predict_and_compare(eng, 1, spec, single_update_bar('rba')['bar'], 'rmsprop', {})
        eng.train_step(0)
        assert eng.bic_adapt('ic', arrays=False)['stats']['tau'] == 3.0 and eng.step == 3
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
    """`VarNet(pde, bicAdapt=...)` on a 12 x 10 1D+t grid, row-wise and de-duplicated: train() registers the parts with the rows,
    the state moves once per epoch, bicRowWeights() and trainRes.bicAdaptHist report it, the case file names the rule, and a
    checkpoint restored into a fresh model continues bit for bit."""
    opt = dict(bicAdapt={'ic': {'rule': 'rba', 'eta': 0.05}}, bicWeights={'bc': lambda x, t: 1.0 + t[:, 0]})
    np.random.seed(0)
    vn = _varnet(**opt)
    res = vn.train(str(tmp_path / 'run'), epochNum=40, tol=0.0, saveFreq=10, verbose=False, dedup=dedup)
    try:
        assert vn.dedup_state['on'] == dedup, vn.dedup_state
        w = vn.bicRowWeights()
        assert set(w) == {'bc', 'ic'} and w['ic']['x'].shape[0] == w['ic']['omega'].size == w['ic']['l'].size
        st = w['ic']['stats']
        assert st['tau'] == 40.0 and abs(st['mean'] - 1.0) <= 1e-12 and st['min'] < 1.0 < st['max'] and 0.0 < st['share'] < 1.0
        assert np.allclose(w['bc']['omega'], 1.0 + w['bc']['x'][:, 1], rtol=1e-6) and w['bc']['stats']['tau'] == 0.0
        assert [e for e, _ in res.bicAdaptHist] == [10, 20, 30, 40]
        assert [h['ic']['tau'] for _, h in res.bicAdaptHist] == [10.0, 20.0, 30.0, 40.0]
        case = open(os.path.join(str(tmp_path / 'run'), 'caseData.txt')).read()
        assert 'Weights on the boundary and initial rows: bc: static; ic: rule rba' in case and 'eta = 0.05' in case
        arrays = vn.checkpoint_arrays()
        np.random.seed(0)
        vn2 = _varnet(**opt)
        try:
            td2 = vn2.tData = vn2._build_tdata()
            td2.select_mor(0)
            if dedup:
                td2.enable_dedup()
            vn2.restore_arrays(arrays)
            vn2.engine.set_weights(res.trainWeight)
            w2 = vn2.bicRowWeights(td2)
            assert np.array_equal(w2['ic']['lambda'], w['ic']['lambda']) and np.array_equal(w2['ic']['omega'], w['ic']['omega'])
            assert w2['ic']['stats'] == st and np.array_equal(w2['bc']['omega'], w['bc']['omega'])
            vn.tData.select_mor(0)
            assert same(run_steps(vn.engine, 3), run_steps(vn2.engine, 3))
        finally:
            vn2.engine.close()
    finally:
        vn.engine.close()


def test_through_varnet_loss_lag_is_only_a_readback_schedule(tmp_path):
    """lossLag = 8 against lossLag = 0 with bicAdapt='rba', the stop inside a block: snapshot, rollback and replay carry the state."""
    np.random.seed(0)
    vn = _varnet(bicAdapt='rba')
    probe = np.array(vn.train(str(tmp_path / 'probe'), epochNum=12, tol=0.0, saveFreq=100, verbose=False, lossLag=0).lossAll)
    vn.engine.close()
    stop = 3                                                              # (with the initial rows weighted the loss turns up after a few
    assert probe[stop] < probe[:stop].min()                               # epochs) it falls at first: epoch 4 is the first below tol
    tol = 0.5 * (probe[stop] + probe[:stop].min())
    runs = []
    for lag in (0, 8):
        np.random.seed(0)
        vn = _varnet(bicAdapt='rba')
        res = vn.train(str(tmp_path / ('lag%d' % lag)), epochNum=40, tol=tol, saveFreq=100, verbose=False, lossLag=lag)
        w = vn.bicRowWeights()['ic']
        runs.append([np.array(res.lossAll), vn.engine.get_params(), w['lambda'], w['omega'], np.array(list(w['stats'].values()))])
        assert vn.engine.step == stop + 1 and w['stats']['tau'] == stop + 1.0     # not one step, not one update beyond the stop
        vn.engine.close()
    assert same(runs[0], runs[1])


def test_through_varnet_set_bic_adapt_and_balance(tmp_path):
    """setBicAdapt re-registers from the initial state or clears; a balance probe between the epochs does not move the state."""
    np.random.seed(0)
    vn = _varnet(bicAdapt={'bc': 'sa', 'ic': 'sa'})
    try:
        vn.train(str(tmp_path / 'a'), epochNum=6, tol=0.0, saveFreq=100, verbose=False, balance={'rule': 'gradnorm', 'freq': 2})
        w = vn.bicRowWeights()
        for p in ('bc', 'ic'):
            assert w[p]['stats']['tau'] == 6.0 and abs(w[p]['stats']['mean'] - 1.0) <= 1e-12      # one update per epoch, no more
        vn.setBicAdapt({'ic': {'rule': 'rba', 'normalize': False}})
        w = vn.bicRowWeights()
        assert set(w) == {'ic'} and w['ic']['stats']['tau'] == 0.0 and np.all(w['ic']['lambda'] == 1.0) and np.all(w['ic']['omega'] == 1.0)
        vn.setBicAdapt(None)
        with pytest.raises(ValueError, match='the rows carry no weights'):
            vn.bicRowWeights()
        with pytest.raises(VNError, match='error 3'):
            vn.engine.bic_adapt('ic')
    finally:
        vn.engine.close()
