"""
GPU tier of the learnt weight scales (vn_set_reparam, vn_get_reparam, vn_set_reparam_state, vn_reparam_grad; vn_reparam.hip).

1 factorise and rebuild; 2 the stage alone against the fp64 chain rule on the device's own gradient buffer; 3 (g_V, g_s) end to end
against tests/reparam_ref.py on the fp64 oracle, on the single-launch, two-pass, de-duplicated and generic routes; 4 trajectories
against Joint64 restarted from the device's state at every step, and every named mutant replayed on what the device did; 5 the
bit-for-bit relations of the step's entry points and of the state functions; 6 one test each next to the polynomial terms, causal
weights, an ansatz batch, learnt source amplitudes and the loss evaluations; 7 every refusal.  Every test needs the four entry
points: without them they fail.

Bars: tests/reparam_ref.py (bar, slot_bar) for the step; tests/parity_cases.py (LOSS_RTOL 1e-5, GRAD_RTOL 1e-4 per parameter tensor
with the fp32 conditioning rule of tests/gradcheck.py, each layer's slice of s a tensor of its own) end to end.

The worst figures are written to reparam_parity.json in the directory VN_RECORD_DIR names (default: profile_out/ beside tests/; the
committed copy: profiles/reparam_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import reparam_cases as rc
from tests import reparam_ref as rr
from tests.gradcheck import assert_grad_close
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL
from varnet_amd.engine import VN_KERNEL_AUTO, VN_KERNEL_FUSED16, VN_KERNEL_GENERIC, VN_KERNEL_LAYERED, VNEngine, VNError

pytestmark = pytest.mark.gpu

RECORD = {}
KNAME = {VN_KERNEL_AUTO: 'auto', VN_KERNEL_GENERIC: 'generic'}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'reparam_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def note(tag, **kw):
    rec = RECORD.setdefault(tag, {})
    for key, val in kw.items():
        rec[key] = max(float(val), rec.get(key, 0.0))


def make_engine(i, kernel=VN_KERNEL_AUTO, optimizer='adam', lr=rc.LR, theta=None):
    d_in, dim, widths, act, n_k, q = rc.CASES[i]
    d = rc.inputs(i)
    eng = VNEngine(dim, d_in, widths, True, q, kernel=kernel, activationFun=act, optimizer_name=optimizer, learning_rate=lr)
    eng.set_params(rc.theta(i) if theta is None else theta)
    eng.set_fe_table(d['N1'], d['dNt1'], None)
    eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=n_k, detJ=rc.DETJ)
    eng.set_bic(d['biInput'], d['biLabel'], rc.BDOF, rc.BIDIMVAL)
    eng.set_weights(rc.W)
    return eng


def register(eng, i, k, lr=rc.LR_S):
    mode, per, n = rc.MODES[k]
    eng.set_reparam(mode, per=per, n=n, s_init=rc.scales(i, k), lr=lr)
    return rc.layout(i, k)


def grad_of(eng, batch=0):
    gb = eng.bind_grad_buffer()
    eng.grad(batch)
    torch.cuda.synchronize()
    return gb.cpu().numpy()


def state_of(eng):
    """Everything the joint step moves, as float32 arrays: V, s, theta_eff, m, v, ms, vs, f; and the step counter."""
    buf = np.asarray(eng.export_state(), dtype=np.uint8)
    P = eng.P
    flat = buf[8:].view(np.float32)
    rp = eng.get_reparam()
    return dict(V=rp['V'], s=rp['s'], f=rp['f'], ms=rp['slots'][0].copy(), vs=rp['slots'][1].copy(), theta=flat[:P].copy(),
                m=flat[P:2 * P].copy(), v=flat[2 * P:3 * P].copy(), t=int(buf[:8].view(np.int64)[0]))


def same_state(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ('V', 's', 'f', 'ms', 'vs', 'theta', 'm', 'v')) and a['t'] == b['t']


def ulps(got, want):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)) / rr.ulp32(want)))


# ---- 1. factorise and rebuild ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(rc.MODES)), ids=rc.MODE_IDS)
@pytest.mark.parametrize('i', [1, 3, 6, 7], ids=[rc.IDS[i] for i in (1, 3, 6, 7)])
def test_factorise_and_rebuild(i, k):
    eng = make_engine(i)
    try:
        th0 = eng.get_params()
        lay = register(eng, i, k)
        st = state_of(eng)
        th1 = eng.get_params()
        mode, per, n = rc.MODES[k]
        s0 = rc.scales(i, k)
        assert np.array_equal(st['s'], s0) and not st['ms'].any() and not st['vs'].any() and np.array_equal(th1, st['theta'])
        note('factorise/%s' % rc.MODE_IDS[k], theta_ulps=ulps(th1, th0), f_ulps=ulps(st['f'], lay.f(s0)))
        assert ulps(th1, th0) <= 2.0                                   # one fp32 divide and one multiply
        assert ulps(st['f'], lay.f(s0)) <= 1.0
        assert np.array_equal(th1, lay.spread(st['f']).astype(np.float32) * st['V'])      # theta_eff == fl32(f_dev V_dev)
        assert np.array_equal(st['V'][lay.group < 0], th0[lay.group < 0])
        assert np.any(st['V'] != th0) or np.all(st['f'] == 1.0)
        if mode == 'slope' and n in (1.0, 2.0):                        # n a power of two, s = 1 / n: f == 1 exactly
            eng.set_reparam(mode, per=per, n=n)
            assert np.array_equal(eng.get_params(), th1) and np.all(eng.get_reparam()['f'] == 1.0)
            eng.set_params(th0)
            assert np.array_equal(eng.get_params(), th0)
    finally:
        eng.close()


# ---- 2. the stage alone ---------------------------------------------------------------------------------------------------
def check_stage(eng, lay, g, tag):
    st = state_of(eng)
    gV, gs = eng.reparam_grad()
    assert same_state(st, state_of(eng))                               # the dry form touches no state
    wV, ws = lay.chain(st['V'], st['s'], g[:lay.P])
    asum = lay.fprime(st['s']) * lay.abs_sums(st['V'], g[:lay.P])
    eV = ulps(gV, wV) if np.any(wV) else 0.0
    es = float(np.max((np.abs(gs - ws) - 0.5 * rr.ulp32(ws)) / np.maximum(1e-12 * asum, 1e-300)))
    note(tag, gV_ulps=eV, gs_excess_over_1e_12=max(es, 0.0))
    assert np.all(np.abs(gV - wV) <= rr.ulp32(wV)), (tag, eV)
    assert np.all(np.abs(gs - ws) <= 0.5 * rr.ulp32(ws) + 1e-12 * asum), (tag, es)
    assert np.any(gs != 0.0)
    return gV, gs


STAGE = [(i, VN_KERNEL_AUTO) for i in range(len(rc.CASES))] + [(i, VN_KERNEL_GENERIC) for i in rc.GENERIC_OK]


@pytest.mark.parametrize('i,kernel', STAGE, ids=['%s/%s' % (rc.IDS[i], KNAME[kn]) for i, kn in STAGE])
def test_stage_alone(i, kernel):
    """reparam_grad() against the fp64 chain rule applied to the device's own gradient buffer, V and s: every case of the file and
    every mode on one engine, on the automatic route and on the generic kernels (which take at most six hidden layers)."""
    eng = make_engine(i, kernel)
    try:
        for k in range(len(rc.MODES)):
            lay = register(eng, i, k)
            g = grad_of(eng)
            a = check_stage(eng, lay, g, 'stage/%s/%s/%s' % (rc.IDS[i], rc.MODE_IDS[k], KNAME[kernel]))
            b = eng.reparam_grad()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])         # bitwise repeatable
            eng.set_reparam(None)
            eng.set_params(rc.theta(i))
    finally:
        eng.close()


# ---- 3. end to end --------------------------------------------------------------------------------------------------------
def s_blocks(lay):
    return [('s%d' % (l + 1), sl) for l, sl in enumerate(lay.layer_s) if sl.stop > sl.start]


def check_end_to_end(eng, i, lay, tag):
    d_in, dim, widths = rc.CASES[i][0], rc.CASES[i][1], rc.CASES[i][2]
    st = state_of(eng)
    g = grad_of(eng).astype(np.float64)
    gV, gs = eng.reparam_grad()
    V, s = st['V'].astype(np.float64), st['s'].astype(np.float64)
    ref, wV, ws = rc.autograd_of(i, lay, V, s)
    r32 = {}

    def ref32():
        if not r32:
            r32['V'], r32['s'] = rc.autograd_of(i, lay, st['V'], st['s'], dtype=torch.float32)[1:]
        return r32
    for got, key in zip(g[lay.P:], ('loss', 'BCloss', 'ICloss', 'varLoss')):
        note(tag, **{key: abs(got - ref[key]) / max(abs(ref[key]), 1e-300)})
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, key, got, ref[key])
    rec = assert_grad_close(gV, wV, d_in, widths, GRAD_RTOL, dim=dim, td=True, what=tag + ' g_V', g32=lambda: ref32()['V'])
    note(tag, gV_worst_block=rec['worst_block_err'])
    scale = max(float(np.max(np.abs(ws))), 1e-300)
    for name, sl in s_blocks(lay):
        bs = max(float(np.max(np.abs(ws[sl]))), 1e-7 * scale)
        assert float(np.max(np.abs(ws[sl]))) > 1e-7 * scale, (tag, name, 'the reference discards this tensor of s: change the input')
        err = float(np.max(np.abs(gs[sl] - ws[sl]))) / bs
        note(tag, gs_worst_block=err)
        if err > GRAD_RTOL:
            dev = float(np.max(np.abs(ref32()['s'][sl] - ws[sl]))) / bs
            assert err <= max(GRAD_RTOL, 2.0 * dev), (tag, name, err, dev)


E2E = [(2, 0, VN_KERNEL_AUTO), (2, 3, VN_KERNEL_GENERIC), (4, 0, VN_KERNEL_AUTO), (4, 7, VN_KERNEL_AUTO), (3, 0, VN_KERNEL_AUTO), (3, 8, VN_KERNEL_AUTO),
       (6, 2, VN_KERNEL_AUTO), (6, 0, VN_KERNEL_GENERIC), (1, 4, VN_KERNEL_GENERIC), (7, 0, VN_KERNEL_AUTO), (8, 6, VN_KERNEL_AUTO), (0, 0, VN_KERNEL_AUTO)]


@pytest.mark.parametrize('i,k,kernel', E2E, ids=['%s/%s/%s' % (rc.IDS[i], rc.MODE_IDS[k], KNAME[kn]) for i, k, kn in E2E])
def test_end_to_end(i, k, kernel):
    """(g_V, g_s) of a gradient evaluation at theta_eff against autograd of the fp64 oracle loss through theta_eff(V, s), at the
    device's V and s: the row-wise single launch (q = 4, 6), the two-pass route (q = 216) and the generic kernels."""
    eng = make_engine(i, kernel)
    try:
        lay = register(eng, i, k)
        kp = tuple(eng.kernel_path())
        if kernel == VN_KERNEL_AUTO:
            assert kp == (VN_KERNEL_FUSED16, 1 if rc.CASES[i][5] == 216 else 0)
        check_end_to_end(eng, i, lay, 'e2e/%s/%s/%s' % (rc.IDS[i], rc.MODE_IDS[k], KNAME[kernel]))
    finally:
        eng.close()


@pytest.mark.parametrize('U', [1, 257])
def test_end_to_end_dedup(U):
    """The de-duplicated step: n_k q rows over U unique points."""
    i, k = 2, 0
    d_in, dim, widths, act, n_k, q = rc.CASES[i]
    d = rc.inputs(i)
    n = n_k * q
    rng = np.random.default_rng(40 + U)
    Xu = rng.uniform(-1, 1, (U, d_in)).astype(np.float32)
    uid = (np.arange(n) % U if U <= n else rng.choice(U, n, replace=False)).astype(np.int32)
    order = np.argsort(uid, kind='stable').astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(uid, minlength=U))]).astype(np.int32)
    eng = make_engine(i)
    try:
        eng.set_interior(0, Xu[uid], d['gcoef'], None, n_k=n_k, detJ=rc.DETJ)
        eng.set_dedup(0, Xu, uid, rowptr, order)
        lay = register(eng, i, k)
        st = state_of(eng)
        g = grad_of(eng).astype(np.float64)
        gV, gs = eng.reparam_grad()
        dd = dict(d, Input=Xu[uid])                                    # the reference on the rows Xu[uid]
        ref, wV, ws = rc.autograd_of(i, lay, st['V'].astype(np.float64), st['s'].astype(np.float64), d=dd)
        r32 = lambda: rc.autograd_of(i, lay, st['V'], st['s'], dtype=torch.float32, d=dd)
        assert abs(g[lay.P] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7
        assert_grad_close(gV, wV, d_in, widths, GRAD_RTOL, dim=dim, td=True, what='dedup U=%d g_V' % U, g32=lambda: r32()[1])
        for name, sl in s_blocks(lay):
            bs = float(np.max(np.abs(ws[sl])))
            assert bs > 1e-7 * float(np.max(np.abs(ws)))
            err = float(np.max(np.abs(gs[sl] - ws[sl]))) / bs
            note('e2e/dedup/U%d' % U, gs_worst_block=err)
            if err > GRAD_RTOL:
                assert err <= max(GRAD_RTOL, 2.0 * float(np.max(np.abs(r32()[2][sl] - ws[sl]))) / bs), (name, err)
    finally:
        eng.close()


# ---- 4. trajectories ------------------------------------------------------------------------------------------------------
def run_trajectory(eng, lay, steps=rc.STEPS):
    """Eight steps alternating train_step and grad + apply; the state of before and after every step and the gradient the step
    used (train_step leaves it in the bound buffer)."""
    gb = eng.bind_grad_buffer()
    out = []
    for t in range(1, steps + 1):
        before = state_of(eng)
        if t % 2:
            eng.train_step(0)
        else:
            eng.grad(0)
            eng.apply()
        torch.cuda.synchronize()
        out.append(dict(t=t, before=before, g=gb.cpu().numpy()[:lay.P].copy(), after=state_of(eng)))
    return out


@pytest.mark.parametrize('i,k', rc.TRAJECTORIES, ids=['%s/%s' % (rc.IDS[i], rc.MODE_IDS[k]) for i, k in rc.TRAJECTORIES])
def test_trajectory(i, k):
    eng = make_engine(i)
    try:
        lay = register(eng, i, k)
        traj = run_trajectory(eng, lay)
    finally:
        eng.close()
    tag = 'trajectory/%s/%s' % (rc.IDS[i], rc.MODE_IDS[k])
    ref = rr.Joint64(lay, rc.LR, rc.LR_S)
    steps = []
    for st in traj:
        b, a, t = st['before'], st['after'], st['t']
        assert b['t'] == t - 1 and a['t'] == t
        ref.load(b['m'], b['v'], b['ms'], b['vs'])
        V, s, _ = ref.step(b['V'], b['s'], st['g'], t)
        lr_t, lr_s_t = rr.lr_t_of(rc.LR, t), rr.lr_t_of(rc.LR_S, t)
        eV = float(np.max(np.abs(a['V'] - V) / rr.bar(b['V'], V, lr_t)))
        es = float(np.max(np.abs(a['s'] - s) / rr.bar(b['s'], s, lr_s_t)))
        slots = [float(np.max(np.abs(a[key] - want) / rr.slot_bar(b[key], want, term)))
                 for key, want, term in (('m', ref.m, (1 - ref.b1) * ref.gV), ('v', ref.v, (1 - ref.b2) * ref.gV ** 2),
                                         ('ms', ref.ms, (1 - ref.b1) * ref.gs), ('vs', ref.vs, (1 - ref.b2) * ref.gs ** 2))]
        note(tag, V_over_bar=eV, s_over_bar=es, slots_over_bar=max(slots), f_ulps=ulps(a['f'], lay.f(a['s'])))
        assert eV <= 1.0 and es <= 1.0 and max(slots) <= 1.0, (tag, t, eV, es, slots)
        assert ulps(a['f'], lay.f(a['s'])) <= 1.0
        assert np.array_equal(a['theta'], lay.spread(a['f']).astype(np.float32) * a['V'])       # rebuilt from the values of after
        assert np.any(a['V'] != b['V']) and np.any(a['s'] != b['s'])
        steps.append(dict(t=t, V=b['V'], s=b['s'], g=st['g'], m=b['m'], v=b['v'], ms=b['ms'], vs=b['vs']))
    # every mutant that applies leaves the bar on what the device did (NumPy alone, teacher-forced from the device's states)
    for name in rr.MUTANTS:
        r = rr.replay(name, lay, steps, rc.LR, rc.LR_S)
        if r is not None:
            note(tag, **{'mutant_' + name: r})
            assert r > 1.0, (tag, name, r)


# ---- 5. bit-for-bit relations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i,k', [(4, 0), (3, 8)], ids=['bench_net_rwf', 'ragged_slope_layer'])
def test_step_relations(i, k):
    """train_step == grad + apply; an epoch == its single steps (loss_acc included); snapshot -> 3 steps -> rollback -> the same 3
    steps; two fresh engines give the same bits."""
    a, b = make_engine(i), make_engine(i)
    try:
        register(a, i, k)
        register(b, i, k)
        assert same_state(state_of(a), state_of(b))
        a.state_snapshot()
        acc = torch.zeros(1, device='cuda')
        a.train_epoch((0, 0, 0), acc)
        one, total, gb = torch.zeros(1, device='cuda'), np.float32(0.0), b.bind_grad_buffer()
        for j in range(3):
            if j == 1:
                b.grad(0)
                b.apply()
                loss = gb[b.P].item()
            else:
                b.train_step(0, one)
                loss = one.item()
            total = np.float32(total + np.float32(loss))
        torch.cuda.synchronize()
        sa, sb = state_of(a), state_of(b)
        assert same_state(sa, sb) and sa['t'] == 3
        assert np.float32(acc.item()) == total                         # the epoch's loss sum, added in the same order
        a.state_rollback()
        assert state_of(a)['t'] == 0
        for _ in range(3):
            a.train_step(0)
        assert same_state(state_of(a), sb)
    finally:
        a.close()
        b.close()


def test_export_import_continues_the_trajectory():
    i, k = 2, 3
    a, b = make_engine(i), make_engine(i, theta=np.zeros_like(rc.theta(i)))
    try:
        register(a, i, k)
        for _ in range(3):
            a.train_step(0)
        blob, rp = a.export_state(), a.get_reparam()
        register(b, i, k)
        b.import_state(blob)
        assert ulps(b.get_params(), a.get_params()) <= 2.0             # V re-factorised from the imported theta_eff with b's own s
        assert np.array_equal(b.get_reparam()['s'], rc.scales(i, k))
        b.set_reparam_state(rp['V'], rp['s'], rp['slots'])
        assert same_state(state_of(a), state_of(b))
        for e in (a, b):
            e.train_step(0)
            e.train_step(0)
        assert same_state(state_of(a), state_of(b)) and state_of(a)['t'] == 5
    finally:
        a.close()
        b.close()


def test_clearing_hands_the_slots_back():
    """set_reparam(None) after k steps, then the plain step, against an engine handed the same theta, m, v and step."""
    i, k = 2, 0
    a, b = make_engine(i), make_engine(i)
    try:
        register(a, i, k)
        for _ in range(3):
            a.train_step(0)
        th = a.get_params()
        a.set_reparam(None)
        assert np.array_equal(a.get_params(), th) and a.reparam is None
        with pytest.raises(VNError, match='error 3'):
            a.get_reparam()
        b.import_state(a.export_state())
        for e in (a, b):
            e.train_step(0)
            e.grad(0)
            e.apply()
        assert np.array_equal(np.asarray(a.export_state()), np.asarray(b.export_state())) and a.step == 5
    finally:
        a.close()
        b.close()


def test_params_init_and_set():
    i, k = 3, 0
    a, b = make_engine(i), make_engine(i)
    try:
        lay = register(a, i, k)
        a.train_step(0)
        a.init_params(seed=5)
        b.init_params(seed=5)
        st = state_of(a)
        assert st['t'] == 0 and not st['m'].any() and not st['v'].any() and not st['ms'].any() and not st['vs'].any()
        assert np.array_equal(st['s'], rc.scales(i, k)) and ulps(st['theta'], b.get_params()) <= 2.0
        assert np.array_equal(st['theta'], lay.spread(st['f']).astype(np.float32) * st['V'])
        a.train_step(0)
        slots = state_of(a)
        a.set_params(rc.theta(i))                                      # re-factorised with the current s; the slots stay
        st = state_of(a)
        assert ulps(st['theta'], rc.theta(i)) <= 2.0 and np.array_equal(st['s'], slots['s'])
        assert all(np.array_equal(st[key], slots[key]) for key in ('m', 'v', 'ms', 'vs'))
    finally:
        a.close()
        b.close()


def test_without_a_registration_nothing_changes():
    """An engine whose scales were registered, stepped and cleared, put back to the start: bit for bit the engine that never had
    any, train_step (the update folded into the reduction) included."""
    i = 4
    a, b = make_engine(i), make_engine(i)
    try:
        s0 = b.export_state()
        register(a, i, 0)
        a.train_step(0)
        a.set_reparam(None)
        a.import_state(s0)
        for e in (a, b):
            e.train_step(0)
            e.train_step(0)
        assert np.array_equal(np.asarray(a.export_state()), np.asarray(b.export_state()))
    finally:
        a.close()
        b.close()


# ---- 6. next to the other stages ------------------------------------------------------------------------------------------
def test_with_the_three_polynomial_terms():
    from tests.nldiff_cases import COEF, DIFF, FLUX
    i, k = 2, 0
    n = rc.CASES[i][4] * rc.CASES[i][5]
    rng = np.random.default_rng(24)
    eng = make_engine(i)
    try:
        eng.set_reaction(0, rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32), COEF)
        eng.set_nlflux(0, rng.standard_normal((n, 1)).astype(np.float32), FLUX)
        eng.set_nldiff(0, (8.0 * rng.standard_normal((n, 1))).astype(np.float32), DIFF)
        g_plain = grad_of(eng)
        lay = register(eng, i, k)
        g = grad_of(eng)
        assert not np.array_equal(g, g_plain)                          # evaluated at theta_eff, up to 2 ulp from theta
        assert np.max(np.abs(g - g_plain)) <= 1e-3 * np.max(np.abs(g_plain))
        check_stage(eng, lay, g, 'with/terms')
        eng.train_step(0)
        st = state_of(eng)
        assert np.array_equal(st['theta'], lay.spread(st['f']).astype(np.float32) * st['V']) and st['t'] == 1
    finally:
        eng.close()


def test_with_causal_weights():
    i, k = 2, 3
    n_k = rc.CASES[i][4]
    eng = make_engine(i)
    try:
        eng.set_causal(0, (np.arange(n_k) * 2 // n_k).astype(np.int32), 2, 1e-3)
        lay = register(eng, i, k)
        check_stage(eng, lay, grad_of(eng), 'with/causal')
        a = state_of(eng)
        eng.train_step(0)
        b = state_of(eng)
        assert b['t'] == 1 and np.any(a['s'] != b['s']) and np.array_equal(b['theta'], lay.spread(b['f']).astype(np.float32) * b['V'])
    finally:
        eng.close()


def test_with_an_ansatz_batch():
    i, k = 2, 0
    n = rc.CASES[i][4] * rc.CASES[i][5]
    rng = np.random.default_rng(31)
    eng = make_engine(i)
    try:
        z = lambda m: rng.uniform(0.5, 1.5, m).astype(np.float32)
        eng.set_ansatz(0, A=z(n), B=z(n), a=z(n), b=z(n))
        eng.set_ansatz_rows('bic', A=z(rc.NB), B=z(rc.NB))
        lay = register(eng, i, k)
        check_stage(eng, lay, grad_of(eng), 'with/ansatz')
        eng.train_step(0)
        st = state_of(eng)
        assert st['t'] == 1 and np.array_equal(st['theta'], lay.spread(st['f']).astype(np.float32) * st['V'])
    finally:
        eng.close()


def test_with_learnt_source_amplitudes():
    """Source amplitudes learnt next to the scales: their own Adam step is what it is without the scales, given the same theta_eff."""
    i, k = 2, 0
    d_in, dim, widths, act, n_k, q = rc.CASES[i]
    d = rc.inputs(i)
    n = n_k * q
    rng = np.random.default_rng(33)
    phi = rng.standard_normal((2, n)).astype(np.float32)
    src = rng.standard_normal((n, 1)).astype(np.float32)
    engs = []
    try:
        for with_scales in (True, False):
            eng = VNEngine(dim, d_in, widths, True, q, isSource=True, activationFun=act, learning_rate=rc.LR)
            engs.append(eng)
            eng.set_params(rc.theta(i))
            eng.set_fe_table(d['N1'], d['dNt1'], None)
            eng.set_interior(0, d['Input'], d['gcoef'], src, n_k=n_k, detJ=rc.DETJ)
            eng.set_bic(d['biInput'], d['biLabel'], rc.BDOF, rc.BIDIMVAL)
            eng.set_weights(rc.W)
            eng.set_source_basis(0, phi)
            eng.set_source_learn(mask=[1, 1], init=[0.3, -0.2], lr=1e-2)
        a, b = engs
        register(a, i, k)
        b.set_params(a.get_params())                                   # the same effective parameters
        for j in range(2):
            if j:
                a.grad(0), a.apply(), b.grad(0), b.apply()
            else:
                a.train_step(0), b.train_step(0)
            amp_a, amp_b = a.get_source_amps(), b.get_source_amps()
            assert np.array_equal(amp_a, amp_b) and not np.array_equal(amp_a, [0.3, -0.2])
            b.set_params(a.get_params())
        assert a.step == 2 and np.any(state_of(a)['s'] != rc.scales(i, k))
    finally:
        for e in engs:
            e.close()


def test_loss_evaluations_read_theta_eff():
    i, k = 2, 7
    eng = make_engine(i)
    try:
        lay = register(eng, i, k)
        eng.train_step(0)
        st = state_of(eng)
        ref, gref = rc.oracle_grad(i, st['theta'])
        out, _ = eng.eval_loss(0)
        assert abs(out[0] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7
        out64, g64, _ = eng.objective64(0)
        assert abs(out64[0] - ref['loss']) <= 1e-9 * abs(ref['loss'])
        assert np.max(np.abs(g64.cpu().numpy() - gref)) <= 1e-9 * np.max(np.abs(gref))       # the gradient is w.r.t. theta_eff
        plain = rc.oracle_grad(i, st['V'])[0]['loss']
        assert abs(plain - ref['loss']) > 100 * LOSS_RTOL * abs(ref['loss'])        # V alone is another network
    finally:
        eng.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_argument_checks():
    i = 2
    eng = make_engine(i)
    try:
        S = rc.layout(i, 0).S
        with pytest.raises(VNError, match='error 1.*scales'):
            eng.set_reparam('rwf', s_init=np.zeros(S - 1))
        with pytest.raises(VNError, match='error 1.*not finite'):
            eng.set_reparam('rwf', s_init=np.r_[np.zeros(S - 1), np.nan])
        with pytest.raises(VNError, match='error 1.*not finite'):
            eng.set_reparam('slope', s_init=np.r_[np.ones(59), np.inf])
        with pytest.raises(VNError, match='error 1.*n must be'):
            eng.set_reparam('slope', n=0.5)
        with pytest.raises(VNError, match='error 1.*== 0'):
            eng.set_reparam('slope', per='layer', n=2.0, s_init=[0.5, 0.0, 0.5])
        with pytest.raises(VNError, match='error 1.*learning rate'):
            eng.set_reparam('rwf', lr=-1e-3)
        with pytest.raises(ValueError):
            eng.set_reparam('rfw')
        with pytest.raises(ValueError):
            eng.set_reparam('slope', per='entry')
        assert eng.reparam is None
        for call in (eng.get_reparam, eng.reparam_grad, lambda: eng.set_reparam_state(s=np.zeros(0))):
            with pytest.raises(VNError, match='error 3'):
                call()
        eng.state_snapshot()
        eng.set_reparam('rwf')
        with pytest.raises(VNError, match='error 3'):                 # the registration invalidated the snapshot
            eng.state_rollback()
        with pytest.raises(VNError, match='error 1.*not finite'):
            eng.set_reparam_state(s=np.r_[np.zeros(S - 1), np.nan])
        with pytest.raises(ValueError):
            eng.set_reparam_state(V=np.zeros(3))
        eng.state_snapshot()
        eng.set_reparam(None)
        with pytest.raises(VNError, match='error 3'):                 # ... and so does clearing it
            eng.state_rollback()
        eng.train_step(0)
    finally:
        eng.close()


@pytest.mark.parametrize('optimizer', ['rmsprop', 'lbfgs'])
def test_other_optimizers_are_refused(optimizer):
    eng = make_engine(2, optimizer=optimizer)
    try:
        with pytest.raises(VNError, match='error 5.*theta_eff space'):
            eng.set_reparam('rwf')
        grad_of(eng)
    finally:
        eng.close()


def test_layer_by_layer_route_is_refused():
    d = rc.inputs(2)
    for widths, kernel in (([20, 20, 20], VN_KERNEL_LAYERED), ([128, 128], VN_KERNEL_AUTO), ([20] * 9, VN_KERNEL_AUTO)):
        eng = VNEngine(1, 2, widths, True, 6, kernel=kernel, activationFun='tanh')
        try:
            eng.init_params(seed=1)
            with pytest.raises(VNError, match='error 5.*fused / generic kernels'):
                eng.set_reparam('rwf')
            assert eng.reparam is None
        finally:
            eng.close()


def test_communicator_is_refused_in_either_order():
    if not VNEngine.comm_available():
        pytest.skip('no RCCL library on this machine')
    eng = make_engine(2)
    try:
        uid = VNEngine.comm_unique_id()
        eng.set_reparam('rwf')
        with pytest.raises(VNError, match='error 5.*vn_set_reparam'):
            eng.comm_init(0, 1, uid)
        eng.set_reparam(None)
        eng.comm_init(0, 1, uid)
        with pytest.raises(VNError, match='error 5.*communicator'):
            eng.set_reparam('rwf')
        eng.comm_destroy()
    finally:
        eng.close()
