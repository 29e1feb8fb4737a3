"""
GPU tier of the per-term gradients (vn_term_stats, vn_term_grads; vn_balance.hip).

1. the statistics kernels on synthetic vectors against exactly rounded sums (tests/balance_ref.py);
2. the definition, bit for bit: G_k and value[k] are what grad() leaves under the one-hot weights on a second engine built the
   same way, on every route and next to every kind of row set;
3. G_k against the fp64 oracle under the one-hot weights;  4. linearity against grad() under w = (3, 2, 5);
5. the statistics of the real gradients;  6. the state contract;  7. two batches, in either order;  8. the refusals.
Figures go to profile_out/balance_parity.json (VN_RECORD_DIR overrides the folder); the committed copy is
profiles/balance_parity.json.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import balance_ref
from tests.gradcheck import assert_grad_close, assert_pair_close
from tests.parity_cases import CASES, GRAD_RTOL, LOSS_RTOL, STEADY, oracle_eval, steady_inputs, synth
from varnet_amd.engine import TERMS, VN_KERNEL_AUTO, VN_KERNEL_GENERIC, VNEngine, VNError

pytestmark = pytest.mark.gpu

RECORD = {}
ONE_HOT = {'bc': ((1.0, 0.0, 0.0), 0.0), 'ic': ((0.0, 1.0, 0.0), 0.0), 'var': ((0.0, 0.0, 1.0), 0.0), 'obs': ((0.0, 0.0, 0.0), 1.0)}
W_USER, LAM_USER = np.array([3.0, 2.0, 5.0]), 0.75


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'balance_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def note(tag, **kw):
    rec = RECORD.setdefault(tag, {})
    for key, val in kw.items():
        rec[key] = max(float(val), rec.get(key, 0.0))


# ---- 1. the statistics on synthetic vectors ---------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 255, 256, 257, 4097, 2 ** 20 + 3]
_SYNTH = {}


def synthetic(n):
    """Four fp32 vectors of length n: mixed sizes with zeros, +-1e30 entries and denormals; a second vector whose dot product with
    the first cancels exactly, pair by pair; a plain normal one; a tiny one.  Their exactly rounded statistics
    are computed once."""
    if n not in _SYNTH:
        rng = np.random.default_rng(1000 + n)
        a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
        a[rng.random(n) < 0.1] = 0.0
        idx = rng.integers(0, n, 4)
        a[idx[0]] = np.float32(1e30)
        a[idx[1]] = np.float32(-1e30) if n > 1 else a[idx[1]]
        if n > 4:
            a[idx[2]] = np.float32(1e-42)                            # a denormal
            a[idx[3]] = np.float32(-3e-45)
        b = np.zeros(n, dtype=np.float32)                               # (b_2i, b_2i+1) = (a_2i+1, -a_2i): every pair of products
        m = n // 2 * 2                                                   # cancels exactly, so sum a_p b_p is 0 under large terms
        b[0:m:2], b[1:m:2] = a[1:m:2], -a[0:m:2]
        c = rng.standard_normal(n).astype(np.float32)
        d = (rng.standard_normal(n) * 1e-20).astype(np.float32)
        T = np.ascontiguousarray(np.stack([a, b, c, d]))
        _SYNTH[n] = (T, {K: balance_ref.stats(T[:K]) for K in (1, 2, 4)})
    return _SYNTH[n]


@pytest.fixture(scope='module')
def stats_engine():
    eng = VNEngine(1, 2, [7], True, 4)
    yield eng
    eng.close()


def check_stats(got_stats, got_gram, T, ref, tag):
    st, gram, absgram = ref
    K, n = T.shape
    bar = balance_ref.sum_bar(n)
    assert np.array_equal(got_gram, got_gram.T)
    assert np.array_equal(np.diag(got_gram).view(np.uint64), got_stats[:, 0].copy().view(np.uint64))      # bitwise sumsq
    assert np.array_equal(got_stats[:, 2].copy().view(np.uint64), st[:, 2].copy().view(np.uint64))        # maxabs: bit-exact
    for k in range(K):
        for c, name in ((0, 'sumsq'), (1, 'sumabs')):
            err = abs(got_stats[k, c] - st[k, c]) / st[k, c] if st[k, c] > 0 else abs(got_stats[k, c])
            note(tag, **{name + '_over_bar': err / bar})
            assert err <= bar, (tag, k, name, got_stats[k, c], st[k, c], err, bar)
        for j in range(k + 1, K):
            err = abs(got_gram[k, j] - gram[k, j])
            lim = bar * absgram[k, j]
            note(tag, gram_over_bar=err / lim if lim > 0 else 0.0)
            assert err <= lim, (tag, k, j, got_gram[k, j], gram[k, j], err, lim)


@pytest.mark.parametrize('K', [1, 2, 4])
@pytest.mark.parametrize('n', SIZES)
def test_term_stats_on_synthetic_vectors(stats_engine, n, K):
    T, refs = synthetic(n)
    Td = torch.as_tensor(np.ascontiguousarray(T[:K]), device='cuda')
    r1 = stats_engine.term_stats(Td)
    r2 = stats_engine.term_stats(Td)
    assert r1['stats'].tobytes() == r2['stats'].tobytes() and r1['gram'].tobytes() == r2['gram'].tobytes()     # two calls, the same bits
    check_stats(r1['stats'], r1['gram'], T[:K], refs[K], 'stats/n%d/K%d' % (n, K))
    if K >= 2 and n >= 2:                                                # the pair is built to cancel
        assert refs[K][1][0, 1] == 0.0 and refs[K][2][0, 1] > 0.0


@pytest.mark.parametrize('n', [65, 4097])
def test_a_nan_entry_makes_that_vectors_sumsq_non_finite(stats_engine, n):
    T = synthetic(n)[0].copy()
    T[1, n // 2] = np.nan
    r = stats_engine.term_stats(torch.as_tensor(T, device='cuda'))
    assert not np.isfinite(r['stats'][1, 0]) and not np.isfinite(r['gram'][1, 1]) and not np.isfinite(r['gram'][0, 1])
    assert np.isfinite(r['stats'][[0, 2, 3], 0]).all() and np.isfinite(r['gram'][0, 2])


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _plain(ci, kernel=VN_KERNEL_AUTO, optimizer='adam', n_batches=1, **kw):
    d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec = CASES[ci]
    eng = VNEngine(dim, d_in, widths, True, q, isSource=source, integWflag=integW, kernel=kernel, optimizer_name=optimizer, **kw)
    eng.init_params(seed=3)
    flat = eng.get_params() + 0.05 * np.random.default_rng(5).standard_normal(eng.P).astype(np.float32)
    eng.set_params(flat)
    data = []
    for b in range(n_batches):
        d = synth(1 + b, d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec)
        if b == 0:
            eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
            eng.set_bic(d['biInput'], d['biLabel'], bDof, 2.0)
        else:
            d0 = data[0]
            d.update(N1=d0['N1'], dNt1=d0['dNt1'], integW=d0['integW'], N=d0['N'], dNt=d0['dNt'], biInput=d0['biInput'], biLabel=d0['biLabel'])
        eng.set_interior(b, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=d['detJ'])
        data.append(d)
    eng.set_weights(W_USER)
    eng._case = (CASES[ci], data, flat)
    return eng


def _steady(si):
    d_in, dim, widths, q, n_k, nB, bDof, act, has_w, detJvec = STEADY[si]
    d, flat = steady_inputs(STEADY[si])
    eng = VNEngine(dim, d_in, widths, False, q, isSource=True, integWflag=has_w, activationFun=act)
    eng.set_params(flat)
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, 1.5)
    eng.set_weights(W_USER)
    return eng


def _dedup(U):
    ci = 0
    d_in, dim, widths, q, n_k = CASES[ci][:5]
    eng = _plain(ci)
    d = eng._case[1][0]
    n = n_k * q
    rng = np.random.default_rng(40 + U)
    Xu = rng.uniform(-1, 1, (U, d_in)).astype(np.float32)
    uid = (np.arange(n) % U).astype(np.int32)
    order = np.argsort(uid, kind='stable').astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(uid, minlength=U))]).astype(np.int32)
    eng.set_interior(0, Xu[uid], d['gcoef'], d['source'], n_k=n_k, detJ=d['detJ'])
    eng.set_dedup(0, Xu, uid, rowptr, order)
    return eng


def _edges():
    eng = _plain(0)
    d_in, dim = CASES[0][:2]
    rng = np.random.default_rng(61)
    nrm = rng.standard_normal((17, dim)).astype(np.float32)
    eng.set_flux_bc(rng.uniform(-1, 1, (17, d_in)).astype(np.float32), nrm, rng.uniform(0, 1, 17).astype(np.float32),
                    rng.standard_normal(17).astype(np.float32), 2.0)
    eng.set_periodic(rng.uniform(-1, 1, (22, d_in)).astype(np.float32), rng.standard_normal((22, dim)).astype(np.float32), 1.0, 2.0)
    return eng


def _obs():
    eng = _plain(0)
    rng = np.random.default_rng(62)
    eng.set_observations(rng.uniform(-1, 1, (33, CASES[0][0])).astype(np.float32), rng.standard_normal(33).astype(np.float32),
                         weight=LAM_USER)
    return eng


def _reaction_causal():
    eng = _plain(0)
    q, n_k = CASES[0][3:5]
    rng = np.random.default_rng(63)
    eng.set_reaction(0, rng.uniform(0.5, 2.0, (n_k * q, 1)).astype(np.float32), [0.7, -0.3, 0.2])
    eng.set_causal(0, (np.arange(n_k) * 4 // n_k).astype(np.int32), 4, 1e-3)
    return eng


BUILD = {
    'P29_one_block': lambda: _plain(4),                             # (2,1,[7],36,...): P = 29, below one reduction block
    '1x20_300': lambda: _plain(19),                                 # (2,1,[20],16,300,...)
    '5x50': lambda: _plain(1),                                      # (3,2,[50]*5,64,9,...): several reduction blocks
    'two_pass': lambda: _plain(12),                                 # (3,2,[50,50,50],216,7,...)
    'generic': lambda: _plain(0, kernel=VN_KERNEL_GENERIC),
    'steady': lambda: _steady(1),                                   # no IC rows: that row is zeros
    'layered_128x128': lambda: _steady(12),
    'dedup_U1': lambda: _dedup(1),
    'dedup_U257': lambda: _dedup(257),
    'flux_periodic': _edges,                                        # folded into BC
    'observations': _obs,                                           # K = 4
    'reaction_causal': _reaction_causal,
}
HAS_IC = {name: name not in ('steady', 'layered_128x128') for name in BUILD}
_PROBES = {}


def probe(name):
    """One probe with the gradients per case, shared by the tests below and left unchanged: (result with 'G' on the host)."""
    if name not in _PROBES:
        eng = BUILD[name]()
        try:
            r = eng.term_grads((0,), grads=True)
            r['G'] = r['G'].cpu().numpy()
            r['P'] = eng.P
        finally:
            eng.close()
        _PROBES[name] = r
    return _PROBES[name]


def grad_of(eng, batch=0):
    gb = eng.bind_grad_buffer()
    eng.grad(batch)
    torch.cuda.synchronize()
    return gb.cpu().numpy().copy()


def one_hot_grad(eng, term, has_obs, batch=0):
    w, lam = ONE_HOT[term]
    eng.set_weights(w)
    if has_obs:
        eng.set_obs_weight(lam)
    g = grad_of(eng, batch)
    val = g[eng.P + 1 + TERMS.index(term)] if term != 'obs' else eng.obs_misfit()
    return g[:eng.P], val


# ---- 2. the definition, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(BUILD))
def test_definition_bit_for_bit(name):
    r = probe(name)
    twin = BUILD[name]()
    try:
        for k, term in enumerate(TERMS):
            present = (term != 'ic' or HAS_IC[name]) and (term != 'obs' or name == 'observations')
            if not present:
                assert not r['G'][k].any() and r['value'][k] == 0.0 and r['sumsq'][k] == 0.0 and not r['gram'][k].any()
                continue
            g, val = one_hot_grad(twin, term, name == 'observations')
            assert np.array_equal(r['G'][k].view(np.uint32), g.view(np.uint32)), (name, term)
            assert r['value'][k] == float(val), (name, term, r['value'][k], val)
            assert g.any(), (name, term)
    finally:
        twin.close()


# ---- 3. the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,ci', [('P29_one_block', 4), ('1x20_300', 19), ('5x50', 1), ('two_pass', 12)])
def test_per_term_gradients_against_the_oracle(name, ci):
    r = probe(name)
    d_in, dim, widths, q, n_k, nB, bDof, source, integW, detJvec = CASES[ci]
    eng = BUILD[name]()
    _, data, flat = eng._case
    eng.close()
    for k, term in enumerate(TERMS[:3]):
        d = dict(data[0], w=np.array(ONE_HOT[term][0]))
        ref, gref = oracle_eval(flat, d, d_in, dim, widths, q, n_k, bDof, source, integW, detJvec)
        rec = {}
        assert_grad_close(r['G'][k], gref, d_in, widths, GRAD_RTOL, dim=dim, rec=rec, what='%s G_%s' % (name, term),
                          g32=lambda: oracle_eval(flat, d, d_in, dim, widths, q, n_k, bDof, source, integW, detJvec, dtype=torch.float32)[1])
        want = ref[('BCloss', 'ICloss', 'varLoss')[k]]
        verr = abs(r['value'][k] - want) / abs(want)
        note('oracle/%s/%s' % (name, term), grad_global=rec['grad_global'], worst_block=rec['worst_block_err'], value=verr)
        assert verr <= LOSS_RTOL, (name, term, r['value'][k], want)


# ---- 4. linearity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['P29_one_block', '5x50', 'two_pass', 'generic', 'dedup_U257', 'flux_periodic', 'observations'])
def test_weighted_sum_of_the_terms_is_the_gradient(name):
    r = probe(name)
    eng = BUILD[name]()
    try:
        g = grad_of(eng)[:eng.P]                                        # under w = (3, 2, 5) (and lambda = 0.75)
        case = getattr(eng, '_case')[0]
    finally:
        eng.close()
    w4 = np.array(list(W_USER) + [LAM_USER if name == 'observations' else 0.0])
    comb = (w4[:, None] * r['G'].astype(np.float64)).sum(axis=0)
    d_in, dim, widths = case[0], case[1], case[2]
    rec = {}
    assert_pair_close(comb, g, d_in, widths, GRAD_RTOL, dim=dim, rec=rec, what='%s sum_k w_k G_k' % name)
    note('linearity/' + name, grad_global=rec['grad_global'], worst_block=rec['worst_block_err'])


# ---- 5. the statistics of the real gradients ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(BUILD))
def test_statistics_of_the_real_gradients(name):
    r = probe(name)
    G = np.ascontiguousarray(r['G'])
    ref = balance_ref.stats(G)
    stats = np.stack([r['sumsq'], r['sumabs'], r['max_abs']], axis=1)
    check_stats(stats, r['gram'], G, ref, 'real/' + name)
    np.testing.assert_array_equal(r['norm2'], np.sqrt(r['sumsq']))
    np.testing.assert_array_equal(r['mean_abs'], r['sumabs'] / r['P'])


# ---- 6. the state contract ----------------------------------------------------------------------------------------------------
def state_bytes(eng):
    return np.asarray(eng.export_state(), dtype=np.uint8).tobytes()


@pytest.mark.parametrize('name', ['1x20_300', 'two_pass', 'observations', 'dedup_U257'])
def test_a_probe_leaves_the_state_and_the_weights_alone(name):
    a, b = BUILD[name](), BUILD[name]()
    try:
        acc = torch.zeros(1, device='cuda')
        a.train_epoch((0,), acc)
        b.train_epoch((0,), torch.zeros(1, device='cuda'))
        torch.cuda.synchronize()
        before = (state_bytes(a), a.get_params().tobytes(), a.step, acc.item())
        a.term_grads((0,))
        after = (state_bytes(a), a.get_params().tobytes(), a.step, acc.item())
        assert before == after and a.step == 1
        ga, gb_ = grad_of(a), grad_of(b)                                 # the weights: the loss scalars of a grad match the twin's
        assert np.array_equal(ga.view(np.uint32), gb_.view(np.uint32))
        for _ in range(3):
            a.train_step(0), b.train_step(0)
        torch.cuda.synchronize()
        assert state_bytes(a) == state_bytes(b) and a.step == b.step == 4
    finally:
        a.close(), b.close()


def test_probe_then_steps_with_learnt_weight_scales():
    engs = []
    try:
        for _ in range(2):
            eng = _plain(0)
            rng = np.random.default_rng(9)
            eng.set_reparam('rwf', s_init=rng.normal(0.0, 0.1, sum(CASES[0][2]) + 1), lr=2e-3)
            engs.append(eng)
        a, b = engs
        ra0 = a.get_reparam()
        r = a.term_grads((0,), grads=True)
        ra1 = a.get_reparam()
        assert all(np.array_equal(ra0[key], ra1[key]) for key in ('V', 's', 'f', 'slots'))
        b.set_weights(ONE_HOT['var'][0])
        twin_g = grad_of(b)[:b.P]
        b.set_weights(W_USER)
        assert np.array_equal(r['G'][2].cpu().numpy().view(np.uint32), twin_g.view(np.uint32))      # with respect to theta_eff
        for _ in range(3):
            a.train_step(0), b.train_step(0)
        torch.cuda.synchronize()
        assert state_bytes(a) == state_bytes(b) and a.step == 3
        fa, fb = a.get_reparam(), b.get_reparam()
        assert all(np.array_equal(fa[key], fb[key]) for key in ('V', 's', 'f', 'slots'))
        assert not np.array_equal(fa['s'], ra0['s'])
    finally:
        for e in engs:
            e.close()


def test_probe_then_steps_with_learnt_source_amplitudes():
    ci = 2                                                               # (3,2,[10,20],64,5,...) with a source
    q, n_k = CASES[ci][3:5]
    rng = np.random.default_rng(33)
    phi = rng.standard_normal((2, n_k * q)).astype(np.float32)
    engs = []
    try:
        for _ in range(2):
            eng = _plain(ci)
            eng.set_source_basis(0, phi)
            eng.set_source_learn(mask=[1, 1], init=[0.3, -0.2], lr=1e-2)
            engs.append(eng)
        a, b = engs
        a.train_step(0), b.train_step(0)
        amps = a.get_source_amps().copy()
        a.term_grads((0,))
        assert np.array_equal(a.get_source_amps(), amps) and a.step == 1
        for _ in range(3):
            a.train_step(0), b.train_step(0)
        torch.cuda.synchronize()
        assert np.array_equal(a.get_source_amps(), b.get_source_amps()) and not np.array_equal(a.get_source_amps(), amps)
        assert state_bytes(a) == state_bytes(b)
    finally:
        for e in engs:
            e.close()


def test_snapshot_probe_steps_rollback_replay():
    eng = _plain(19)
    try:
        eng.train_step(0)
        eng.state_snapshot()
        eng.term_grads((0,))
        eng.train_step(0), eng.train_step(0)
        torch.cuda.synchronize()
        first = state_bytes(eng)
        eng.state_rollback()
        assert eng.step == 1
        eng.train_step(0), eng.train_step(0)
        torch.cuda.synchronize()
        assert state_bytes(eng) == first and eng.step == 3
    finally:
        eng.close()


# ---- 7. two batches -----------------------------------------------------------------------------------------------------------
def test_two_batches_sum_in_list_order():
    eng = _plain(0, n_batches=2)
    try:
        r0 = eng.term_grads((0,), grads=True)
        G0, v0 = r0['G'].cpu().numpy(), r0['value'].copy()
        r1 = eng.term_grads((1,), grads=True)
        G1, v1 = r1['G'].cpu().numpy(), r1['value'].copy()
        r01 = eng.term_grads((0, 1), grads=True)
        r10 = eng.term_grads((1, 0), grads=True)
        assert not np.array_equal(G0[2], G1[2])
        assert np.array_equal(r01['G'].cpu().numpy().view(np.uint32), (G0 + G1).astype(np.float32).view(np.uint32))
        assert np.array_equal(r10['G'].cpu().numpy().view(np.uint32), (G1 + G0).astype(np.float32).view(np.uint32))
        np.testing.assert_array_equal(r01['value'], v0 + v1)
        np.testing.assert_array_equal(r10['value'], v1 + v0)
        # three batches in the order given: ((G1 + G0) + G1), one rounding per add
        r101 = eng.term_grads((1, 0, 1), grads=True)
        want = ((G1 + G0).astype(np.float32) + G1).astype(np.float32)
        assert np.array_equal(r101['G'].cpu().numpy().view(np.uint32), want.view(np.uint32))
    finally:
        eng.close()


def test_term_mask_selects_the_terms():
    eng = _plain(19)
    try:
        full = eng.term_grads((0,), grads=True)
        part = eng.term_grads((0,), terms=('bc', 'var'), grads=True)
        Gf, Gp = full['G'].cpu().numpy(), part['G'].cpu().numpy()
        assert np.array_equal(Gf[[0, 2]], Gp[[0, 2]]) and not Gp[1].any() and not Gp[3].any()
        assert part['value'][1] == 0.0 and part['sumsq'][1] == 0.0 and not part['gram'][1].any() and not part['gram'][:, 1].any()
        assert part['gram'][0, 2] == full['gram'][0, 2] and part['sumsq'][0] == full['sumsq'][0]
    finally:
        eng.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    lb = _plain(0, optimizer='lbfgs')
    try:
        with pytest.raises(VNError, match='error 5: vn_term_grads on an L-BFGS engine'):
            lb.term_grads((0,))
    finally:
        lb.close()
    eng = _plain(0)
    try:
        for mask in (0, 1 << 4, 0x1f):
            with pytest.raises(VNError, match='error 1: vn_term_grads: term_mask'):
                eng.term_grads((0,), terms=mask)
        for bad in ((1,), (-1,), (0, 7)):
            with pytest.raises(VNError, match='error 1: vn_term_grads: batches'):
                eng.term_grads(bad)
        with pytest.raises(VNError, match='error 1: vn_term_grads: the batch list is null or empty'):
            eng.term_grads(())
        with pytest.raises(ValueError, match='unknown term'):
            eng.term_grads((0,), terms=('bc', 'flux'))
        g0 = grad_of(eng)                                                # every refusal left the weights alone
        T = torch.zeros((5, 8), device='cuda')
        with pytest.raises(VNError, match=r'error 1: vn_term_stats: K = 5 is outside 1\.\.4'):
            eng.term_stats(T)
        with pytest.raises(VNError, match='error 1: vn_term_stats: n = 0 must be at least 1'):
            eng.term_stats(torch.zeros((2, 0), device='cuda'))
        with pytest.raises(VNError, match='error 1: vn_term_stats: null argument'):
            eng.term_stats(None)
        assert np.array_equal(grad_of(eng), g0)
    finally:
        eng.close()
