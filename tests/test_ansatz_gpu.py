"""
GPU tier of the hard-constraint ansatz u = A + B n (vn_set_ansatz, vn_set_ansatz_points, vn_set_ansatz_rows; vn_ansatz.hip).

Parity of the loss components, the loss field and the gradient against the fp64 restatement (tests/ansatz_ref.py) on the
automatic route (single-launch 8-wave -> two-pass sequence, two-pass) and on the generic kernels, on the BC/IC rows, on every
edge set (flux rows, pairs with gamma = 0 and 1, observations without and with directions and a rowptr), on the de-duplicated
step, together with the polynomial terms and the loss weights; the composition of the step's entry points; exactness of the
BC/IC components at B = 0, A = label; the registration contract, every refusal and the all-or-nothing rule.  Every test here
needs the three entry points: without them they fail.

Bars are those of tests/test_nldiff_gpu.py, taken over unchanged (tests/parity_cases.py: LOSS_RTOL 1e-5, LVEC_RTOL 1e-4,
GRAD_RTOL 1e-4 per parameter tensor through tests/gradcheck.assert_grad_close with its fp32 conditioning callback).  That the
streams make a missing A or B fail is asserted on the CPU (tests/test_ansatz_host.py).

The worst errors per case and route are written to ansatz_parity.json in the directory VN_RECORD_DIR names (default:
profile_out/ beside tests/; the committed copy: profiles/ansatz_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import ansatz_cases as ac
from tests.ansatz_cases import CASES, IDS
from tests.gradcheck import assert_grad_close, assert_pair_close, block_errors, fp32_deviation
from tests.nldiff_cases import COEF, DIFF, FLUX
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL
from varnet_amd.engine import VN_KERNEL_AUTO, VN_KERNEL_FUSED, VN_KERNEL_GENERIC, VN_KERNEL_LAYERED, VNEngine, VNError

pytestmark = pytest.mark.gpu

KEYS = ['loss', 'BCloss', 'ICloss', 'varLoss']
RECORD = {}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'ansatz_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def make_engine(i, kernel=VN_KERNEL_AUTO, az='default', optimizer='adam', xcheck=False):
    """CASES[i] with its default ansatz on the interior and the BC/IC rows (az None: no ansatz)."""
    d_in, dim, widths, q, n_k, nB, bDof, td, act, source, integW = CASES[i]
    d = ac.inputs(i)
    eng = VNEngine(dim, d_in, widths, td, q, isSource=source, integWflag=integW, kernel=kernel, activationFun=act,
                   optimizer_name=optimizer, xcheck=xcheck)
    eng.set_params(ac.theta(i))
    eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
    eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], bDof, ac.BIDIMVAL)
    eng.set_weights(d['w'])
    if az is not None:
        register_ansatz(eng, ac.ansatz(i) if isinstance(az, str) else az)
    return eng


def register_ansatz(eng, az, batch=0):
    eng.set_ansatz(batch, **az['int'])
    eng.set_ansatz_rows('bic', **az['bic'])
    for name in ('flux', 'periodic', 'obs'):
        if az.get(name) is not None:
            eng.set_ansatz_rows(name, **az[name])


def grad_of(eng, batch=0):
    gb = eng.bind_grad_buffer()
    eng.grad(batch)
    torch.cuda.synchronize()
    return gb.cpu().numpy().astype(np.float64)


def check_parity(net, eng, ref, tag, g32, keys=KEYS):
    """eval_loss (with lossVec) and grad of batch 0 against the reference (ref, gref); prints and records every figure, then
    asserts.  net = (d_in, dim, widths, td)."""
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
    print('ansatz %s: %s' % (tag, json.dumps(rec, sort_keys=True)))
    assert np.all(np.isfinite(g))
    for got, key in zip(out, KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'eval', key, got, ref[key])
    for got, key in zip(g[P:], KEYS):
        assert abs(got - ref[key]) <= LOSS_RTOL * abs(ref[key]) + 1e-7, (tag, 'grad', key, got, ref[key])
    assert rec['lossVec'] <= LVEC_RTOL, (tag, rec['lossVec'])
    assert_grad_close(g[:P], gref, d_in, widths, GRAD_RTOL, dim=dim, td=td, what=tag, g32=g32)
    return g


def net_of(i):
    return CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][7]


# ---- interior and BC/IC rows on both routes ---------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_parity(i, kernel):
    """Every case on the automatic route and on the generic kernels; two grad calls return the same bits; both forms of
    vn_eval_loss agree."""
    eng = make_engine(i, kernel)
    try:
        g32 = lambda: ac.reference(i, dtype=torch.float32)[1]
        g1 = check_parity(net_of(i), eng, ac.reference64(i), '%s/%s' % (IDS[i], 'auto' if kernel == VN_KERNEL_AUTO else 'generic'), g32)
        assert np.array_equal(g1, grad_of(eng))
        assert eng.eval_loss(0)[0] == eng.eval_loss(0, lossVec=True)[0]
    finally:
        eng.close()


def test_routes_of_the_cases():
    """What the cases run on: the single-launch 8-wave route (whose ansatz batches take the two-pass sequence) and the two-pass
    route; 1028 rows fill two 256-thread blocks of the four-row kernels with a partial last one, 18 rows are no multiple of four."""
    from varnet_amd.engine import VN_KERNEL_FUSED16
    for i, kp in {0: (VN_KERNEL_FUSED16, 0), 1: (VN_KERNEL_FUSED16, 0), 2: (VN_KERNEL_FUSED16, 0), 3: (VN_KERNEL_FUSED16, 0),
                  4: (VN_KERNEL_FUSED16, 1)}.items():
        eng = make_engine(i, az=None)
        try:
            assert tuple(eng.kernel_path()) == kp, (IDS[i], eng.kernel_path())
        finally:
            eng.close()
    rows = [c[3] * c[4] for c in CASES]
    assert rows[:4] == [4, 18, 1028, 1028] and 256 < 1028 // 4 < 512 and 18 % 4 and sorted({c[5] for c in CASES}) == [1, 33, 257]


@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
def test_streams_off_the_16_byte_grid_take_the_one_row_kernels(kernel):
    """1028 rows with each stream in turn, and all of them, registered from a view one float off the 16-byte grid: the result is
    that of the aligned registration at the bars (the one-row kernels spell the same fmaf chain: bit for bit)."""
    i = 2
    az = ac.ansatz(i)
    eng = make_engine(i, kernel)
    try:
        g0 = grad_of(eng)
        for which in ('A', 'B', 'a', 'b', 'all'):
            dev = {}
            for k, v in az['int'].items():
                off = 1 if which in (k, 'all') else 0
                buf = torch.zeros(v.size + 4, device='cuda')
                base = (-buf.data_ptr() // 4) % 4                       # first element of buf on the 16-byte grid
                view = buf[base + off:base + off + v.size]
                view.copy_(torch.as_tensor(v, device='cuda'))
                assert (view.data_ptr() % 16 == 0) == (off == 0)
                dev[k] = view
            eng.set_ansatz(0, **dev)
            g = check_parity(net_of(i), eng, ac.reference64(i), '%s/%s/off_grid_%s' % (IDS[i], 'auto' if kernel == VN_KERNEL_AUTO else 'generic', which),
                             lambda: ac.reference(i, dtype=torch.float32)[1])
            assert np.array_equal(g, g0), which
    finally:
        eng.close()


# ---- the edge sets ----------------------------------------------------------------------------------------------------
def register_edge(eng, name, reg):
    if name == 'flux':
        eng.set_flux_bc(reg['X'], reg['normal'], reg['coef'], reg['label'], ac.BIDIMVAL)
    elif name == 'periodic':
        eng.set_periodic(reg['X'], reg['dir'], reg['gamma'], ac.BIDIMVAL)
    else:
        eng.set_observations(reg['X'], reg['value'], q=reg.get('q'), dir=reg.get('dir'), rowptr=reg.get('rowptr'), wgt=reg.get('wgt'),
                             weight=reg['lam'])


@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('rows', ac.EDGE_ROWS)
@pytest.mark.parametrize('kind', ac.EDGE_KINDS)
def test_edge_sets(kind, rows, kernel):
    """One edge set of 1, 33, 257 or 600 rows next to the batch, all under the ansatz."""
    i = ac.EDGE_CASE
    name, reg, z = ac.edge(kind, rows)
    az = dict(ac.ansatz(i), **{name: z})
    eng = make_engine(i, kernel, az=None)
    try:
        register_edge(eng, name, reg)
        register_ansatz(eng, az)
        ref = ac.reference(i, az, **{name: reg})
        g32 = lambda: ac.reference(i, az, dtype=torch.float32, **{name: reg})[1]
        check_parity(net_of(i), eng, ref, 'edge/%s/%d/%s' % (kind, rows, 'auto' if kernel == VN_KERNEL_AUTO else 'generic'), g32)
        if name == 'obs':
            assert abs(eng.obs_misfit() - ref[0]['obs']) <= LOSS_RTOL * abs(ref[0]['obs']) + 1e-7
    finally:
        eng.close()


# ---- the de-duplicated step -------------------------------------------------------------------------------------------
def make_dedup_engine(j):
    U, dim, d_in, widths, q, n_k, act = ac.DEDUP[j]
    d = ac.dedup_inputs(j)
    eng = VNEngine(dim, d_in, widths, True, q, activationFun=act)
    eng.set_params(d['theta'])
    eng.set_fe_table(d['N1'], d['dNt1'], None)
    eng.set_interior(0, d['Input'], d['gcoef'], None, n_k=n_k, detJ=ac.DEDUP_DETJ)
    eng.set_bic(d['biInput'], d['biLabel'], ac.DEDUP_BDOF, ac.BIDIMVAL)
    eng.set_weights(d['w'])
    eng.set_ansatz(0, **d['rows32'])
    eng.set_ansatz_rows('bic', **d['bic'])
    return eng, d


@pytest.mark.parametrize('j', range(len(ac.DEDUP)), ids=ac.DEDUP_IDS)
def test_dedup(j):
    """U in {1, 255, 256, 257}, dim in {1, 2, 3}, a map in which some points own no row: the de-duplicated step against the
    reference on Xu[uid] (grad and both forms of vn_eval_loss) and against the row-wise step of the same batch."""
    U, dim, d_in, widths, q, n_k, act = ac.DEDUP[j]
    net = (d_in, dim, widths, True)
    eng, d = make_dedup_engine(j)
    try:
        assert U == 1 or d['empty'] > 0
        ref = ac.dedup_reference(j)
        g32 = lambda: ac.dedup_reference(j, torch.float32)[1]
        g_row = check_parity(net, eng, ref, 'dedup/%s/rowwise' % ac.DEDUP_IDS[j], g32)
        eng.set_dedup(0, d['Xu'], d['uid'], d['rowptr'], d['rowidx'])
        with pytest.raises(VNError, match='error 3.*vn_set_ansatz_points'):     # a map and an ansatz but no point streams
            eng.grad(0)
        eng.set_ansatz_points(0, d['pts']['A'], d['pts']['B'], d['pts']['gA'], d['pts']['gB'])
        g1 = check_parity(net, eng, ref, 'dedup/%s/dedup' % ac.DEDUP_IDS[j], g32)
        assert np.array_equal(g1, grad_of(eng))
        assert not np.array_equal(g1, g_row)                           # another formulation ran
        dev32 = lambda: fp32_deviation(g32(), ref[1], d_in, widths, dim)
        RECORD['dedup/%s/vs_rowwise' % ac.DEDUP_IDS[j]] = assert_pair_close(g1, g_row, d_in, widths, GRAD_RTOL, dim=dim, dev32=dev32,
                                                                            what='dedup vs row-wise')
        eng.set_dedup(0, d['Xu'], d['uid'], d['rowptr'], d['rowidx'])  # a new map drops the point streams
        with pytest.raises(VNError, match='error 3'):
            eng.eval_loss(0)
    finally:
        eng.close()


# ---- together with the terms, the weights and the other sets ------------------------------------------------------------
def terms_of(i):
    n = CASES[i][3] * CASES[i][4]
    rng = np.random.default_rng(24)
    psi = (8.0 * rng.standard_normal((n, 1))).astype(np.float32)
    phi = rng.standard_normal((n, 1)).astype(np.float32)
    rate = rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    return dict(nldiff=(psi, DIFF), nlflux=(phi, FLUX), reaction=(rate, COEF))


@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
def test_with_the_three_polynomial_terms(kernel):
    """The ansatz with D(u) + psi + flux + reaction together: the terms read the transformed u, ud."""
    i = 3
    t = terms_of(i)
    eng = make_engine(i, kernel)
    try:
        eng.set_reaction(0, *t['reaction'])
        eng.set_nlflux(0, *t['nlflux'])
        eng.set_nldiff(0, *t['nldiff'])
        cast = lambda f: {k: (v[0].astype(f), v[1]) for k, v in t.items()}
        ref = ac.reference(i, **cast(np.float64))
        g32 = lambda: ac.reference(i, dtype=torch.float32, **cast(np.float32))[1]
        check_parity(net_of(i), eng, ref, '%s/terms/%s' % (IDS[i], 'auto' if kernel == VN_KERNEL_AUTO else 'generic'), g32)
        none = ac.reference64(i)[0]
        assert abs(ref[0]['varLoss'] - none['varLoss']) > 100 * LOSS_RTOL * abs(none['varLoss'])     # the terms are in play
    finally:
        eng.close()


def test_with_causal_weights():
    """Causal time-slab weights next to the ansatz: the weights are formed from the loss field of the transformed solution and
    scale the seeds before the adjoint stage.  Reference: tests/causal_ref.weighted on the ansatz loss field and the gradient
    of sum_k omega_k lossVec[k] with omega held constant."""
    from tests import ansatz_ref
    from oracle import tf1_graph as og
    from tests.causal_ref import causal_weights
    i = 2
    d_in, dim, widths, q, n_k, nB, bDof, td, act, source, integW = CASES[i]
    slab = (np.arange(n_k) * 4 // n_k).astype(np.int32)
    eps = 1e-3
    ref0, _ = ac.reference64(i)
    lv = np.asarray(ref0['lossVec'], dtype=np.float64).reshape(-1)
    omega, omega_s = causal_weights(lv, slab, 4, eps)

    def weighted(dtype):
        f = np.float64 if dtype == torch.float64 else np.float32
        params = og.unflatten(ac.theta(i).astype(f), d_in, widths, dtype=dtype, requires_grad=True)
        kw = {k: (torch.as_tensor(v, dtype=dtype) if isinstance(v, np.ndarray) else v) for k, v in ac.ref_kw(i, dtype).items()}
        az = ac.cast(ac.ansatz(i), f)
        out = ansatz_ref.loss_fun(params, ansatz=ansatz_ref.streams(az['int'], dtype), ansatz_bic=ansatz_ref.streams(az['bic'], dtype), **kw)
        var = (torch.as_tensor(omega, dtype=dtype) * out['lossVec'][:, 0]).sum()
        w = kw['w']
        loss = w[0] * out['BCloss'] + w[1] * out['ICloss'] + w[2] * var
        loss.backward()
        res = dict(loss=float(loss.detach()), BCloss=float(out['BCloss'].detach()), ICloss=float(out['ICloss'].detach()), varLoss=float(var.detach()),
                   lossVec=out['lossVec'].detach().numpy())
        return res, og.flatten_grads(params).detach().numpy()

    eng = make_engine(i)
    try:
        eng.set_causal(0, slab, 4, eps)
        w_dev = eng.causal_weights(0)
        assert np.max(np.abs(w_dev - omega_s)) <= 1e-5 and omega_s.min() < 0.99     # the weights are in play
        check_parity(net_of(i), eng, weighted(torch.float64), '%s/causal' % IDS[i], lambda: weighted(torch.float32)[1])
    finally:
        eng.close()


def test_with_flux_pairs_and_observations_together():
    """fluxBC, periodic pairs and observations registered at once next to the batch, all under the ansatz."""
    i = ac.EDGE_CASE
    sets, az = {}, dict(ac.ansatz(i))
    for kind, rows in (('flux', 33), ('periodic_g1', 33), ('obs_dirs_rowptr', 33)):
        name, reg, z = ac.edge(kind, rows)
        sets[name], az[name] = reg, z
    eng = make_engine(i, az=None)
    try:
        for name, reg in sets.items():
            register_edge(eng, name, reg)
        register_ansatz(eng, az)
        check_parity(net_of(i), eng, ac.reference(i, az, **sets), 'edge/all_three', lambda: ac.reference(i, az, dtype=torch.float32, **sets)[1])
    finally:
        eng.close()


# ---- the step's entry points ------------------------------------------------------------------------------------------
def _theta_after(eng, state, fn):
    eng.import_state(state)
    fn()
    torch.cuda.synchronize()
    return eng.get_params()


def test_train_step_is_grad_plus_apply():
    """train_step folds the update into the gradient reduction; grad + apply runs it as its own kernel.  Their relation is
    measured first without the ansatz, then required to hold with it (tests/test_nldiff_gpu.py measures it the same way)."""
    i = 3
    eng = make_engine(i, az=None)
    try:
        s0 = eng.export_state()
        flat = eng.get_params()
        gap = []
        for with_ansatz in (False, True):
            if with_ansatz:
                register_ansatz(eng, ac.ansatz(i))
            a = _theta_after(eng, s0, lambda: eng.train_step(0))
            b = _theta_after(eng, s0, lambda: (eng.grad(0), eng.apply()))
            assert np.max(np.abs(a - flat)) > 1e-4                       # the step moved theta
            gap.append(float(np.max(np.abs(a - b))))
        print('ansatz train_step vs grad + apply: gap without %.3e, with %.3e' % tuple(gap))
        assert gap[1] <= max(2.0 * gap[0], 1e-6), gap
    finally:
        eng.close()


def test_epoch_is_its_single_steps():
    """Two batches (the second with other streams); an epoch over (0, 1, 0) against the three single steps; snapshot and
    rollback return the parameters of before."""
    i = 1
    d = ac.inputs(i)
    z1 = ac.stream_set(np.random.default_rng(25), CASES[i][3] * CASES[i][4])
    engs = [make_engine(i), make_engine(i)]
    try:
        for e in engs:
            e.set_interior(1, d['Input'], d['gcoef'], d['source'], n_k=CASES[i][4], detJ=d['detJ'])
            e.set_ansatz(1, **z1)
        a, b = engs
        a.state_snapshot()
        acc = torch.zeros(1, device='cuda')
        a.train_epoch((0, 1, 0), acc)
        one = torch.zeros(1, device='cuda')
        total = 0.0
        for batch in (0, 1, 0):
            b.train_step(batch, one)
            total += float(one.item())
        torch.cuda.synchronize()
        assert np.array_equal(a.get_params(), b.get_params())
        assert abs(float(acc.item()) - total) <= 1e-5 * abs(total)
        a.state_rollback()
        assert np.array_equal(a.get_params(), ac.theta(i)) and a.step == 0
        g0, g1 = grad_of(a, 0), grad_of(a, 1)
        assert not np.array_equal(g0, g1)                              # the second batch's streams are its own
    finally:
        for e in engs:
            e.close()


def test_lbfgs_step():
    """vn_lbfgs_step on an ansatz batch: the first call's f_k is the reference loss, accepted steps lower it, a changed
    registration invalidates (f_k, g_k); the fp64 loss is refused."""
    i = 1
    eng = make_engine(i, optimizer='lbfgs')
    try:
        ref = ac.reference64(i)[0]
        info = eng.lbfgs_step(0)
        assert abs(info['f_k'] - ref['loss']) <= LOSS_RTOL * abs(ref['loss']) + 1e-7
        assert info['status'] == 0 and info['f_next'] < info['f_k']
        f = info['f_next']
        for _ in range(3):
            info = eng.lbfgs_step(0)
            assert info['status'] == 0 and abs(info['f_k'] - f) <= 1e-6 * abs(f) and info['f_next'] < f
            f = info['f_next']
        az = ac.ansatz(i)
        eng.set_ansatz(0, **dict(az['int'], A=None))                   # another objective
        info = eng.lbfgs_step(0)
        assert info['pairs'] == 0 and abs(info['f_k'] - f) > 1e-3 * abs(f)
        eng.lbfgs_loss64(True)
        with pytest.raises(VNError, match='error 5.*fp64'):
            eng.lbfgs_step(0)
    finally:
        eng.close()


# ---- exactness, bit-for-bit neutrality --------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
@pytest.mark.parametrize('i', [0, 2], ids=[IDS[0], IDS[2]])
def test_exact_data_on_the_bcic_rows(i, kernel):
    """B = 0 and A = label on every BC/IC row: the bc and ic components are 0.0 exactly, and the gradient equals, bit for bit,
    that of the same engine with w_b = w_i = 0."""
    d = ac.inputs(i)
    nB = CASES[i][5]
    az = dict(ac.ansatz(i), bic=dict(A=d['biLabel'].reshape(-1), B=np.zeros(nB, dtype=np.float32), a=None, b=None))
    eng = make_engine(i, kernel, az=az)
    try:
        out, _ = eng.eval_loss(0)
        g = grad_of(eng)
        assert out[1] == 0.0 and out[2] == 0.0 and g[eng.P + 1] == 0.0 and g[eng.P + 2] == 0.0
        assert out[0] == d['w'][2] * out[3] or abs(out[0] - d['w'][2] * out[3]) <= 1e-6 * abs(out[0])
        eng.set_weights([0.0, 0.0, d['w'][2]])
        g0 = grad_of(eng)
        assert np.array_equal(g[:eng.P], g0[:eng.P]) and np.any(g[:eng.P] != 0.0)
    finally:
        eng.close()


@pytest.mark.parametrize('kernel', [VN_KERNEL_AUTO, VN_KERNEL_GENERIC], ids=['auto', 'generic'])
def test_cleared_ansatz_is_bit_for_bit_no_ansatz(kernel):
    """An engine whose ansatz was registered, used and cleared against one that never had one."""
    i = 3
    a, b = make_engine(i, kernel), make_engine(i, kernel, az=None)
    try:
        ga = grad_of(a)
        a.set_ansatz(0)
        a.set_ansatz_rows('bic')
        g1, g2 = grad_of(a), grad_of(b)
        assert np.array_equal(g1, g2) and not np.array_equal(ga, g2)
        assert a.eval_loss(0, lossVec=True)[0] == b.eval_loss(0, lossVec=True)[0]
        assert tuple(a.kernel_path()) == tuple(b.kernel_path())
    finally:
        a.close()
        b.close()


# ---- the registration contract and every refusal ----------------------------------------------------------------------
def test_all_or_nothing_rule():
    """A batch with an ansatz and a registered row set without one, or the other way round, is refused at the evaluation with a
    sentence that names what is missing."""
    i = ac.EDGE_CASE
    az = ac.ansatz(i)
    eng = make_engine(i, az=None)
    try:
        eng.set_ansatz(0, **az['int'])
        for call in (lambda: eng.grad(0), lambda: eng.eval_loss(0), lambda: eng.train_step(0)):
            with pytest.raises(VNError, match=r'error 3.*BC/IC rows \(VN_ANSATZ_BIC\) have no ansatz streams'):
                call()
        eng.set_ansatz_rows('bic', **az['bic'])
        eng.grad(0)
        for kind, label in (('flux', 'boundary-flux rows'), ('periodic_g1', 'periodic pairs'), ('obs_values', 'observations')):
            name, reg, z = ac.edge(kind, 33)
            register_edge(eng, name, reg)
            with pytest.raises(VNError, match='error 3.*%s.*have no ansatz streams' % label):
                eng.grad(0)
            eng.set_ansatz_rows(name, **z)
            eng.grad(0)
            register_edge(eng, name, reg)                              # registering the set again drops its streams
            with pytest.raises(VNError, match='error 3.*%s.*have no ansatz streams' % label):
                eng.eval_loss(0)
            eng.set_ansatz_rows(name, **z)
        eng.set_ansatz(0)                                              # the other way round
        with pytest.raises(VNError, match='error 3.*batch 0 has no ansatz'):
            eng.grad(0)
        eng.set_ansatz(0, **az['int'])
        d = ac.inputs(i)
        eng.set_bic(d['biInput'], d['biLabel'], CASES[i][6], ac.BIDIMVAL)   # ... and vn_set_bic drops the BC/IC streams
        with pytest.raises(VNError, match=r'error 3.*VN_ANSATZ_BIC'):
            eng.grad(0)
        eng.set_ansatz_rows('bic', **az['bic'])
        eng.grad(0)
        eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=CASES[i][4], detJ=d['detJ'])   # a new vn_set_interior clears the batch's
        with pytest.raises(VNError, match='error 3.*batch 0 has no ansatz'):
            eng.grad(0)
    finally:
        eng.close()


def test_registration_contract():
    i = ac.EDGE_CASE
    az = ac.ansatz(i)
    d = ac.inputs(i)
    n = CASES[i][3] * CASES[i][4]
    eng = make_engine(i, az=None)
    try:
        with pytest.raises(VNError, match='error 3'):                  # an unregistered batch
            eng.set_ansatz(5, **az['int'])
        with pytest.raises(VNError, match='error 1.*B_dev is required'):
            eng.set_ansatz(0, A=az['int']['A'])
        with pytest.raises(ValueError):                                # the binding checks the lengths
            eng.set_ansatz(0, B=az['int']['B'][:-1])
        bad = az['int']['B'].copy()
        bad[7] = np.nan
        with pytest.raises(VNError, match='error 1.*1 non-finite entry'):
            eng.set_ansatz(0, B=bad)
        bad = az['int']['a'].copy()
        bad[[0, n - 1]] = np.inf
        with pytest.raises(VNError, match='error 1.*2 non-finite entries'):
            eng.set_ansatz(0, **dict(az['int'], a=bad))
        with pytest.raises(VNError, match='error 3.*no de-duplication map'):
            eng.set_ansatz_points(0, B=np.ones(3, dtype=np.float32))
        # row sets: not registered; derivatives on a set without directions
        for name in ('flux', 'periodic', 'obs'):
            with pytest.raises(VNError, match='error 3.*are not registered'):
                eng.set_ansatz_rows(name, B=np.ones(4, dtype=np.float32))
        with pytest.raises(ValueError):
            eng.set_ansatz_rows('walls', B=np.ones(4, dtype=np.float32))
        nB = CASES[i][5]
        ones = np.ones(nB, dtype=np.float32)
        with pytest.raises(VNError, match='error 1.*have no direction'):
            eng.set_ansatz_rows('bic', B=ones, a=ones)
        for kind in ('periodic_g0', 'obs_values'):
            name, reg, z = ac.edge(kind, 33)
            register_edge(eng, name, reg)
            with pytest.raises(VNError, match='error 1.*have no direction'):
                eng.set_ansatz_rows(name, B=z['B'], b=z['B'])
            eng.set_ansatz_rows(name, **z)
        # a per-batch BC/IC copy next to BC/IC streams, in either order
        eng.set_ansatz_rows('bic', **az['bic'])
        with pytest.raises(VNError, match='error 5.*vn_set_batch_bic'):
            eng.set_batch_bic(0, d['biInput'], d['biLabel'])
        eng.set_ansatz_rows('bic')
        eng.set_batch_bic(0, d['biInput'], d['biLabel'])
        with pytest.raises(VNError, match='error 5.*vn_set_batch_bic'):
            eng.set_ansatz_rows('bic', **az['bic'])
        eng.set_batch_bic(0)
    finally:
        eng.close()


def test_refusals():
    """The 4-wave cross-check geometry, the layer-by-layer route, the fp64 objective and learnt vectors next to an ansatz."""
    for kernel, i in ((VN_KERNEL_FUSED, 2), (VN_KERNEL_LAYERED, ac.EDGE_CASE)):     # (the 4-wave geometry takes sigmoid nets)
        az = ac.ansatz(i)
        eng = make_engine(i, kernel, az=None)
        try:
            with pytest.raises(VNError, match='error 5'):
                eng.set_ansatz(0, **az['int'])
            with pytest.raises(VNError, match='error 5'):
                eng.set_ansatz_rows('bic', **az['bic'])
            grad_of(eng)                                               # ... and the engine goes on without one
        finally:
            eng.close()
    i = ac.EDGE_CASE
    eng = make_engine(i)
    try:
        with pytest.raises(VNError, match='error 5.*vn_objective_f64'):
            eng.objective64(0)
        with pytest.raises(VNError, match='error 5.*vn_objective_f64'):
            eng.eval_loss(0, fp64=True)
        eng.set_reaction(0, None, [0.5, 0.0, 0.0])
        eng.set_coef_learn(mask=[1, 0, 0, 0, 0, 0, 0, 0, 0], init=[0.5, 0, 0, 0, 0, 0, 1, 0, 0], lr=1e-3)
        with pytest.raises(VNError, match='error 5.*learnt .* next to a hard-constraint ansatz'):
            eng.grad(0)
    finally:
        eng.close()
