"""
Randomised cross-check of the nonlinear PDE terms (vn_set_reaction, vn_set_nlflux, vn_set_nldiff) and the boundary-flux rows
(vn_set_flux_bc) on every GPU route, against the fp64 restatement tests/nldiff_ref.py (test infrastructure: plain module, no
pytest marks; shared by tests/test_fuzz_terms_host.py and tests/test_fuzz_terms_gpu.py).

Cases: tests/fuzz_routes.draw_case (its draw sequence untouched: a seed names the same net as there) cut to GPU-seconds sizes
(n_k <= 40 and n_k * q <= 20 000 rows, never `big`); everything else comes from generators of this module, default_rng([seed,
7000 + case]): one draw in six becomes a block-crossing draw (q in {4, 8, 16}, n_k in 257..300: more than one 256-test-function
seed block), a non-empty subset of the three terms (all three in a third of the cases) with streams rate = U(0.5, 2) or None,
phi = 4 N(0,1), psi = 8 N(0,1) or None, coefficients the full cubic / quadratic, a single non-zero coefficient or the degenerate
D = (0, 0, 1); one case in four registers its streams from views one float off the 16-byte grid (the one-row forms of the
elementwise kernels); one case in three draws 10..60 boundary-flux rows.  Inputs as tests/nldiff_cases.py scales them: gcoef x 8,
parameters 2 x (init_params(seed=case) + 0.05 N(0,1)) in fp32 -- that a missing term then fails the bars is asserted from the
reference alone in tests/test_fuzz_terms_host.py.  Rows share points (the map of tests/fuzz_routes.py, from default_rng(5000 +
case)) wherever the de-duplicated step could take the case (q <= 256, no detJ vector, no per-row tables), whether or not the net
is one it serves: the inputs of a case do not depend on the device.

Routes, on the same inputs: AUTO (0), the generic kernels (1) when in range, both forms of the layer-by-layer route (tile kernels
4, GEMM form 40) on every net, the de-duplicated step (30) where the engine supports it, vn_objective_f64 (64) where its range
allows (elsewhere the documented VN_EUNSUPPORTED is asserted).  Boundary-flux rows run on every engine that takes them (AUTO and
generic inside VN_KMAX_*, the de-duplicated step, the fp64 objective); the layer-by-layer engines and nets outside the range must
refuse them with VN_EUNSUPPORTED and run the case without.  Every fourth case also registers batch 1 on the AUTO engine (2-3 x
the test functions, another term subset: the engine-owned work buffers grow) and requires grad(0), grad(1), grad(0) to give the
same bits for batch 0 and batch 1 to meet the bars against its own reference.

Bars (none of this module's own): tests/fuzz_routes.py LOSS_BAR, GRAD_BAR, PAIR_BAR with its per-block rule and its whitelist
rule (bars widen to 2 x dev32 only when the fp32 reference itself deviates by more than 1e-4); eval_loss's lossVec at
LVEC_RTOL (tests/test_engine_gpu.py); vn_objective_f64 at the LOSS_BAR, GRAD_BAR and LVEC_BAR of tests/test_obj64_gpu.py.

    python -m tests.fuzz_terms [cases] [seed]      (soak; on the GPU box)
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import tf1_graph as og  # noqa: E402
from tests import flux_ref, nldiff_ref  # noqa: E402
from tests import fuzz_routes as fz  # noqa: E402
from tests.fuzz_routes import COND_WHITELIST, GRAD_BAR, LOSS_BAR, PAIR_BAR, U32  # noqa: E402
from tests.gradcheck import block_errors  # noqa: E402
from tests.nldiff_cases import DEGENERATE, DIFF, GCOEF_SCALE, PSI_SCALE, THETA_SCALE  # noqa: E402
from tests.nlflux_cases import FLUX  # noqa: E402
from tests.reaction_cases import COEF  # noqa: E402
from tests.test_engine_gpu import LVEC_RTOL  # noqa: E402
from tests.test_obj64_gpu import GRAD_BAR as GRAD64_BAR, LOSS_BAR as LOSS64_BAR, LVEC_BAR as LVEC64_BAR  # noqa: E402

KEYS = ['loss', 'BCloss', 'ICloss', 'varLoss']
MAX_ROWS = 20000
MAX_NK = 40
VN_KMAX_LAYERS, VN_KMAX_WIDTH, VN_KMAX_DIN = 6, 64, 8
TERMS = ('reaction', 'nlflux', 'nldiff')
PHI_SCALE = 4.0             # phi = 4 N(0,1) (rate = U(0.5, 2) and psi = PSI_SCALE N(0,1) as in the seven-case tables)
# full coefficient sets: those of tests/reaction_cases.py, tests/nlflux_cases.py, tests/nldiff_cases.py
FULL = {'reaction': COEF, 'nlflux': FLUX, 'nldiff': DIFF}
BIDIMVAL = 2.0

# (seed, cases, steady, mor): the lists of the pytest tiers, at most 8 cases each
SEED_LISTS = [(0, 8, False, False), (7, 8, False, False), (12, 8, False, False), (31, 8, True, False), (5, 8, False, True)]


# ---- cases ----------------------------------------------------------------------------------------------------------
def in_kernel_range(c):
    """The net lies inside VN_KMAX_* (one activation always: draw_case draws one name per net)."""
    return c['L'] <= VN_KMAX_LAYERS and max(c['widths']) <= VN_KMAX_WIDTH and c['d_in'] <= VN_KMAX_DIN


def shares_points(c):
    """Rows draw their inputs from a smaller set of unique points: wherever the de-duplicated step's own conditions (other than
    the net) hold."""
    return not c['djv'] and not c['rows'] and c['dim'] <= 3 and c['q'] <= 256


def _coef(r, term):
    full = FULL[term]
    kinds = ['cubic', 'quadratic', 'single'] + (['degenerate'] if term == 'nldiff' else [])
    kind = kinds[int(r.integers(0, len(kinds)))]
    k = int(r.integers(0, 3))
    if kind == 'cubic':
        return full
    if kind == 'quadratic':
        return (full[0], full[1], 0.0)
    if kind == 'degenerate':
        return DEGENERATE
    return tuple(full[j] if j == k else 0.0 for j in range(3))


def _subset(r):
    if r.random() < 1.0 / 3.0:
        return TERMS
    proper = [('reaction',), ('nlflux',), ('nldiff',), ('reaction', 'nlflux'), ('reaction', 'nldiff'), ('nlflux', 'nldiff')]
    return proper[int(r.integers(0, len(proper)))]


def _terms(r, names, n):
    """{term: (stream [n,1] fp32 or None, coef)} for the drawn names."""
    f32 = np.float32
    t = {}
    if 'reaction' in names:
        rate = None if r.random() < 0.25 else r.uniform(0.5, 2.0, (n, 1)).astype(f32)
        t['reaction'] = (rate, _coef(r, 'reaction'))
    if 'nlflux' in names:
        t['nlflux'] = ((f32(PHI_SCALE) * r.standard_normal((n, 1)).astype(f32)).astype(f32), _coef(r, 'nlflux'))
    if 'nldiff' in names:
        psi = None if r.random() < 0.25 else (f32(PSI_SCALE) * r.standard_normal((n, 1)).astype(f32)).astype(f32)
        coef = _coef(r, 'nldiff')
        if psi is None and coef == (1.0, 0.0, 0.0):      # (not drawable from FULL; D = 1 without psi would clear the registration)
            coef = FULL['nldiff']
        t['nldiff'] = (psi, coef)
    return t


def draw_case(rng, case, seed, steady=False, mor=False):
    """fuzz_routes.draw_case (rng advanced exactly as there) under the size rules, plus this module's own draws."""
    c = fz.draw_case(rng, case, steady=steady, mor=mor)
    r = np.random.default_rng([seed, 7000 + case])
    c['seed'] = seed
    c['crossing'] = bool(r.random() < 1.0 / 6.0)
    q_x, nk_x = int(r.choice([4, 8, 16])), int(r.integers(257, 301))
    if c['crossing']:
        c['q'], c['n_k'] = q_x, nk_x
    else:
        c['n_k'] = min(c['n_k'], MAX_NK)
        while c['n_k'] * c['q'] > MAX_ROWS:
            c['n_k'] -= 1
    c['big'] = False
    n = c['n_k'] * c['q']
    c['terms'] = _terms(r, _subset(r), n)
    c['offset'] = bool(r.random() < 0.25)
    c['flux'] = None
    if r.random() < 1.0 / 3.0:
        nF = int(r.integers(10, 61))
        nrm = r.standard_normal((nF, c['dim']))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        coef = r.uniform(0.5, 2.0, nF)
        coef[:nF // 2] = 0.0
        c['flux'] = {k: np.asarray(v).astype(np.float32) for k, v in
                     dict(X=r.uniform(-1, 1, (nF, c['d_in'])), normal=nrm, coef=coef, label=r.standard_normal(nF)).items()}
    c['grow'] = None
    if case % 4 == 0:
        names = _subset(r)
        while set(names) == set(c['terms']):
            names = _subset(r)
        n_k1 = int(r.integers(2 * c['n_k'], 3 * c['n_k'] + 1))
        c['grow'] = dict(n_k=n_k1, terms=_terms(r, names, n_k1 * c['q']))
    return c


def draw_list(seed, ncases, steady=False, mor=False):
    rng = np.random.default_rng(seed)
    return [draw_case(rng, case, seed, steady, mor) for case in range(ncases)]


def all_cases():
    return [c for lst in SEED_LISTS for c in draw_list(*lst)]


def case_inputs(c, batch=0):
    """(inputs dict of fuzz_routes.synth with gcoef x 8, shared-point map or None).  Batch 1 (the buffer-growth check): rows of
    its own on the FE table, per-row tables and BC/IC rows of batch 0."""
    n_k = c['n_k'] if batch == 0 else c['grow']['n_k']
    d = fz.synth(1000 + c['case'] + 100000 * batch, c['d_in'], c['dim'], c['widths'], c['q'], n_k, c['nB'], c['bDof'], c['src'], c['iw'],
                 c['djv'])
    if batch:
        d0 = fz.synth(1000 + c['case'], c['d_in'], c['dim'], c['widths'], c['q'], c['n_k'], c['nB'], c['bDof'], c['src'], c['iw'], c['djv'])
        for k in ('N1', 'dNt1', 'integW', 'biInput', 'biLabel', 'w'):
            d[k] = d0[k]
        n = n_k * c['q']
        d['N'], d['dNt'] = np.tile(d['N1'], n_k).reshape(n, 1), np.tile(d['dNt1'], n_k).reshape(n, 1)
    d['gcoef'] = (np.float32(GCOEF_SCALE) * d['gcoef']).astype(np.float32)
    dd = None
    if batch == 0 and shares_points(c):
        r5 = np.random.default_rng(5000 + c['case'])
        n = n_k * c['q']
        U = max(1, n // int(r5.integers(1, 9)))
        uid = r5.integers(0, U, n).astype(np.int32)
        uid[:U] = np.arange(U)                      # every unique point is used
        r5.shuffle(uid)
        Xu = d['Input'][:U].copy()
        d['Input'] = Xu[uid]
        rowptr = np.zeros(U + 1, dtype=np.int32)
        rowptr[1:] = np.cumsum(np.bincount(uid, minlength=U))
        dd = (Xu, uid, rowptr, np.argsort(uid, kind='stable').astype(np.int32))
    return d, dd


def theta(c):
    """2 x (init_params(seed=case) + 0.05 N(0,1)) in fp32 (oracle glorot_init == vn_params_init bit for bit)."""
    flat = og.glorot_init(c['d_in'], c['widths'], c['case'])
    flat = flat + 0.05 * np.random.default_rng(c['case']).standard_normal(flat.size).astype(np.float32)
    return (np.float32(THETA_SCALE) * flat.astype(np.float32)).astype(np.float32)


def reference(c, d, flat, dtype=torch.float64, terms=None, flux=None, n_k=None):
    """tests/nldiff_ref.loss_and_grad with the case's terms ({} / missing names: without them; none: the oracle bit for bit),
    plus tests/flux_ref.flux_term composed as tests/test_nldiff_gpu.py composes it.  Returns (result dict, gradient [P])."""
    f = np.float64 if dtype == torch.float64 else np.float32
    cv = lambda a: None if a is None else np.asarray(a).astype(f)
    terms = c['terms'] if terms is None else terms
    cast = lambda t: None if t is None else (cv(t[0]), t[1])
    flat = np.asarray(flat).astype(f)
    res, g = nldiff_ref.loss_and_grad(
        flat, c['d_in'], c['widths'], cast(terms.get('nldiff')), cast(terms.get('nlflux')), cast(terms.get('reaction')), dtype,
        Input=cv(d['Input']), gcoef=cv(d['gcoef']), source=cv(d['source']), N=cv(d['N']), dNt=cv(d['dNt']), integW=cv(d['integW']),
        intShape=[c['n_k'] if n_k is None else n_k, c['q']], detJ=(cv(d['detJ']) if c['djv'] else float(d['detJ'])),
        detJvec=c['djv'], biInput=cv(d['biInput']), biLabel=cv(d['biLabel']), bDof=c['bDof'], biDimVal=BIDIMVAL, w=d['w'],
        dim=c['dim'], time_dependent=c['td'], is_source=c['src'], integWflag=c['iw'], activation=c['act'])
    g = np.asarray(g, dtype=np.float64)
    if flux is not None:
        F, gF, _ = flux_ref.flux_term(flat, c['d_in'], c['widths'], c['dim'], cv(flux['X']), cv(flux['normal']), cv(flux['coef']),
                                      cv(flux['label']), BIDIMVAL, c['act'], dtype)
        res = dict(res)
        res['BCloss'] = res['BCloss'] + F
        res['loss'] = res['loss'] + d['w'][0] * F
        g = g + d['w'][0] * gF
    return res, g


def describe(c):
    t = ' '.join('%s=%s%s' % (k, '(' + ','.join('%g' % x for x in v[1]) + ')', '' if v[0] is not None else '/nostream')
                 for k, v in c['terms'].items())
    return ('%sseed %d case %3d %s L=%d widths=%s d_in=%d dim=%d q=%d n_k=%d nB=%d src=%d iw=%d djv=%d rows=%d%s%s%s%s [%s]'
            % ('' if c['td'] else 'steady ', c['seed'], c['case'], c['act'], c['L'], c['widths'], c['d_in'], c['dim'], c['q'], c['n_k'],
               c['nB'], c['src'], c['iw'], c['djv'], c['rows'], ' crossing' if c['crossing'] else '', ' offset' if c['offset'] else '',
               ' fluxbc=%d' % len(c['flux']['X']) if c['flux'] else '', ' grow=%d' % c['grow']['n_k'] if c['grow'] else '', t))


# ---- the GPU side ---------------------------------------------------------------------------------------------------
def _stream(a, offset, keep):
    """A registered stream on the device: contiguous, or a view one float off the 16-byte grid."""
    if a is None:
        return None
    flat = torch.as_tensor(np.reshape(a, -1), device='cuda')
    if not offset:
        return flat
    buf = torch.zeros(flat.numel() + 1, device='cuda')
    buf[1:] = flat
    assert buf[1:].data_ptr() % 16 != 0
    keep.append(buf)
    return buf[1:]


def register_terms(eng, batch, terms, offset, keep):
    if 'reaction' in terms:
        eng.set_reaction(batch, _stream(terms['reaction'][0], offset, keep), terms['reaction'][1])
    if 'nlflux' in terms:
        eng.set_nlflux(batch, _stream(terms['nlflux'][0], offset, keep), terms['nlflux'][1])
    if 'nldiff' in terms:
        eng.set_nldiff(batch, _stream(terms['nldiff'][0], offset, keep), terms['nldiff'][1])


def register_interior(eng, c, d, batch, n_k):
    kw = dict(N_rows=d['N'], dNt_rows=d['dNt']) if c['rows'] else {}
    eng.set_interior(batch, d['Input'], d['gcoef'], d['source'], n_k=n_k, detJ=d['detJ'], **kw)


def grad_of(eng, gb, batch=0):
    eng.grad(batch)
    torch.cuda.synchronize()
    return gb.cpu().numpy().astype(np.float64)


def _rel(got, want):
    return abs(got - want) / max(abs(want), 1e-300) if want != 0.0 else abs(got)


class _Judge:
    """The bars of tests/fuzz_routes.run_case for a group of gradients that share a reference."""

    def __init__(self, c, ref, gref, g32):
        self.c, self.ref, self.g64, self.g32fn = c, ref, gref, g32
        self.grads, self.routes = [], []

    def add(self, route, g):
        self.grads.append(g)
        self.routes.append(route)

    def verdict(self, per_route):
        c, grads, g64 = self.c, self.grads, self.g64
        P = g64.size
        bk = lambda a, b: block_errors(a, b, c['d_in'], c['widths'], c['dim'], c['td'])
        pair = lpair = 0.0
        pairb = {}
        for i in range(len(grads)):
            for j in range(i):
                sc = max(np.max(np.abs(grads[j][:P])), 1e-30)
                pair = max(pair, np.max(np.abs(grads[i][:P] - grads[j][:P])) / sc)
                lpair = max(lpair, abs(grads[i][P] - grads[j][P]) / max(abs(grads[j][P]), 1e-30))
                for b, e in bk(grads[i], grads[j]).items():
                    pairb[b] = max(pairb.get(b, 0.0), e)
        sc = max(np.max(np.abs(g64)), 1e-30)
        gerr = lerr = 0.0
        gerrb = {}
        for route, g in zip(self.routes, grads):
            ge = float(np.max(np.abs(g[:P] - g64)) / sc)
            le = max(_rel(g[P + k], self.ref[KEYS[k]]) for k in range(4))
            be = bk(g, g64)
            rec = per_route.setdefault(str(route), {})
            for k, v in (('grad', ge), ('grad_block', max(be.values())), ('loss', le)):
                rec[k] = max(rec.get(k, 0.0), v)
            gerr, lerr = max(gerr, ge), max(lerr, le)
            for b, e in be.items():
                gerrb[b] = max(gerrb.get(b, 0.0), e)
        out = dict(pair=pair, lpair=lpair, gerr=gerr, lerr=lerr, cond=None, cond_blocks={}, finite=all(np.all(np.isfinite(g)) for g in grads),
                   gerr_block=max(gerrb, key=gerrb.get), gerr_block_err=max(gerrb.values()),
                   pair_block_err=max(pairb.values(), default=0.0))
        gbar, pbar = GRAD_BAR, PAIR_BAR
        need32 = (pair > PAIR_BAR or out['pair_block_err'] > PAIR_BAR or gerr > GRAD_BAR or out['gerr_block_err'] > GRAD_BAR)
        if need32:
            g32 = self.g32fn()
            dev32 = np.max(np.abs(g32 - g64)) / sc
            out['cond'] = dev32 / U32
            if out['cond'] > COND_WHITELIST:            # ill-conditioned draw: bars follow its measured conditioning
                gbar, pbar = max(GRAD_BAR, 2 * dev32), max(PAIR_BAR, 2 * dev32)
            dev32b = bk(g32, g64)
            out['cond_blocks'] = {b: dev32b[b] / U32 for b in dev32b if gerrb.get(b, 0.0) > GRAD_BAR or pairb.get(b, 0.0) > PAIR_BAR}
        cb = out['cond_blocks']
        blocks_ok = all(pairb[b] <= max(pbar, 2 * cb.get(b, 0.0) * U32) for b in pairb)
        blocks_ok = blocks_ok and all(e <= max(gbar, 2 * cb.get(b, 0.0) * U32) for b, e in gerrb.items())
        out['ok'] = bool(out['finite'] and pair <= pbar and lpair <= 5e-5 and blocks_ok and gerr <= gbar and lerr <= LOSS_BAR)
        return out


def _check_eval(eng, ref, rec, batch=0):
    """eval_loss with lossVec against the reference: loss components at LOSS_BAR, lossVec at LVEC_RTOL of its maximum."""
    out, lv = eng.eval_loss(batch, lossVec=True)
    le = max(_rel(got, ref[k]) for got, k in zip(out, KEYS))
    lref = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1)
    ve = float(np.max(np.abs(lv.cpu().numpy() - lref)) / max(np.max(np.abs(lref)), 1e-300))
    rec['eval_loss'] = max(rec.get('eval_loss', 0.0), le)
    rec['lossVec'] = max(rec.get('lossVec', 0.0), ve)
    return le <= LOSS_BAR and ve <= LVEC_RTOL, le, ve


def _check_obj64(eng, c, ref, gref, rec):
    out, g, lv = eng.objective64(0, grad=True, lossVec=True)
    le = max(_rel(got, ref[k]) for got, k in zip(out, KEYS))
    lref = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1)
    ve = float(np.max(np.abs(lv.cpu().numpy() - lref)) / max(np.max(np.abs(lref)), 1e-300))
    gn = g.cpu().numpy()
    be = max(block_errors(gn, gref, c['d_in'], c['widths'], c['dim'], c['td']).values())
    for k, v in (('loss', le), ('lossVec', ve), ('grad_block', be)):
        rec[k] = max(rec.get(k, 0.0), v)
    return bool(np.all(np.isfinite(gn)) and le <= LOSS64_BAR and ve <= LVEC64_BAR and be <= GRAD64_BAR), le, ve, be


def _refused(fn):
    """The call is refused with the documented VN_EUNSUPPORTED (error 5)."""
    from varnet_amd.engine import VNError
    try:
        fn()
    except VNError as e:
        return 'error 5' in str(e)
    return False


def run_case(c):
    """Every route that can take the case.  Returns a result dict: result['ok'] the verdict, result['msg'] a line,
    result['per_route'] {route: {quantity: worst error}}, result['paths'] {requested kernel: kernel_path()}."""
    d, dd = case_inputs(c)
    flat = theta(c)
    rng_ok = in_kernel_range(c)
    flux = c['flux']
    ref_p, g_p = reference(c, d, flat)                                           # without flux rows
    plain = _Judge(c, ref_p, g_p, lambda: reference(c, d, flat, torch.float32)[1])
    withf = None
    if flux is not None and rng_ok:
        ref_f, g_f = reference(c, d, flat, flux=flux)
        withf = _Judge(c, ref_f, g_f, lambda: reference(c, d, flat, torch.float32, flux=flux)[1])
    kernels = [0]
    if rng_ok:
        try:
            fz.make_engine(c['d_in'], c['dim'], c['widths'], c['q'], c['src'], c['iw'], 1, c['act'], c['td']).close()
            kernels.append(1)
        except Exception:                       # deep + wide: too big for the generic kernels' LDS
            pass
    kernels += [4, 40]
    per_route, paths, notes, fails = {}, {}, [], []
    grow = None
    for kernel in kernels:
        eng = fz.make_engine(c['d_in'], c['dim'], c['widths'], c['q'], c['src'], c['iw'], kernel, c['act'], c['td'])
        keep = []
        try:
            eng.set_params(flat)
            eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
            register_interior(eng, c, d, 0, c['n_k'])
            eng.set_bic(d['biInput'], d['biLabel'], c['bDof'], BIDIMVAL)
            eng.set_weights(d['w'])
            register_terms(eng, 0, c['terms'], c['offset'], keep)
            kp = tuple(eng.kernel_path())
            paths[str(kernel)] = list(kp)
            layered = kp[0] == 4
            judge, ref, gref = plain, ref_p, g_p
            if flux is not None:
                set_flux = lambda: eng.set_flux_bc(flux['X'], flux['normal'], flux['coef'], flux['label'], BIDIMVAL)
                if rng_ok and not layered:
                    set_flux()
                    judge, ref, gref = withf, ref_f, g_f
                elif not _refused(set_flux):         # outside VN_KMAX_* / layer by layer: the documented refusal, never silent
                    fails.append('route %d: flux rows not refused with VN_EUNSUPPORTED' % kernel)
            gb = eng.bind_grad_buffer()
            route = kernel                           # 0: whatever AUTO chose (kernel_path() is recorded under paths)
            g0 = grad_of(eng, gb)
            judge.add(route, g0)
            rec = per_route.setdefault(str(route), {})
            ok, le, ve = _check_eval(eng, ref, rec)
            if not ok:
                fails.append('route %d: eval_loss %.1e lossVec %.1e' % (route, le, ve))
            if kernel != 0:
                continue
            # the fp64 objective of the same batch, where the header's range allows
            if rng_ok and c['dim'] <= 3:
                ok, le, ve, be = _check_obj64(eng, c, ref, gref, per_route.setdefault('64', {}))
                notes.append('obj64 %.1e/%.1e/%.1e' % (le, ve, be))
                if not ok:
                    fails.append('objective64: loss %.1e lossVec %.1e gradient block %.1e' % (le, ve, be))
            elif not _refused(lambda: eng.objective64(0, grad=True)):
                fails.append('objective64 not refused with VN_EUNSUPPORTED')
            # buffer growth: a larger batch 1 with another term subset between two evaluations of batch 0
            if c['grow'] is not None:
                d1, _ = case_inputs(c, 1)
                n_k1, t1 = c['grow']['n_k'], c['grow']['terms']
                register_interior(eng, c, d1, 1, n_k1)
                register_terms(eng, 1, t1, False, keep)
                fx = flux if judge is withf else None
                ref1, gref1 = reference(c, d1, flat, terms=t1, flux=fx, n_k=n_k1)
                j1 = _Judge(c, ref1, gref1, lambda: reference(c, d1, flat, torch.float32, terms=t1, flux=fx, n_k=n_k1)[1])
                g1 = grad_of(eng, gb, 1)
                j1.add(route, g1)
                again = grad_of(eng, gb, 0)
                tmp = {}
                grow = j1.verdict(tmp)
                per_route['grow'] = tmp[str(route)]
                grow['bitwise'] = bool(np.array_equal(g0, again))
                notes.append('grow n_k=%d %.1e/%.1e%s' % (n_k1, grow['gerr'], grow['lerr'], '' if grow['bitwise'] else ' NOT BITWISE'))
                if not (grow['ok'] and grow['bitwise']):
                    fails.append('buffer growth: batch 1 gradient %.1e loss %.1e, batch 0 bitwise %s' % (grow['gerr'], grow['lerr'], grow['bitwise']))
            # the de-duplicated step on the shared-point map
            if dd is not None and eng.dedup_supported():
                eng.set_dedup(0, *dd)
                judge.add(30, grad_of(eng, gb))
                ok, le, ve = _check_eval(eng, ref, per_route.setdefault('30', {}))
                if not ok:
                    fails.append('route 30: eval_loss %.1e lossVec %.1e' % (le, ve))
        finally:
            eng.close()
            del keep
    groups = [j for j in (plain, withf) if j is not None and j.grads]
    verdicts = [j.verdict(per_route) for j in groups]
    routes = [r for j in groups for r in j.routes]
    flux_routes = list(withf.routes) + ([64] if rng_ok and c['dim'] <= 3 else []) if withf is not None else []
    ok = all(v['ok'] for v in verdicts) and not fails
    res = dict(case=c['case'], seed=c['seed'], routes=routes, flux_routes=flux_routes, per_route=per_route, paths=paths, grow=grow,
               verdicts=verdicts, ok=bool(ok), fails=fails,
               cond=max((v['cond'] for v in verdicts if v['cond'] is not None), default=None))
    msg = describe(c) + ' routes=%s%s:' % (routes, ' flux on %s' % flux_routes if flux is not None else '')
    for v in verdicts:
        msg += '  pair %.1e/%.1e pair/block %.1e ref %.1e/%.1e ref/block %.1e (%s)' % (
            v['pair'], v['lpair'], v['pair_block_err'], v['gerr'], v['lerr'], v['gerr_block_err'], v['gerr_block'])
        if v['cond'] is not None:
            msg += ' cond %.1e%s' % (v['cond'], ' (whitelisted)' if v['cond'] > COND_WHITELIST else '')
        if v['cond_blocks']:
            msg += ' cond/block ' + ', '.join('%s %.1e' % kv for kv in v['cond_blocks'].items())
    msg += '  ' + '  '.join(notes)
    if not ok:
        msg += '   <<<<<<<< MISMATCH ' + '; '.join(fails)
        save_mismatch(c, d, flat, groups)
    res['msg'] = msg
    return res


def save_mismatch(c, d, flat, groups):
    """The case in the shape of fuzz_routes' fuzz_mismatch.npz, with the streams, coefficients and flux rows added."""
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(ROOT, 'profile_out')      # where the tier's record goes as well
    os.makedirs(out, exist_ok=True)
    z = lambda a: np.zeros(0) if a is None else np.asarray(a)
    extra = {}
    for name, (stream, coef) in c['terms'].items():
        extra['term_%s_stream' % name], extra['term_%s_coef' % name] = z(stream), np.asarray(coef)
    for k, v in (c['flux'] or {}).items():
        extra['flux_' + k] = v
    np.savez(os.path.join(out, 'fuzz_terms_mismatch.npz'), widths=np.array(c['widths']), d_in=c['d_in'], dim=c['dim'], q=c['q'],
             n_k=c['n_k'], nB=c['nB'], bDof=c['bDof'], td=c['td'], src=c['src'], iw=c['iw'], djv=c['djv'], rows=c['rows'], act=c['act'],
             flat=flat, seed=c['seed'], case=c['case'], offset=c['offset'],
             routes=np.array([r for j in groups for r in j.routes]), grads=np.array([g for j in groups for g in j.grads]),
             **extra, **{'d_' + k: z(v) for k, v in d.items()})


def merge_record(record, res):
    """Worst error per route and quantity, and the kernel paths seen per requested kernel."""
    for route, rec in res['per_route'].items():
        tgt = record.setdefault('routes', {}).setdefault(route, {})
        for k, v in rec.items():
            tgt[k] = max(tgt.get(k, 0.0), float(v))
    for v in res['verdicts']:
        if v['cond'] is None or v['cond'] <= COND_WHITELIST:
            record['pair'] = max(record.get('pair', 0.0), float(v['pair']))
    for kernel, kp in res['paths'].items():
        seen = record.setdefault('kernel_paths', {}).setdefault(kernel, [])
        if kp not in seen:
            seen.append(kp)
            seen.sort()
    for r in res['flux_routes']:
        fr = record.setdefault('flux_bc_routes', [])
        if r not in fr:
            fr.append(r)
            fr.sort()


def main():
    ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    record = {}
    n_wl = 0
    t0 = time.time()
    for c in draw_list(seed, ncases):
        r = run_case(c)
        print(r['msg'], flush=True)
        if not r['ok']:
            sys.exit(1)
        n_wl += r['cond'] is not None and r['cond'] > COND_WHITELIST
        merge_record(record, r)
    print('all %d cases agree (seed %d, %.0f s); %d ill-conditioned draws whitelisted by their condition estimate; worst per route: %s'
          % (ncases, seed, time.time() - t0, n_wl, record.get('routes')))


if __name__ == '__main__':
    main()
