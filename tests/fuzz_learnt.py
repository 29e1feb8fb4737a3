"""
Randomised cross-check of the five learnt vectors (vn_set_coef_learn, vn_set_source_learn, vn_set_field_learn, vn_set_bic_learn,
vn_set_fluxbc_learn), the periodic pairs, the observations and the per-test-function weights (static and causal) on every GPU
route, against the fp64 restatement of the joint problem tests/joint_ref.py (test infrastructure: plain module, no pytest marks;
shared by tests/test_fuzz_learnt_host.py and tests/test_fuzz_learnt_gpu.py).

Cases: tests/fuzz_terms.draw_case with its draw sequence untouched (a seed names the same net, sizes, terms, flux rows and
`offset` flag as there); this module's own draws come from default_rng([seed, 9000 + case]), always in the same order whatever is
then used.  One case in four is a `weights` case (omega = U(0.25, 4) per test function, or on a time-dependent case with n_k >= 2,
one time in two, causal slabs: n_slabs in 2..6, slab = permutation(arange(n_k) % n_slabs), eps = ln 4 / C_{S-1} of the fp64
reference's own loss field, the rule of tests/causal_cases.py); no vector is learnt there and every set_*_learn call must be
refused with VN_EUNSUPPORTED.  The others are `learn` cases: a non-empty subset of the vectors the case can carry (the flux / Robin
amplitudes only with flux rows); the first case of a list that can carry all five carries all five.  Coefficients: a non-empty
mask over the entries of the registered terms and, one time in two, one entry of a term the batch does not carry, whose gradient
the header documents to read 0 and which the step leaves alone while its slots are zero; the nine start from the terms' own values
rounded to fp32 (a term only batch 1 carries: its values there).  Source J in {1, 3, 8, 9, 17, 64} (has_source = 1 and a zero s0
when the case has no source), field J in {1, 3, 8, 9, 32}, BC/IC J in {1, 3, 9, 64} with streams over all nB rows, flux / Robin
(Jl, Jc) in {(1,0), (0,1), (2,1), (7,2), (8,1), (9,8)}.  Masks: one in two full, else random with at least one entry; for J > 8 one
time in four one whole group of eight is masked out.  Basis streams: the formula of tests/bic_cases.basis (Gaussian bump, wave,
bump times a coordinate) on the coordinates of the rows the stream lives on, for the field times a unit direction per stream;
amplitudes N(0, 1); all rounded to fp32 (generators default_rng([seed, 9500 + case, k])).  With the case's `offset` flag the basis
streams and the base streams a learnt vector mixes from (s0, g0, label0) are registered from views one float off the 16-byte grid;
the flux rows' own coef and label go through the host wrapper, which uploads them aligned.  Independently one case in three gets
periodic pairs (nP in 1..40, gamma in {0, 0.5, 1}, X = U(-1, 1), one N(0, 1) direction per pair) and one in three observations (nO
in 1..50, q / dir / wgt each present or not, rowptr absent or segments of 1..4 points, lambda in {0.5, 2}).  Every fourth case has a
batch 1 as in tests/fuzz_terms.py, with source and field basis streams of its own.

Routes, on the same inputs: AUTO (0), the generic kernels (1) when in range, both forms of the layer-by-layer route (4, 40), the
de-duplicated step (30) on the case's shared-point map, vn_objective_f64 (64) where its range allows.  What a route is documented
to refuse must be refused with VN_EUNSUPPORTED -- the three edge sets (and with the flux rows the flux / Robin amplitudes) outside
VN_KMAX_* and on the layer-by-layer route, the field amplitudes on the layer-by-layer route -- and the case runs there without the
refused piece, against the joint reference without it (one reference per distinct set of pieces).  On networks of the generic
kernels that the 8-wave point pass does not serve the header allows the field amplitudes to be refused: the requested generic
engine must then decide as the AUTO engine of the same net did, and an AUTO engine on the 8-wave kernel must accept.  dim <= 3 always.  In
a weights case the field probe on the layer-by-layer route is refused by the route's own check, which the engine makes first.

Checks per route, at bars that all exist already: loss pieces (eval_loss, gradient tail) at fuzz_routes.LOSS_BAR, lossVec at
LVEC_RTOL, the observation misfit at LOSS_BAR, the theta-gradient at GRAD_BAR / PAIR_BAR with the per-block rule and the whitelist
exactly as fuzz_terms._Judge applies them, every vector gradient per component at |g - g64| <= GRAD_RTOL max(|g64|, COND_FLOOR S_j)
(tests/parity_cases.py, tests/bic_cases.py), masked-out entries exactly 0.0, a second grad the same bits, vn_objective_f64 at the
bars of tests/test_obj64_gpu.py against the joint reference evaluated at the streams the device mixes (fp32, one fused
multiply-add per stream: tests/bic_cases.fma_mix restated).  On the AUTO engine: grad(0), grad(1), grad(0) leaves batch 0's bits,
batch 1 meets the bars against its own joint reference; then one train_step(0): step == 1, every masked-in entry moved (but a
coefficient of a term the batch does not carry, which the header documents to stay while its slots are zero), every masked-out
entry kept its bits; last, where the batch is de-duplicated and carries a flux term or D(u), a table with N_p == 0 makes the step
return the documented VN_EUNSUPPORTED.

Seed lists: three time-dependent, one steady, one MOR-shaped, each the cases 0..n-1 of its seed, n <= 8.  Scanned for the
conditions of tests/test_fuzz_learnt_host.py: time-dependent seeds 0..1599, steady seeds 0..499, MOR seeds 0..499, each with its
longest prefix of cases that all meet every per-case condition (most seeds: one or two cases -- at gcoef x 8 the interior part of
the gradient dwarfs the boundary rows' and the observations', so a case with BC/IC or flux amplitudes, periodic pairs or
observations rarely meets the 10 x GRAD_BAR / 100 x LOSS_BAR conditions); kept: the five lists that together reach every path of
the host tier's reach table with the most cases.  The seeds of tests/fuzz_terms.py (0, 7, 12, 31, 5) were replaced because cases
of theirs miss a condition.

    python -m tests.fuzz_learnt [cases] [seed]      (soak; on the GPU box)
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import fuzz_routes as fz  # noqa: E402
from tests import fuzz_terms as ft  # noqa: E402
from tests import inverse_ref, joint_ref  # noqa: E402
from tests.bic_cases import BINDING_FRAC, COND_FLOOR  # noqa: E402,F401  (the host tier reads its bars from here)
from tests.fuzz_routes import COND_WHITELIST, GRAD_BAR, LOSS_BAR, U32  # noqa: E402,F401
from tests.fuzz_terms import BIDIMVAL, KEYS  # noqa: E402
from tests.parity_cases import GRAD_RTOL  # noqa: E402

VECTORS = joint_ref.VECTORS
GETTERS = dict(coef='coefs', source='source_amps', field='field_amps', bic='bic_amps', fluxbc='fluxbc_amps')
SRC_J, FLD_J, BIC_J = (1, 3, 8, 9, 17, 64), (1, 3, 8, 9, 32), (1, 3, 9, 64)
FBC_J = ((1, 0), (0, 1), (2, 1), (7, 2), (8, 1), (9, 8))
LN4 = float(np.log(4.0))
LR = 0.01

# (seed, cases, steady, mor): the lists of the pytest tiers, at most 8 cases each
SEED_LISTS = [(544, 2, False, False), (543, 1, False, False), (114, 5, False, False), (123, 4, True, False), (347, 5, False, True)]


# ---- cases ----------------------------------------------------------------------------------------------------------
def _mask(r, J):
    full = r.random() < 0.5
    m = (r.random(J) < 0.5).astype(np.int32)
    keep = int(r.integers(0, J))
    group = int(r.integers(0, (J + 7) // 8))
    zero_group = r.random() < 0.25
    if full:
        m[:] = 1
    m[keep] = 1
    if J > 8 and zero_group:
        m[8 * group:8 * group + 8] = 0
        if not m.any():
            m[(8 * group + 8) % J] = 1
    return m


def _amp(r, J):
    return r.standard_normal(J).astype(np.float32).astype(np.float64)


def draw_extras(c, seed):
    """This module's own draws for one case of fuzz_terms.draw_case: always the same sequence, whatever the case then uses."""
    r = np.random.default_rng([seed, 9000 + c['case']])
    d_in, dim = c['d_in'], c['dim']
    x = dict(mode='weights' if r.random() < 0.25 else 'learn')
    has_per, has_obs = r.random() < 1.0 / 3.0, r.random() < 1.0 / 3.0
    nP = int(r.integers(1, 41))
    per = dict(gamma=float(r.choice([0.0, 0.5, 1.0])), X=r.uniform(-1, 1, (2 * nP, d_in)).astype(np.float32),
               dir=np.tile(r.standard_normal((nP, dim)), (2, 1)).astype(np.float32))
    nO = int(r.integers(1, 51))
    seg = r.integers(1, 5, nO) if r.random() < 0.5 else None
    n = nO if seg is None else int(seg.sum())
    flags = r.random(3) < 0.5
    obs = dict(X=r.uniform(-1, 1, (n, d_in)).astype(np.float32), value=r.standard_normal(nO).astype(np.float32),
               q=r.uniform(0.5, 1.5, n).astype(np.float32), dir=r.standard_normal((n, dim)).astype(np.float32),
               wgt=r.uniform(0.5, 2.0, nO).astype(np.float32), lam=float(r.choice([0.5, 2.0])),
               rowptr=None if seg is None else np.concatenate([[0], np.cumsum(seg)]).astype(np.int32))
    for k, on in zip(('q', 'dir', 'wgt'), flags):
        if not on:
            obs[k] = None
    x['periodic'], x['obs'] = per if has_per else None, obs if has_obs else None
    # weights
    x['omega'] = r.uniform(0.25, 4.0, c['n_k']).astype(np.float32)
    S = min(int(r.integers(2, 7)), c['n_k'])
    x['causal'] = (r.permutation(np.arange(c['n_k']) % S).astype(np.int32), S) if (r.random() < 0.5 and c['td'] and c['n_k'] >= 2) else None
    # the five vectors, all drawn
    here = [3 * k + j for k, t in enumerate(('reaction', 'nlflux', 'nldiff')) if t in c['terms'] for j in range(3)]
    away = [i for i in range(9) if i not in here]
    m9 = np.zeros(9, dtype=np.int32)
    pick = r.random(len(here)) < 0.5
    pick[int(r.integers(0, len(here)))] = True
    m9[np.array(here)[pick]] = 1
    stray = int(r.integers(0, max(len(away), 1)))
    if r.random() < 0.5 and away:
        m9[away[stray]] = 1
    v = dict(coef=dict(mask=m9))
    for name, Js in (('source', SRC_J), ('field', FLD_J), ('bic', BIC_J)):
        J = int(r.choice(Js))
        v[name] = dict(J=J, mask=_mask(r, J), amp=_amp(r, J))
    Jl, Jc = FBC_J[int(r.integers(0, len(FBC_J)))]
    v['fluxbc'] = dict(J=Jl + Jc, Jl=Jl, mask=_mask(r, Jl + Jc), amp=_amp(r, Jl + Jc))
    can = [k for k in VECTORS if k != 'fluxbc' or c['flux'] is not None]
    on = [k for k, p in zip(VECTORS, r.random(5) < 0.5) if p and k in can]
    x['can'] = can
    x['learn'] = on if on else [can[int(r.integers(0, len(can)))]]
    x['vec'] = v
    if x['mode'] == 'weights':
        x['learn'] = []
    return x


def draw_case(rng, case, seed, steady=False, mor=False):
    c = ft.draw_case(rng, case, seed, steady, mor)
    c['x'] = draw_extras(c, seed)
    return c


def draw_list(seed, ncases, steady=False, mor=False):
    """The cases of one seed; the first learn case that can carry all five vectors carries all five."""
    rng = np.random.default_rng(seed)
    cs = [draw_case(rng, case, seed, steady, mor) for case in range(ncases)]
    for c in cs:
        if c['x']['mode'] == 'learn' and len(c['x']['can']) == 5:
            c['x']['learn'] = list(VECTORS)
            break
    return cs


def all_cases():
    return [c for lst in SEED_LISTS for c in draw_list(*lst)]


def streams(rng, x, J):
    """[J, rows] fp32: the formula of tests/bic_cases.basis on the coordinates x [rows, dim]."""
    x = np.asarray(x, dtype=np.float64)
    dim = x.shape[1]
    B = np.empty((J, x.shape[0]), dtype=np.float32)
    for j in range(J):
        c, s = rng.uniform(-0.7, 0.7, dim), rng.uniform(0.3, 0.8)
        k, p = rng.uniform(1.0, 3.0, dim), rng.uniform(0.0, 2.0 * np.pi)
        bump = np.exp(-np.sum((x - c) ** 2, axis=1) / (2.0 * s * s))
        kind = 2 if J == 1 else j % 3
        B[j] = (bump, np.sin(x @ k + p), bump * (x[:, 0] - c[0]) / s)[kind]
    return B


def _field_streams(rng, x, J):
    dirs = rng.standard_normal((J, x.shape[1]))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return (streams(rng, x, J)[:, :, None] * dirs[:, None, :]).astype(np.float32)


def nine_of(c):
    """The nine coefficients the engine starts from when they are learnt: batch 0's terms, for a term only batch 1 carries its
    values there, rounded to fp32."""
    t = dict(c['grow']['terms']) if c['grow'] else {}
    t.update(c['terms'])
    return inverse_ref.nine(t.get('nldiff'), t.get('nlflux'), t.get('reaction')).astype(np.float32).astype(np.float64)


def prepare(c, batch=0):
    """Everything of one batch of a case that is data: inputs, shared-point map, bases.  dict(d, dd, n_k, terms, bases)."""
    d, dd = ft.case_inputs(c, batch)
    dim, v = c['dim'], c['x']['vec']
    g = lambda k: np.random.default_rng([c['seed'], 9500 + c['case'], k + 10 * batch])
    xi = d['Input'][:, :dim]
    b = dict(source=streams(g(0), xi, v['source']['J']), field=_field_streams(g(1), xi, v['field']['J']))
    if batch == 0:
        b['bic'] = streams(g(2), d['biInput'][:, :dim], v['bic']['J'])
        if c['flux'] is not None:
            b['fluxbc'] = streams(g(3), c['flux']['X'][:, :dim], v['fluxbc']['J'])
    return dict(d=d, dd=dd, batch=batch, n_k=c['n_k'] if batch == 0 else c['grow']['n_k'], terms=c['terms'] if batch == 0 else c['grow']['terms'],
                bases=b)


def ref_kw(c, d, n_k):
    return dict(Input=d['Input'], gcoef=d['gcoef'], source=d['source'], N=d['N'], dNt=d['dNt'], integW=d['integW'], intShape=[n_k, c['q']],
                detJ=(d['detJ'] if c['djv'] else float(d['detJ'])), detJvec=c['djv'], biInput=d['biInput'], biLabel=d['biLabel'],
                bDof=c['bDof'], biDimVal=BIDIMVAL, w=d['w'], dim=c['dim'], time_dependent=c['td'], is_source=c['src'], integWflag=c['iw'],
                activation=c['act'])


_EPS = {}            # eps of the causal cases, computed once (the case dicts are never modified)


def causal_eps(c, p, flat):
    """ln 4 / C_{S-1} of the fp64 reference's own loss field (tests/causal_cases.eps_of): the smallest weight is 1/4 there."""
    slab, S = c['x']['causal']
    lv = np.asarray(joint_ref.evaluate(flat, c['d_in'], c['widths'], p['terms'], ref_kw(c, p['d'], p['n_k']))[0]['lossVec']).reshape(-1)
    L = np.array([lv[slab == s].mean() if np.any(slab == s) else 0.0 for s in range(S)])
    return LN4 / float(np.sum(L[:-1]))


def weights_of(c, p, flat):
    """(omega, causal) of a weights case as tests/joint_ref.evaluate takes them; (None, None) on a learn case."""
    x = c['x']
    if x['mode'] != 'weights':
        return None, None
    if x['causal'] is None:
        return x['omega'], None
    key = (c['seed'], c['case'], c['td'], c['d_in'])
    if key not in _EPS:
        _EPS[key] = causal_eps(c, p, flat)
    return None, (x['causal'][0], x['causal'][1], _EPS[key])


def pieces_of(c, edges=True, field=True):
    """The pieces an engine carries: names of learnt vectors and edge sets.  edges False: what a route without edge passes keeps;
    field False: without the field amplitudes.  Batch 1 shares the engine-wide sets and vectors."""
    x = c['x']
    ps = set(x['learn'])
    ps.update(k for k in ('periodic', 'obs') if x[k] is not None)
    if c['flux'] is not None:
        ps.add('flux')
    if not edges:
        ps -= {'flux', 'periodic', 'obs', 'fluxbc'}
    if not field:
        ps.discard('field')
    return frozenset(ps)


def reference(c, p, flat, pieces, dtype=torch.float64, amps=None, zero=(), scales=True, weights=True, mixed=False):
    """tests/joint_ref.evaluate of one batch with the pieces named.  amps: {vector: values} in place of the drawn ones; zero: vectors
    evaluated at zero amplitudes (the coefficients: every term with a learnt entry at the values that switch it off); weights False: a weights case
    without its weights; mixed: every learnt stream mixed as the device mixes it (fp32, one fused multiply-add per stream) and
    nothing learnt -- the objective vn_objective_f64 evaluates."""
    x, v, b, d = c['x'], c['x']['vec'], p['bases'], p['d']
    amp = lambda k: np.zeros(v[k]['J']) if k in zero else (v[k]['amp'] if amps is None or k not in amps else np.asarray(amps[k], dtype=np.float64))
    kw = dict(learn_coef='coef' in pieces)
    coef = None
    if 'coef' in pieces:
        coef = nine_of(c) if amps is None or 'coef' not in amps else np.asarray(amps['coef'], dtype=np.float64)
        if 'coef' in zero:                       # every term with a learnt entry: switched off
            off = np.repeat(v['coef']['mask'].reshape(3, 3).any(axis=1), 3)
            coef = np.where(off, np.array(inverse_ref.OFF), coef)
    rk = ref_kw(c, d, p['n_k'])
    if 'source' in pieces:
        kw['source'] = (d['source'], b['source'], amp('source'))
    if 'field' in pieces:
        kw['field'] = (b['field'], amp('field'))
    if 'bic' in pieces:
        kw['bic'] = (b['bic'] if 'bic' in b else prepare(c)['bases']['bic'], amp('bic'))
    if 'flux' in pieces:
        kw['flux'] = dict(c['flux'])
        if 'fluxbc' in pieces:
            S = b['fluxbc'] if 'fluxbc' in b else prepare(c)['bases']['fluxbc']
            kw['flux'].update(S=S, Jl=v['fluxbc']['Jl'], amp=amp('fluxbc'))
    if mixed:
        rk, kw = dict(rk), dict(kw, learn_coef=False)
        if 'source' in kw:
            s0, Phi, a = kw.pop('source')
            rk['source'] = fma_mix(np.zeros(Phi.shape[1], dtype=np.float32) if s0 is None else s0, Phi, a).reshape(-1, 1)
            rk['is_source'] = True
        if 'field' in kw:
            G, a = kw.pop('field')
            rk['gcoef'] = fma_mix(rk['gcoef'], G.reshape(G.shape[0], -1), a).reshape(rk['gcoef'].shape)
        if 'bic' in kw:
            B, a = kw.pop('bic')
            rk['biLabel'] = fma_mix(rk['biLabel'], B, a).reshape(-1, 1)
        if 'S' in kw.get('flux', {}):
            fx = kw['flux']
            S, Jl, a = fx.pop('S'), fx.pop('Jl'), fx.pop('amp')
            if Jl:
                fx['label'] = fma_mix(fx['label'], S[:Jl], a[:Jl])
            if Jl < len(a):
                fx['coef'] = fma_mix(fx['coef'], S[Jl:], a[Jl:])
    if 'periodic' in pieces:
        kw['periodic'] = x['periodic']
    if 'obs' in pieces:
        kw['obs'] = x['obs']
    if weights and p['batch'] == 0:
        kw['omega'], kw['causal'] = weights_of(c, p, flat)
    return joint_ref.evaluate(flat, c['d_in'], c['widths'], p['terms'], rk, dtype, coef=coef, scales=scales, **kw)


def fma_mix(base, B, amp):
    """tests/bic_cases.fma_mix: fp32, from base, j ascending, one fused multiply-add per stream (the product of two fp32 numbers is
    exact in fp64, so each step is one fp64 addition rounded to fp32)."""
    s = np.asarray(base, dtype=np.float32).reshape(-1)
    for j in range(len(amp)):
        s = (np.float64(np.float32(amp[j])) * B[j].astype(np.float64) + s.astype(np.float64)).astype(np.float32)
    return s


def vector_bars(g64, S):
    """The allowed |g - g64| per component (tests/bic_cases.bars)."""
    return GRAD_RTOL * np.maximum(np.abs(g64), COND_FLOOR * S)


def mask_of(c, k):
    return np.asarray(c['x']['vec'][k]['mask']) != 0


def describe(c):
    x, v = c['x'], c['x']['vec']
    lv = ' '.join('%s[%s%s]' % (k, ('%d+%d' % (v[k]['Jl'], v[k]['J'] - v[k]['Jl'])) if k == 'fluxbc' else ('J=%d' % v[k]['J'] if k != 'coef' else ''),
                                ' mask=' + ''.join(str(int(m)) for m in v[k]['mask']) if not np.all(v[k]['mask']) else '') for k in x['learn'])
    w = '' if x['mode'] == 'learn' else (' weights=causal(S=%d)' % x['causal'][1] if x['causal'] is not None else ' weights=static')
    return ft.describe(c) + '%s%s%s {%s}' % (w, ' periodic=%d(gamma %g)' % (len(x['periodic']['X']) // 2, x['periodic']['gamma']) if x['periodic'] else '',
                                             ' obs=%d' % len(x['obs']['value']) if x['obs'] else '', lv)


# ---- the GPU side ---------------------------------------------------------------------------------------------------
def _dev(a, offset, keep):
    """A device stream of a's shape: contiguous, or a view one float off the 16-byte grid."""
    a = np.asarray(a, dtype=np.float32)
    return ft._stream(a, offset, keep).reshape(a.shape)


def _register_batch(eng, c, p, batch, learn, offset, keep):
    """Interior rows, terms and the batch's own bases (source, field) of one batch."""
    d = p['d']
    src = d['source']
    if 'source' in learn and src is None:
        src = np.zeros((d['Input'].shape[0], 1), dtype=np.float32)
    d = dict(d, source=None if src is None else (_dev(src, offset, keep) if 'source' in learn else src),
             gcoef=_dev(d['gcoef'], offset, keep) if 'field' in learn else d['gcoef'])
    ft.register_interior(eng, c, d, batch, p['n_k'])
    ft.register_terms(eng, batch, p['terms'], c['offset'] and batch == 0, keep)
    if 'source' in learn:
        eng.set_source_basis(batch, _dev(p['bases']['source'], offset, keep))
    if 'field' in learn:
        eng.set_field_basis(batch, _dev(p['bases']['field'], offset, keep))


def _vector_state(eng, names, c):
    """{vector: (values, gradient)} of the engine's learnt vectors."""
    return {k: getattr(eng, 'get_' + GETTERS[k])(grad=True, **({} if k == 'coef' else {'J': c['x']['vec'][k]['J']})) for k in names}


def _check_vectors(tag, c, state, vref, rec, fails):
    """Every learnt vector's gradient against the joint reference, per component; masked-out entries exactly 0."""
    for k, (_, g) in state.items():
        g64, S = vref[k]
        on = mask_of(c, k)
        bar = vector_bars(g64, S)
        rel = np.where(on, np.abs(g - g64) / np.maximum(bar, 1e-300), 0.0)
        r = rec.setdefault(k, {})
        r['err_over_bar'] = max(r.get('err_over_bar', 0.0), float(rel.max()))
        if not np.all(np.isfinite(g)) or rel.max() > 1.0:
            j = int(rel.argmax())
            fails.append('%s: %s gradient component %d: %.6e against %.6e (bar %.1e, S %.1e)' % (tag, k, j, g[j], g64[j], bar[j], S[j]))
        if not np.all(g[~on] == 0.0):
            fails.append('%s: %s gradient of a masked-out entry is not 0.0' % (tag, k))


def _learn_args(c, k):
    v = c['x']['vec'][k]
    return (v['mask'], nine_of(c) if k == 'coef' else v['amp'])


def run_case(c):
    """Every route that can take the case.  Returns a result dict: result['ok'] the verdict, result['msg'] a line,
    result['per_route'] {route: {quantity: worst error}}, result['per_vector'] {vector: {route: err / bar}}."""
    from varnet_amd.engine import VN_KERNEL_FUSED16, VN_KERNEL_LAYERED
    x = c['x']
    p0 = prepare(c)
    d, dd = p0['d'], p0['dd']
    flat = ft.theta(c)
    rng_ok = ft.in_kernel_range(c)
    learn = list(x['learn'])
    src_flag = c['src'] or 'source' in learn
    refs, judges = {}, {}

    def ref_of(pieces, p=p0):
        key = (pieces, p['batch'])
        if key not in refs:
            refs[key] = reference(c, p, flat, pieces)
        return refs[key]

    def judge_of(pieces):
        if pieces not in judges:
            res, g, _ = ref_of(pieces)
            judges[pieces] = ft._Judge(c, res, g, lambda: reference(c, p0, flat, pieces, torch.float32, scales=False)[1])
        return judges[pieces]

    kernels = [0]
    if rng_ok:
        try:
            fz.make_engine(c['d_in'], c['dim'], c['widths'], c['q'], src_flag, c['iw'], 1, c['act'], c['td']).close()
            kernels.append(1)
        except Exception:                       # deep + wide: too big for the generic kernels' LDS
            pass
    kernels += [4, 40]
    per_route, per_vector, paths, notes, fails = {}, {}, {}, [], []
    carried = {}                                 # route -> the vectors it ran with
    field_auto = None
    for kernel in kernels:
        eng = fz.make_engine(c['d_in'], c['dim'], c['widths'], c['q'], src_flag, c['iw'], kernel, c['act'], c['td'])
        keep = []
        try:
            eng.set_params(flat)
            eng.set_fe_table(d['N1'], d['dNt1'], d['integW'])
            _register_batch(eng, c, p0, 0, learn, c['offset'], keep)
            eng.set_bic(d['biInput'], _dev(d['biLabel'], c['offset'], keep).reshape(-1) if 'bic' in learn else d['biLabel'], c['bDof'], BIDIMVAL)
            eng.set_weights(d['w'])
            kp = tuple(eng.kernel_path())
            paths[str(kernel)] = list(kp)
            layered = kp[0] == VN_KERNEL_LAYERED
            edges = rng_ok and not layered
            # edge sets: registered, or refused with the documented error
            fx, pr, ob = c['flux'], x['periodic'], x['obs']
            sets = [('flux rows', fx, lambda: eng.set_flux_bc(fx['X'], fx['normal'], fx['coef'], fx['label'], BIDIMVAL)),
                    ('periodic pairs', pr, lambda: eng.set_periodic(pr['X'], pr['dir'], pr['gamma'], BIDIMVAL)),
                    ('observations', ob, lambda: eng.set_observations(ob['X'], ob['value'], ob['q'], ob['dir'], ob['rowptr'], ob['wgt'], ob['lam']))]
            for name, data, call in sets:
                if data is None:
                    continue
                if edges:
                    call()
                elif not ft._refused(call):
                    fails.append('route %d: %s not refused with VN_EUNSUPPORTED' % (kernel, name))
            # weights, and the refusal of every vector next to them
            if x['mode'] == 'weights':
                om, causal = weights_of(c, p0, flat)
                if causal is not None:
                    eng.set_causal(0, causal[0], causal[1], causal[2])
                else:
                    eng.set_tf_weights(0, om)
                for k in VECTORS:
                    J = 9 if k == 'coef' else 1
                    if not ft._refused(lambda: getattr(eng, 'set_%s_learn' % k)([1] * J, np.array(inverse_ref.OFF) if k == 'coef' else np.zeros(J), lr=LR)):
                        fails.append('route %d: set_%s_learn next to weights not refused with VN_EUNSUPPORTED' % (kernel, k))
            # the vectors
            on = []
            for k in learn:
                if k == 'fluxbc' and not edges:
                    continue                     # (its rows were refused above)
                if k == 'bic':
                    eng.set_bic_basis(-1, _dev(p0['bases']['bic'], c['offset'], keep))
                if k == 'fluxbc':
                    eng.set_fluxbc_basis(_dev(p0['bases']['fluxbc'], c['offset'], keep), x['vec'][k]['Jl'])
                call = lambda: getattr(eng, 'set_%s_learn' % k)(*_learn_args(c, k), lr=LR)
                if k == 'field':
                    if layered:
                        if not ft._refused(call):
                            fails.append('route %d: field amplitudes on the layer-by-layer route not refused with VN_EUNSUPPORTED' % kernel)
                        continue
                    taken = not ft._refused(call)
                    if kernel == 0:
                        field_auto = taken
                        if kp[0] == VN_KERNEL_FUSED16 and not taken:
                            fails.append('route 0: field amplitudes refused on the 8-wave kernel')
                    elif kernel == 1 and field_auto is not None and taken != field_auto:
                        fails.append('route %d: field amplitudes %s here, %s under AUTO' % (kernel, *(('taken', 'refused') if taken else ('refused', 'taken'))))
                    if not taken:
                        continue
                else:
                    call()
                on.append(k)
            pieces = pieces_of(c, edges, 'field' in on)
            assert set(on) == set(learn) & pieces, (on, pieces)
            carried[kernel] = on
            ref, gref, vref = ref_of(pieces)
            judge = judge_of(pieces)
            gb = eng.bind_grad_buffer()
            route = kernel
            tag = 'route %d' % route
            g0 = ft.grad_of(eng, gb)
            s0 = _vector_state(eng, on, c)
            judge.add(route, g0)
            rec = per_route.setdefault(str(route), {})
            _check_vectors(tag, c, s0, vref, per_vector.setdefault(str(route), {}), fails)
            for k in on:
                want = nine_of(c) if k == 'coef' else x['vec'][k]['amp']
                if not np.array_equal(s0[k][0], want):
                    fails.append('%s: %s values read back differ from the registered ones' % (tag, k))
            g0b = ft.grad_of(eng, gb)
            s0b = _vector_state(eng, on, c)
            if not (np.array_equal(g0, g0b) and all(np.array_equal(s0[k][1], s0b[k][1]) for k in on)):
                fails.append('%s: a second grad gives other bits' % tag)
            ok, le, ve = ft._check_eval(eng, ref, rec)
            if not ok:
                fails.append('%s: eval_loss %.1e lossVec %.1e' % (tag, le, ve))
            if 'obs' in pieces:
                oe = ft._rel(eng.obs_misfit(), ref['obs'])
                rec['obs'] = max(rec.get('obs', 0.0), oe)
                if oe > LOSS_BAR:
                    fails.append('%s: observation misfit %.1e' % (tag, oe))
            if kernel != 0:
                continue
            # the fp64 objective of the same batch, where the header's range allows: at the streams the device mixes
            if rng_ok and c['dim'] <= 3:
                mixes = bool(set(on) & {'source', 'field', 'bic', 'fluxbc'})
                r64, g64, _ = reference(c, p0, flat, pieces, mixed=True, scales=False) if mixes else (ref, gref, None)
                ok, le, ve, be = ft._check_obj64(eng, c, r64, g64, per_route.setdefault('64', {}))
                notes.append('obj64 %.1e/%.1e/%.1e' % (le, ve, be))
                if not ok:
                    fails.append('objective64: loss %.1e lossVec %.1e gradient block %.1e' % (le, ve, be))
            elif not ft._refused(lambda: eng.objective64(0, grad=True)):
                fails.append('objective64 not refused with VN_EUNSUPPORTED')
            # buffer growth: a larger batch 1 with bases of its own between two evaluations of batch 0
            if c['grow'] is not None:
                p1 = prepare(c, 1)
                _register_batch(eng, c, p1, 1, on, False, keep)
                pieces1 = pieces
                ref1, gref1, vref1 = ref_of(pieces1, p1)
                j1 = ft._Judge(c, ref1, gref1, lambda: reference(c, p1, flat, pieces1, torch.float32, scales=False)[1])
                g1 = ft.grad_of(eng, gb, 1)
                s1 = _vector_state(eng, on, c)
                j1.add(route, g1)
                _check_vectors('batch 1', c, s1, vref1, per_vector.setdefault('grow', {}), fails)
                again = ft.grad_of(eng, gb, 0)
                sa = _vector_state(eng, on, c)
                tmp = {}
                grow = j1.verdict(tmp)
                per_route['grow'] = tmp[str(route)]
                bitwise = bool(np.array_equal(g0, again) and all(np.array_equal(s0[k][1], sa[k][1]) for k in on))
                notes.append('grow n_k=%d %.1e/%.1e%s' % (p1['n_k'], grow['gerr'], grow['lerr'], '' if bitwise else ' NOT BITWISE'))
                if not (grow['ok'] and bitwise):
                    fails.append('buffer growth: batch 1 gradient %.1e loss %.1e, batch 0 bitwise %s' % (grow['gerr'], grow['lerr'], bitwise))
            # the de-duplicated step on the shared-point map
            if dd is not None and eng.dedup_supported():
                eng.set_dedup(0, *dd)
                gd = ft.grad_of(eng, gb)
                sd = _vector_state(eng, on, c)
                judge.add(30, gd)
                carried[30] = on
                _check_vectors('route 30', c, sd, vref, per_vector.setdefault('30', {}), fails)
                gd2 = ft.grad_of(eng, gb)
                sd2 = _vector_state(eng, on, c)
                if not (np.array_equal(gd, gd2) and all(np.array_equal(sd[k][1], sd2[k][1]) for k in on)):
                    fails.append('route 30: a second grad gives other bits')
                rec30 = per_route.setdefault('30', {})
                ok, le, ve = ft._check_eval(eng, ref, rec30)
                if not ok:
                    fails.append('route 30: eval_loss %.1e lossVec %.1e' % (le, ve))
                if 'obs' in pieces:
                    oe = ft._rel(eng.obs_misfit(), ref['obs'])
                    rec30['obs'] = max(rec30.get('obs', 0.0), oe)
                    if oe > LOSS_BAR:
                        fails.append('route 30: observation misfit %.1e' % oe)
            # one step: the counter moves, masked-in entries move, masked-out entries keep their bits
            if on:
                before = _vector_state(eng, on, c)
                eng.grad(0)
                torch.cuda.synchronize()
                gnow = _vector_state(eng, on, c)
                eng.train_step(0)
                torch.cuda.synchronize()
                after = _vector_state(eng, on, c)
                if eng.step != 1:
                    fails.append('train_step: step counter %d' % eng.step)
                for k in on:
                    live = mask_of(c, k)
                    if k == 'coef':              # (a term the batch does not carry: gradient 0, and with zero slots the entry stays)
                        gone = np.repeat([t not in c['terms'] for t in ('reaction', 'nlflux', 'nldiff')], 3)
                        if not np.all(gnow[k][1][gone] == 0.0):
                            fails.append('train_step: the gradient of a coefficient whose term the batch does not carry is not 0.0')
                        live = live & ~gone
                    if not np.all(after[k][0][live] != before[k][0][live]):
                        fails.append('train_step: a masked-in entry of %s did not move' % k)
                    if not np.array_equal(after[k][0][~live], before[k][0][~live]):
                        fails.append('train_step: an entry of %s that is masked out (or belongs to a term the batch does not carry) moved' % k)
            # the documented refusal of the de-duplicated step on a table with N_p == 0 (flux term or D(u) on the batch)
            if 30 in carried and ({'nlflux', 'nldiff'} & set(c['terms'])):
                N0 = d['N1'].copy()
                N0[0] = 0.0
                eng.set_fe_table(N0, d['dNt1'], d['integW'])
                if not ft._refused(lambda: eng.grad(0)):
                    fails.append('route 30: a table with N_p == 0 not refused with VN_EUNSUPPORTED')
                else:
                    notes.append('N_p == 0 refused')
        finally:
            eng.close()
            del keep
    groups = [j for j in judges.values() if j.grads]
    verdicts = [j.verdict(per_route) for j in groups]
    routes = [r for j in groups for r in j.routes]
    ok = all(v['ok'] for v in verdicts) and not fails
    res = dict(case=c['case'], seed=c['seed'], routes=routes, carried={str(k): v for k, v in carried.items()}, per_route=per_route,
               per_vector=per_vector, paths=paths, verdicts=verdicts, ok=bool(ok), fails=fails,
               cond=max((v['cond'] for v in verdicts if v['cond'] is not None), default=None))
    msg = describe(c) + ' routes=%s:' % routes
    for v in verdicts:
        msg += '  pair %.1e/%.1e pair/block %.1e ref %.1e/%.1e ref/block %.1e (%s)' % (
            v['pair'], v['lpair'], v['pair_block_err'], v['gerr'], v['lerr'], v['gerr_block_err'], v['gerr_block'])
        if v['cond'] is not None:
            msg += ' cond %.1e%s' % (v['cond'], ' (whitelisted)' if v['cond'] > COND_WHITELIST else '')
    msg += '  vectors err/bar ' + ', '.join('%s:%s %.2f' % (r, k, e['err_over_bar']) for r, pv in per_vector.items() for k, e in pv.items())
    msg += '  ' + '  '.join(notes)
    if not ok:
        msg += '   <<<<<<<< MISMATCH ' + '; '.join(fails)
        save_mismatch(c, p0, flat, groups)
    res['msg'] = msg
    return res


def save_mismatch(c, p, flat, groups):
    """The case in the shape of fuzz_terms' fuzz_terms_mismatch.npz, with the bases, masks, amplitudes and edge sets added."""
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(ROOT, 'profile_out')
    os.makedirs(out, exist_ok=True)
    z = lambda a: np.zeros(0) if a is None else np.asarray(a)
    x = c['x']
    extra = {}
    for name, (stream, coef) in c['terms'].items():
        extra['term_%s_stream' % name], extra['term_%s_coef' % name] = z(stream), np.asarray(coef)
    for k, v in (c['flux'] or {}).items():
        extra['flux_' + k] = v
    for s in ('periodic', 'obs'):
        for k, v in (x[s] or {}).items():
            extra['%s_%s' % (s, k)] = z(v)
    for k in x['learn']:
        extra['vec_%s_mask' % k] = x['vec'][k]['mask']
        if k != 'coef':
            extra['vec_%s_amp' % k], extra['vec_%s_basis' % k] = x['vec'][k]['amp'], p['bases'][k]
    np.savez(os.path.join(out, 'fuzz_learnt_mismatch.npz'), widths=np.array(c['widths']), d_in=c['d_in'], dim=c['dim'], q=c['q'],
             n_k=c['n_k'], nB=c['nB'], bDof=c['bDof'], td=c['td'], src=c['src'], iw=c['iw'], djv=c['djv'], rows=c['rows'], act=c['act'],
             flat=flat, seed=c['seed'], case=c['case'], offset=c['offset'], mode=x['mode'], learn=np.array(x['learn'], dtype='U8'),
             routes=np.array([r for j in groups for r in j.routes]), grads=np.array([g for j in groups for g in j.grads]),
             **extra, **{'d_' + k: z(v) for k, v in p['d'].items()})


def merge_record(record, res):
    """Worst error per route and quantity, per route and vector, and the kernel paths seen per requested kernel."""
    for route, rec in res['per_route'].items():
        tgt = record.setdefault('routes', {}).setdefault(route, {})
        for k, v in rec.items():
            tgt[k] = max(tgt.get(k, 0.0), float(v))
    for route, pv in res['per_vector'].items():
        for k, e in pv.items():
            tgt = record.setdefault('vectors', {}).setdefault(k, {})
            tgt[route] = max(tgt.get(route, 0.0), float(e['err_over_bar']))
    for v in res['verdicts']:
        if v['cond'] is None or v['cond'] <= COND_WHITELIST:
            record['pair'] = max(record.get('pair', 0.0), float(v['pair']))
    for kernel, kp in res['paths'].items():
        seen = record.setdefault('kernel_paths', {}).setdefault(kernel, [])
        if kp not in seen:
            seen.append(kp)
            seen.sort()
    for route, names in res['carried'].items():
        for k in names:
            got = record.setdefault('vector_routes', {}).setdefault(k, [])
            if int(route) not in got:
                got.append(int(route))
                got.sort()


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
    print('all %d cases agree (seed %d, %.0f s); %d ill-conditioned draws whitelisted by their condition estimate; worst per route: %s; '
          'worst err/bar per vector: %s' % (ncases, seed, time.time() - t0, n_wl, record.get('routes'), record.get('vectors')))


if __name__ == '__main__':
    main()
