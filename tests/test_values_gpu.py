"""GPU tier of the value-regime parity suite (tests/value_cases.py): every step route, the point kernels and one optimizer step
at saturated, offset, scaled and near-zero values, against the fp64 oracle.  The bars are those of the suites that check the same
routes at the usual operating point, unchanged: loss components 1e-5 purely relative (no absolute floor; a reference term that is
exactly 0 must come back as 0), lossVec and gradient 1e-4 (globally and per block, tests/gradcheck.py with its fp32 rule),
routes pairwise 3e-4, two consecutive grad calls bitwise equal, every output finite, the fp64 objective at 1e-12 / 1e-11
(tests/test_obj64_gpu.py), the point kernels at 2e-6 / 2e-5 / 1e-4 and 1e-13 / 1e-11 (tests/test_fuzz_points_gpu.py).
tests/test_values_host.py shows on the CPU that the fp32 oracle keeps a quarter of these bars on every case.

A case that misses a gradient bar by the activation formula alone -- the route stays within 2 x the deviation of the formula's
float32 restatement (value_cases.kernel_formula) on the same block -- is kept in KNOWN_MISSES as a strict expected failure with
its numbers, and so is a point case whose u stays within 2 x the restatement's deviation (POINT_KNOWN_MISSES); any other miss fails
the test (a known case raises UnexpectedMiss for it, which the xfail mark does not cover), and so does a known route that stops
missing.  test_the_nets_reach_every_route holds the known misses to 5 % of the combinations and to steep4 / offset100 / shrunk.

The worst error per transform, route and quantity is written to values_parity.json in the directory VN_RECORD_DIR names
(default: profile_out/ beside tests/; the committed copy: profiles/values_parity.json)."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import fuzz_routes as fz  # noqa: E402
from tests import value_cases as vc  # noqa: E402
from tests.gradcheck import assert_grad_close, assert_pair_close, block_errors, column_errors, fp32_deviation, global_error  # noqa: E402
from tests.parity_cases import GRAD_RTOL, LOSS_RTOL, LVEC_RTOL  # noqa: E402

KEYS = ('loss', 'BCloss', 'ICloss', 'varLoss')
OBJ_GRAD_BAR, OBJ_LVEC_BAR, OBJ_LOSS_BAR = 1e-11, 1e-11, 1e-12       # tests/test_obj64_gpu.py
KMAX_LAYERS, KMAX_WIDTH, KMAX_DIN = 6, 64, 8
RECORD = {}


class UnexpectedMiss(Exception):
    """A miss that is not a recorded property of the activation formula."""


# (net, transform, activation) -> (routes that miss the gradient bar, what was measured on an MI355X: the worst block of the worst
# route | the float32 restatement of the activation formula on that block).  All of them are tanh at |z| << 1: tanh = 2 sigmoid(2z)
# - 1 carries an absolute error of one ulp of 0.5 whatever the size of tanh z, so a gradient block that is a sum of small activations
# (the last hidden layer's weights, the output weights) loses the relative bar; the GEMM form of the layer-by-layer route (tanhf)
# and the fp64 objective keep it on every one of these cases.
ROUTES4 = ('fused16', 'dedup', 'generic', 'tiles')
KNOWN_MISSES = {
    ('3x20', 'shrunk', 'tanh'): (ROUTES4, 'W3 5.02e-03 on dedup | formula restatement 5.03e-03; Wo 1.05e-03 | 1.05e-03'),
    ('2x32', 'shrunk', 'tanh'): (ROUTES4, 'Wo 6.93e-04 on dedup | formula restatement 6.07e-04; W2 1.33e-04 | 1.35e-04'),
    ('5x50', 'shrunk', 'tanh'): (ROUTES4, 'Wo 5.50e-04 on fused16 | formula restatement 5.49e-04; W5 3.48e-04 | 3.48e-04'),
    ('40_50_34', 'shrunk', 'tanh'): (ROUTES4, 'Wo 5.86e-04 on fused16 | formula restatement 5.86e-04; W3 2.59e-04 | 2.51e-04'),
    ('4x60', 'shrunk', 'tanh'): (ROUTES4, 'Wo 6.10e-04 on dedup | formula restatement 6.10e-04; W4 2.74e-04 | 2.74e-04'),
    ('2x64', 'shrunk', 'tanh'): (ROUTES4, 'Wo 3.41e-03 on dedup | formula restatement 3.41e-03; W2 1.28e-04 | 1.27e-04'),
    ('3x50_q216', 'shrunk', 'tanh'): (ROUTES4, 'Wo 7.52e-04 on generic | formula restatement 7.52e-04; W3 6.11e-04 | 6.11e-04'),
    ('4x50_mor', 'shrunk', 'tanh'): (ROUTES4, 'Wo 6.05e-04 on fused16 | formula restatement 6.05e-04; W4 3.00e-04 | 3.00e-04'),
    ('5x50_steady', 'shrunk', 'tanh'): (ROUTES4, 'Wo 6.14e-04 on generic | formula restatement 6.14e-04; W5 2.95e-04 | 2.95e-04'),
    ('2x96', 'shrunk', 'tanh'): (('tiles',), 'Wo 1.48e-03 on tiles | formula restatement 1.48e-03'),
}

# (net, transform, activation, n) -> (point routes that miss, what was measured): u at inputs offset by 100 under tanh.  Not the
# activation formula but the first layer's cancellation in float32: the fp32 oracle itself misses the 2e-6 bar there (CPU).
BOTH = ('auto', 'per_thread')
POINT_KNOWN_MISSES = {
    ('3x20', 'offset100', 'tanh', 17): (BOTH, 'u 2.53e-06 auto, 2.53e-06 per thread | fp32 oracle 6.53e-06, formula restatement 6.46e-06'),
    ('3x20', 'offset100', 'tanh', 128): (BOTH, 'u 3.02e-06 auto, 3.02e-06 per thread | fp32 oracle 5.63e-06, formula restatement 5.60e-06'),
    ('3x20', 'offset100', 'tanh', 1000): (BOTH, 'u 3.52e-06 auto, 3.52e-06 per thread | fp32 oracle 6.78e-06, formula restatement 6.87e-06'),
    ('5x50', 'offset100', 'tanh', 17): (BOTH, 'u 2.93e-06 auto, 2.93e-06 per thread | fp32 oracle 2.70e-06, formula restatement 2.34e-06'),
    ('5x50', 'offset100', 'tanh', 128): (BOTH, 'u 4.16e-06 auto, 4.22e-06 per thread | fp32 oracle 4.21e-06, formula restatement 4.45e-06'),
    ('5x50', 'offset100', 'tanh', 1000): (BOTH, 'u 4.26e-06 auto, 4.56e-06 per thread | fp32 oracle 4.78e-06, formula restatement 4.84e-06'),
    ('2x64', 'offset100', 'tanh', 17): (BOTH, 'u 2.19e-06 auto, 2.49e-06 per thread | fp32 oracle 2.69e-06, formula restatement 2.75e-06'),
    ('2x64', 'offset100', 'tanh', 128): (BOTH, 'u 3.42e-06 auto, 3.42e-06 per thread | fp32 oracle 4.21e-06, formula restatement 4.06e-06'),
    ('2x64', 'offset100', 'tanh', 1000): (BOTH, 'u 3.39e-06 auto, 3.51e-06 per thread | fp32 oracle 5.16e-06, formula restatement 5.13e-06'),
    ('4x60', 'offset100', 'tanh', 17): (BOTH, 'u 2.20e-06 auto, 2.23e-06 per thread | fp32 oracle 2.94e-06, formula restatement 2.92e-06'),
    ('4x60', 'offset100', 'tanh', 128): (BOTH, 'u 2.56e-06 auto, 2.64e-06 per thread | fp32 oracle 4.46e-06, formula restatement 4.43e-06'),
    ('4x60', 'offset100', 'tanh', 1000): (BOTH, 'u 3.71e-06 auto, 3.71e-06 per thread | fp32 oracle 6.15e-06, formula restatement 6.03e-06'),
}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'values_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def note(transform, route, **q):
    rec = RECORD.setdefault(transform, {}).setdefault(route, {})
    for k, v in q.items():
        rec[k] = max(rec.get(k, 0.0), float(v))


def make(net, act, kernel, **kw):
    d_in, dim, widths, q, n_k, td = vc.NETS[net]
    if kw:
        from varnet_amd.engine import VNEngine
        return VNEngine(dim, d_in, widths, td, q, isSource=True, integWflag=False, kernel=kernel, activationFun=act, **kw)
    return fz.make_engine(d_in, dim, widths, q, True, False, kernel, act, td)


def feed(eng, net, transform):
    d = vc.inputs(net, transform)[0]
    eng.set_params(vc.theta(net, transform))
    eng.set_fe_table(d['N1'], d['dNt1'], None)
    eng.set_interior(0, d['Input'], d['gcoef'], d['source'], n_k=vc.NETS[net][4], detJ=d['detJ'])
    eng.set_bic(d['biInput'], d['biLabel'], vc.BDOF, vc.BIDIMVAL)
    eng.set_weights(d['w'])


def fused32_instantiated(net, act):
    """The 4-wave kernel's table (tests/test_engine_gpu._skip_unsupported): sigmoid only."""
    d_in, dim, widths, q, n_k, td = vc.NETS[net]
    hm, L = max(widths), len(widths)
    return act == 'sigmoid' and not (q > 128 or hm > 50 or (hm > 20 and L < 2) or (hm > 32 and L < 3) or L > (5 if hm > 32 else 4))


def step_engines(net, act):
    """(route name, engine) of every step route that can run the net, fed by the caller; engines the library refuses are left out
    (test_the_nets_reach_every_route says which route must exist where)."""
    from varnet_amd.engine import VNError, VN_KERNEL_FUSED16
    d_in, dim, widths, q, n_k, td = vc.NETS[net]
    in_range = len(widths) <= KMAX_LAYERS and max(widths) <= KMAX_WIDTH and d_in <= KMAX_DIN
    out = []
    for name, kernel, may in (('fused16', 3, in_range), ('fused32', 2, fused32_instantiated(net, act)), ('generic', 1, in_range),
                              ('tiles', 4, True), ('gemm', 40, True)):
        if not may:
            continue
        try:
            eng = make(net, act, kernel)
        except VNError:
            if kernel in (4, 40):
                raise
            continue
        if kernel == 3 and eng.kernel_path()[0] != VN_KERNEL_FUSED16:
            eng.close()
            continue
        out.append((name, eng))
    return out


def run_grad(eng):
    gb = eng.bind_grad_buffer()
    eng.grad(0)
    torch.cuda.synchronize()
    g1 = gb.cpu().numpy().copy()
    eng.grad(0)
    torch.cuda.synchronize()
    return g1, gb.cpu().numpy().copy()


def check_route(fails, route, transform, ref, gref, g32, dims, out, lv, g1, g2):
    """One fp32 route against the fp64 oracle: appends (route, kind, text) per miss, notes the figures."""
    d_in, dim, widths, td = dims
    P = gref.size
    bad = lambda kind, text: fails.append((route, kind, text))
    lvn = lv.cpu().numpy().astype(np.float64)
    if not (np.all(np.isfinite(out)) and np.all(np.isfinite(lvn)) and np.all(np.isfinite(g1))):
        bad('finite', 'non-finite output')
        return
    lerr = 0.0
    for got, key in zip(list(out) + [float(g1[P])], KEYS + ('loss',)):
        if ref[key] == 0.0:
            if got != 0.0:
                bad('loss', '%s = %r where the reference is exactly 0' % (key, got))
            continue
        e = abs(got - ref[key]) / abs(ref[key])
        lerr = max(lerr, e)
        if e > LOSS_RTOL:
            bad('loss', '%s off by %.3e > %.1e (%r against %r)' % (key, e, LOSS_RTOL, got, ref[key]))
    lref = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1)
    lverr = float(np.max(np.abs(lvn - lref)) / np.max(np.abs(lref)))
    if lverr > LVEC_RTOL:
        bad('lvec', 'lossVec off by %.3e > %.1e' % (lverr, LVEC_RTOL))
    errs = block_errors(g1, gref, d_in, widths, dim, td)
    worst = max(errs, key=errs.get)
    note(transform, route, loss=lerr, lossVec=lverr, grad=global_error(g1[:P], gref), grad_block=errs[worst])
    try:
        assert_grad_close(g1, gref, d_in, widths, GRAD_RTOL, g32=g32, dim=dim, td=td, what=route)
    except AssertionError as e:
        bad('grad', str(e))
    if not np.array_equal(g1, g2):
        bad('bitwise', 'two grad calls differ in %d entries' % int(np.sum(g1 != g2)))


def check_obj64(fails, route, transform, ref, gref, dims, out, g, lv):
    d_in, dim, widths, td = dims
    bad = lambda kind, text: fails.append((route, kind, text))
    gn, lvn = g.cpu().numpy(), lv.cpu().numpy()
    if not (np.all(np.isfinite(out)) and np.all(np.isfinite(gn)) and np.all(np.isfinite(lvn))):
        bad('finite', 'non-finite output')
        return
    lerr = 0.0
    for got, key in zip(out, KEYS):
        e = abs(got) if ref[key] == 0.0 else abs(got - ref[key]) / abs(ref[key])
        lerr = max(lerr, e)
        if e > OBJ_LOSS_BAR:
            bad('loss', '%s off by %.3e > %.1e' % (key, e, OBJ_LOSS_BAR))
    lref = np.asarray(ref['lossVec'], dtype=np.float64).reshape(-1)
    lverr = float(np.max(np.abs(lvn - lref)) / np.max(np.abs(lref)))
    if lverr > OBJ_LVEC_BAR:
        bad('lvec', 'lossVec off by %.3e > %.1e' % (lverr, OBJ_LVEC_BAR))
    errs = block_errors(gn, gref, d_in, widths, dim, td)
    worst = max(errs, key=errs.get)
    if errs[worst] > OBJ_GRAD_BAR:
        bad('grad', 'block %s off by %.3e > %.1e' % (worst, errs[worst], OBJ_GRAD_BAR))
    note(transform, route, loss=lerr, lossVec=lverr, grad_block=errs[worst])


def run_objective64(eng, net, transform):
    """objective64 at the case's parameters, or None where the entry point refuses the net (outside its range)."""
    from varnet_amd.engine import VNError
    try:
        return eng.objective64(0, theta=vc.theta(net, transform).astype(np.float64), grad=True, lossVec=True)
    except VNError:
        return None


STEP_CASES = [(n, t, a) for n in vc.NETS for t in vc.TRANSFORMS for a in vc.ACTS]


def _marked(cases):
    return [pytest.param(*c, marks=pytest.mark.xfail(strict=True, raises=AssertionError, reason='%s: %s' % (
        ', '.join(KNOWN_MISSES[c][0]), KNOWN_MISSES[c][1]))) if c in KNOWN_MISSES else c for c in cases]


@pytest.mark.parametrize('net,transform,act', _marked(STEP_CASES))
def test_step_routes(net, transform, act):
    d_in, dim, widths, q, n_k, td = vc.NETS[net]
    dims = (d_in, dim, widths, td)
    ref, gref = vc.oracle(net, transform, act)
    g32 = lambda: vc.oracle(net, transform, act, False)[1]
    P = gref.size
    fails, grads, blocks = [], {}, {}
    obj_done = False
    for route, eng in step_engines(net, act):
        try:
            feed(eng, net, transform)
            out, lv = eng.eval_loss(0, lossVec=True)
            g1, g2 = run_grad(eng)
            check_route(fails, route, transform, ref, gref, g32, dims, out, lv, g1, g2)
            grads[route] = g1
            if route == 'fused16' and eng.dedup_supported():
                eng.set_dedup(0, *vc.inputs(net, transform)[1])
                out, lv = eng.eval_loss(0, lossVec=True)
                g1, g2 = run_grad(eng)
                check_route(fails, 'dedup', transform, ref, gref, g32, dims, out, lv, g1, g2)
                grads['dedup'] = g1
                eng.set_dedup(0)
            if not obj_done:
                res = run_objective64(eng, net, transform)
                obj_done = True
                if res is not None:
                    check_obj64(fails, 'obj64', transform, ref, gref, dims, *res)
        finally:
            eng.close()
    names = list(grads)
    dev32 = lambda: fp32_deviation(g32(), gref, d_in, widths, dim, td)
    for i, a in enumerate(names):
        if not np.all(np.isfinite(grads[a])):
            continue
        blocks[a] = block_errors(grads[a], gref, d_in, widths, dim, td)
        for b in names[:i]:
            if not np.all(np.isfinite(grads[b])):
                continue
            pe = max(global_error(grads[a][:P], grads[b][:P]), max(block_errors(grads[a], grads[b], d_in, widths, dim, td).values()))
            note(transform, a, pair=pe)
            note(transform, b, pair=pe)
            try:
                assert_pair_close(grads[a], grads[b], d_in, widths, fz.PAIR_BAR, dev32=dev32, dim=dim, td=td, what='%s against %s' % (a, b))
            except AssertionError as e:
                fails.append(('%s|%s' % (a, b), 'pair', str(e)))
    for f in fails:
        print('MISS %s %s %s: %s %s: %s' % ((net, transform, act) + f))
    _verdict((net, transform, act), fails, blocks, gref, dims)


def _verdict(key, fails, blocks, gref, dims):
    """No miss: pass.  A case of KNOWN_MISSES: its routes must miss the gradient bar (and nothing else) within 2 x the formula
    restatement's deviation per block, no other route may miss anything -> AssertionError (the strict xfail); else UnexpectedMiss."""
    known = KNOWN_MISSES.get(key, ((), ''))[0]
    d_in, dim, widths, td = dims
    if fails or known:
        yard = block_errors(vc.kernel_formula(*key)[1], gref, d_in, widths, dim, td)
        RECORD.setdefault('misses', {})['%s %s %s' % key] = {
            r: {b: [e, yard[b]] for b, e in blocks[r].items() if e > GRAD_RTOL} for r in sorted({f[0] for f in fails if f[1] == 'grad'})}
    if not known:
        assert not fails, '\n'.join('%s %s: %s' % f for f in fails)
        return
    unexpected = []
    for route, kind, text in fails:
        involved = route.split('|')
        if kind == 'pair' and any(r in known for r in involved):
            continue                            # a route with a known miss also differs from the routes without one
        if kind == 'grad' and route in known:
            continue
        unexpected.append('%s %s: %s' % (route, kind, text))
    missed = {r for r, kind, _ in fails if kind == 'grad'}
    unexpected += ['%s no longer misses the gradient bar' % r for r in known if r not in missed]
    for r in known:
        for b, e in blocks.get(r, {}).items():
            if e > GRAD_RTOL and e > 2.0 * yard[b]:
                unexpected.append('%s block %s off by %.3e, more than 2 x the formula restatement (%.3e)' % (r, b, e, yard[b]))
    if unexpected:
        raise UnexpectedMiss('\n'.join(unexpected))
    raise AssertionError('known misses of the activation formula: ' + '; '.join(
        '%s %s' % (r, {b: '%.2e (formula %.2e)' % (e, yard[b]) for b, e in blocks[r].items() if e > GRAD_RTOL}) for r in known))


@pytest.mark.parametrize('net,act', [(n, a) for n in vc.NETS for a in vc.ACTS])
def test_objective64_planted800(net, act):
    """Biases of +-800 / +-1600: exp overflows in double, the fp64 objective stays finite and at its bars."""
    d_in, dim, widths, q, n_k, td = vc.NETS[net]
    eng = make(net, act, 0)
    try:
        feed(eng, net, 'planted800')
        res = run_objective64(eng, net, 'planted800')
        if res is None:
            assert len(widths) > KMAX_LAYERS or max(widths) > KMAX_WIDTH
            return
        fails = []
        check_obj64(fails, 'obj64', 'planted800', *vc.oracle(net, 'planted800', act), (d_in, dim, widths, td), *res)
        assert not fails, fails
    finally:
        eng.close()


def test_the_nets_reach_every_route():
    """What the net table turns into on the device, from the engines' own answers (no step is run)."""
    from varnet_amd.engine import VN_KERNEL_FUSED16, VN_KERNEL_LAYERED
    seen = {}
    for net in vc.NETS:
        for act in vc.ACTS:
            engs = step_engines(net, act)
            s = seen.setdefault((net, act), set())
            for route, eng in engs:
                s.add(route)
                if route == 'fused16':
                    s.add('twopass' if eng.kernel_path()[1] else 'onepass')
                    if eng.dedup_supported():
                        s.add('dedup')
                eng.close()
            auto = make(net, act, 0)
            s.add('auto%d' % auto.kernel_path()[0])
            auto.close()
    print({'%s %s' % k: sorted(v) for k, v in seen.items()})
    for act in vc.ACTS:
        for net in ('3x20', '2x32', '5x50', '40_50_34', '4x60', '2x64', '4x50_mor', '5x50_steady'):
            assert {'fused16', 'onepass', 'dedup', 'generic', 'tiles', 'gemm', 'auto%d' % VN_KERNEL_FUSED16} <= seen[(net, act)], (net, act)
        assert {'fused16', 'twopass', 'dedup'} <= seen[('3x50_q216', act)]
        for net in ('2x96', '272_260'):
            assert seen[(net, act)] == {'tiles', 'gemm', 'auto%d' % VN_KERNEL_LAYERED}, (net, act)
    assert 'fused32' in seen[('3x20', 'sigmoid')] and 'fused32' in seen[('5x50', 'sigmoid')]
    assert not any('fused32' in seen[(net, 'tanh')] for net in vc.NETS)
    # the known misses: none on a transform whose arithmetic leaves no excuse, and at most 5 % of the (net, transform, activation,
    # route) combinations, the point kernels' included (two point routes per case, the point counts not multiplied in)
    step_routes = {'fused16', 'fused32', 'dedup', 'generic', 'tiles', 'gemm'}
    obj64 = lambda net: len(vc.NETS[net][2]) <= KMAX_LAYERS and max(vc.NETS[net][2]) <= KMAX_WIDTH      # objective64's range
    total = sum(len(s & step_routes) + obj64(net) for (net, _), s in seen.items()) * len(vc.TRANSFORMS)
    total += len(vc.POINT_NETS) * len(vc.POINT_TRANSFORMS) * len(vc.ACTS) * 2
    point_known = {k[:3]: v[0] for k, v in POINT_KNOWN_MISSES.items()}
    known = sum(len(v[0]) for v in KNOWN_MISSES.values()) + sum(len(v) for v in point_known.values())
    print('known misses: %d of %d combinations (%.1f %%)' % (known, total, 100.0 * known / total))
    assert all(k[1] in ('steep4', 'offset100', 'shrunk') for k in list(KNOWN_MISSES) + list(POINT_KNOWN_MISSES))
    assert known <= 0.05 * total


# -- point kernels ---------------------------------------------------------------------------------------------------------------

POINT_CASES = [(n, t, a, k) for n in vc.POINT_NETS for t in vc.POINT_TRANSFORMS + ('planted800',) for a in vc.ACTS for k in vc.POINT_N]


@pytest.mark.parametrize('net,transform,act,n', [
    pytest.param(*c, marks=pytest.mark.xfail(strict=True, raises=AssertionError, reason=POINT_KNOWN_MISSES[c][1]))
    if c in POINT_KNOWN_MISSES else c for c in POINT_CASES])
def test_point_kernels(net, transform, act, n):
    """forward, forward_grad and residual on both point routes (debug_point_route), forward_f64 and residual(fp64=True), at the
    bars of tests/test_fuzz_points_gpu.py with its per-column rule; planted800 on the fp64 entry points only."""
    from varnet_amd.engine import VNEngine
    d_in, dim, widths = vc.POINT_NETS[net]
    c = vc.point_case(net, transform, act, n)
    uref, gref, rref = c['uref'], c['gref'], c['rref']
    su, sg, sr = max(1.0, np.abs(uref).max()), max(1e-30, np.abs(gref).max()), max(1.0, np.abs(rref).max())
    eng = VNEngine(dim, d_in, widths, True, 16, activationFun=act)
    try:
        eng.set_params(c['flat'])
        args = (c['diff'], c['vel'], c['src'], c['ddx'])
        fails = []
        for per_thread in (False, True):
            eng.debug_point_route(per_thread)
            tag = 'per_thread' if per_thread else 'auto'
            u64 = eng.forward_f64(c['X']).cpu().numpy()
            u64r, r64 = (t.cpu().numpy() for t in eng.residual(c['X'], *args, fp64=True))
            e = {'u64': max(np.abs(u64 - uref).max(), np.abs(u64r - uref).max()) / su, 'res64': np.abs(r64 - rref).max() / sr}
            bars = {'u64': 1e-13, 'res64': 1e-11}
            outs = [u64, u64r, r64]
            if transform != 'planted800':
                u, g = (t.cpu().numpy() for t in eng.forward_grad(c['X32']))
                uf = eng.forward(c['X32']).cpu().numpy()
                ur, r = (t.cpu().numpy() for t in eng.residual(c['X32'], *args, fp64=False))
                outs += [u, g, uf, ur, r]
                cols = column_errors(g, gref)
                e.update(u=max(np.abs(u - uref).max(), np.abs(uf - uref).max(), np.abs(ur - uref).max()) / su,
                         grad=np.abs(g - gref).max() / sg, grad_column=max(cols), res=np.abs(r - rref).max() / sr)
                bars.update(u=2e-6, grad=2e-5, res=1e-4)
                if per_thread:
                    e['res_vs_pointwise'] = np.abs(r - r_auto).max() / sr
                    bars['res_vs_pointwise'] = 1e-4
                r_auto = r
                if e['grad_column'] > 2e-5:      # per column: within the bar or within 2 x the fp32 oracle's own deviation there
                    d32 = column_errors(vc.point_grad32(net, transform, act, n), gref)
                    if not all(e_c <= max(2e-5, 2 * d_c) for e_c, d_c in zip(cols, d32)):
                        fails.append((tag, 'grad_column', cols, d32))
            print('points %s %s %s n=%d %s: %s' % (net, transform, act, n, tag, {k: '%.2e' % v for k, v in e.items()}))
            note('points_' + transform, tag, **e)
            if not all(np.all(np.isfinite(o)) for o in outs):
                fails.append((tag, 'non-finite output'))
            fails += [(tag, k, float(e[k]), bars[k]) for k in bars if not e[k] <= bars[k]]
        eng.debug_point_route(False)
        known = POINT_KNOWN_MISSES.get((net, transform, act, n), ((), ''))[0]
        if (fails or known) and transform != 'planted800':
            uk, gk = vc.point_formula(net, transform, act, n)
            yard = np.abs(uk - uref).max() / su
            print('formula restatement: u %.2e grad %.2e' % (yard, np.abs(gk - gref).max() / sg))
            RECORD.setdefault('misses', {})['points %s %s %s %d' % (net, transform, act, n)] = {'fails': [list(f[:3]) for f in fails], 'formula_u': yard}
        if not known:
            assert not fails, fails
            return
        unexpected = [f for f in fails if f[1] != 'u' or f[0] not in known or f[2] > 2.0 * yard]
        unexpected += ['%s no longer misses the bar on u' % t for t in known if t not in {f[0] for f in fails if f[1] == 'u'}]
        if unexpected:
            raise UnexpectedMiss(unexpected)
        raise AssertionError('known miss: %s (formula restatement %.2e)' % (fails, yard))
    finally:
        eng.close()


# -- one optimizer step ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('net,transform,act', [(n, t, a) for n in ('5x50', '3x20') for t in vc.STEP_TRANSFORMS for a in vc.ACTS])
def test_one_adam_step(net, transform, act):
    """One train_step on the auto route and on the de-duplicated route against the fp64 restatement of TF-1 Adam, at the bar of
    test_engine_gpu.test_adam_trajectory_parity (1e-2 relative): the loss the step reports, the loss at the updated parameters,
    and the first-order decrease g . (theta - theta') the update buys.  The decrease weighs each entry's update by its gradient,
    so an entry whose tiny gradient changes sign in fp32 (Adam normalises it to a full step) carries no weight, while eps acting
    at the wrong magnitude under `tiny` (|g| ~ eps / sqrt(1 - beta2)) changes it by a multiple; the fp32 storage of theta puts
    2^-24 |theta| / lr < 1e-4 on it."""
    d_in, dim, widths, q, n_k, td = vc.NETS[net]
    ref0, g0 = vc.oracle(net, transform, act)
    th0 = vc.theta(net, transform).astype(np.float64)
    th_ref, ref1 = vc.adam_step(net, transform, act)
    dec_ref = float(g0 @ (th0 - th_ref))
    assert dec_ref > 0.0
    fails = []
    for route in ('auto', 'dedup'):
        eng = make(net, act, 0, optimizer_name='adam')
        try:
            feed(eng, net, transform)
            if route == 'dedup':
                assert eng.dedup_supported()
                eng.set_dedup(0, *vc.inputs(net, transform)[1])
            loss = torch.zeros(1, device='cuda')
            eng.train_step(0, loss)
            torch.cuda.synchronize()
            assert eng.step == 1
            th1 = eng.get_params().astype(np.float64)
            out, _ = eng.eval_loss(0)
            e = {'loss_before': abs(float(loss[0]) - ref0['loss']) / abs(ref0['loss']),
                 'loss_after': abs(out[0] - ref1['loss']) / abs(ref1['loss']),
                 'decrease': abs(float(g0 @ (th0 - th1)) - dec_ref) / dec_ref}
            print('adam %s %s %s %s: %s' % (net, transform, act, route, {k: '%.2e' % v for k, v in e.items()}))
            note('adam_' + transform, route, **e)
            assert np.all(np.isfinite(th1))
            fails += [(route, k, v) for k, v in e.items() if not v <= 1e-2]
        finally:
            eng.close()
    assert not fails, fails
