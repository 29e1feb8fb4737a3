"""GPU tier of the nonlinear-term fuzz (tests/fuzz_terms.py): the reaction term, the flux term, the diffusivity D(u) and the
boundary-flux rows of random cases on every route that can take them -- AUTO, the generic kernels, the tile kernels and the GEMM
form of the layer-by-layer route, the de-duplicated step, vn_objective_f64 -- against the fp64 restatement tests/nldiff_ref.py
(loss 4e-5, gradient 1e-4 globally and per block, lossVec 1e-4; the fp64 objective at 1e-12 / 1e-11) and against each other
(3e-4), with the buffer-growth check on every fourth case.  The bars and the whitelist rule are those of tests/fuzz_routes.py;
that the drawn inputs make a missing term fail them is asserted on the CPU (tests/test_fuzz_terms_host.py).

The worst error per route and quantity is written to fuzz_terms_parity.json in the directory VN_RECORD_DIR names (default:
profile_out/ beside tests/; to be committed as profiles/fuzz_terms_parity.json once measured)."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import fuzz_terms as ft  # noqa: E402

IDS = ['%s%s%d' % ('steady' if st else 'td', '_mor' if mor else '', seed) for seed, n, st, mor in ft.SEED_LISTS]
RECORD = {}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'fuzz_terms_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.mark.parametrize('seed,ncases,steady,mor', ft.SEED_LISTS, ids=IDS)
def test_terms_agree_with_the_reference_on_every_route(seed, ncases, steady, mor):
    bad = []
    whitelisted = 0
    for c in ft.draw_list(seed, ncases, steady, mor):
        r = ft.run_case(c)
        print(r['msg'])
        ft.merge_record(RECORD.setdefault(IDS[ft.SEED_LISTS.index((seed, ncases, steady, mor))], {}), r)
        ft.merge_record(RECORD.setdefault('all', {}), r)
        whitelisted += r['cond'] is not None and r['cond'] > ft.COND_WHITELIST
        if not r['ok']:
            bad.append(r['msg'])
    assert not bad, '\n'.join(bad)
    assert whitelisted <= 1


def test_the_lists_reach_every_route_on_the_device():
    """What the case table of tests/test_fuzz_terms_host.py turns into on the device, from the engines' own kernel_path() and
    dedup_supported() (no step is run): the single-launch 8-wave route, the two-pass route, the generic kernels under AUTO or on
    request, the layer-by-layer route under AUTO, a 7-8 layer net on the fused kernel, the de-duplicated step, and boundary-flux
    rows on each of AUTO, generic and the de-duplicated step."""
    from varnet_amd.engine import VN_KERNEL_FUSED16, VN_KERNEL_GENERIC, VN_KERNEL_LAYERED
    seen = set()
    for c in ft.all_cases():
        eng = ft.fz.make_engine(c['d_in'], c['dim'], c['widths'], c['q'], c['src'], c['iw'], 0, c['act'], c['td'])
        try:
            kp = tuple(eng.kernel_path())
            dedup = ft.shares_points(c) and eng.dedup_supported()
        finally:
            eng.close()
        generic = False
        if ft.in_kernel_range(c):
            try:
                ft.fz.make_engine(c['d_in'], c['dim'], c['widths'], c['q'], c['src'], c['iw'], 1, c['act'], c['td']).close()
                generic = True
            except Exception:
                pass
        seen.add({(VN_KERNEL_FUSED16, 0): 'fused8', (VN_KERNEL_FUSED16, 1): 'twopass', (VN_KERNEL_GENERIC, 0): 'auto_generic',
                  (VN_KERNEL_LAYERED, 0): 'auto_layered'}[kp])
        if kp[0] == VN_KERNEL_FUSED16 and c['L'] >= 7:
            seen.add('deep_fused')
        if kp[0] == VN_KERNEL_LAYERED:
            assert not ft.in_kernel_range(c) or not generic
        seen.update(k for k, v in (('generic', generic), ('dedup', dedup)) if v)
        if c['flux'] and ft.in_kernel_range(c) and kp[0] != VN_KERNEL_LAYERED:
            seen.add('flux_auto')
            seen.update(k for k, v in (('flux_generic', generic), ('flux_dedup', dedup)) if v)
        if dedup and c['terms'].keys() >= {'nlflux', 'nldiff', 'reaction'}:
            seen.add('dedup_all_terms')
    print('reached:', sorted(seen))
    want = {'fused8', 'twopass', 'auto_layered', 'deep_fused', 'generic', 'dedup', 'dedup_all_terms', 'flux_auto', 'flux_generic',
            'flux_dedup'}
    assert want <= seen, sorted(want - seen)
