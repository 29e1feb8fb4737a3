"""GPU tier of the learnt-vector fuzz (tests/fuzz_learnt.py): the five learnt vectors, the periodic pairs, the observations and the
per-test-function weights of random cases on every route that can take them -- AUTO, the generic kernels, both forms of the
layer-by-layer route, the de-duplicated step, vn_objective_f64 -- against the fp64 restatement of the joint problem
tests/joint_ref.py, with the documented refusals, the buffer-growth check and one train step on the AUTO engine.  The bars are
those of tests/fuzz_routes.py, tests/parity_cases.py and tests/bic_cases.py; that the drawn inputs make a missing piece fail them is
asserted on the CPU (tests/test_fuzz_learnt_host.py).

The worst figures per route and per vector are written to fuzz_learnt_parity.json in the directory VN_RECORD_DIR names (default:
profile_out/ beside tests/; committed copy: profiles/fuzz_learnt_parity.json)."""
import json
import os

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import fuzz_learnt as fl  # noqa: E402

IDS = ['%s%s%d' % ('steady' if st else 'td', '_mor' if mor else '', seed) for seed, n, st, mor in fl.SEED_LISTS]
ITEMS = [(k, case) for k, lst in enumerate(fl.SEED_LISTS) for case in range(lst[1])]
RECORD = {}


@pytest.fixture(scope='module', autouse=True)
def _dump_record():
    yield
    out = os.environ.get('VN_RECORD_DIR') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profile_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'fuzz_learnt_parity.json'), 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.mark.parametrize('k, case', ITEMS, ids=['%s-%d' % (IDS[k], case) for k, case in ITEMS])
def test_the_joint_problem_agrees_with_the_reference_on_every_route(k, case):
    c = fl.draw_list(*fl.SEED_LISTS[k])[case]
    r = fl.run_case(c)
    print(r['msg'])
    fl.merge_record(RECORD.setdefault(IDS[k], {}), r)
    fl.merge_record(RECORD.setdefault('all', {}), r)
    assert r['ok'], r['msg']


def test_every_vector_ran_on_every_route_that_carries_it():
    """From what the items above recorded on the device: each learnt vector was carried at least once by AUTO (0), the generic
    kernels (1) and the de-duplicated step (30), and -- the field and the flux / Robin amplitudes excepted, which those routes are
    documented to refuse -- by both forms of the layer-by-layer route (4, 40); the fp64 objective ran too."""
    if 'all' not in RECORD:                      # (run on its own: the cases are run here)
        for k, case in ITEMS:
            fl.merge_record(RECORD.setdefault('all', {}), fl.run_case(fl.draw_list(*fl.SEED_LISTS[k])[case]))
    got = RECORD['all']
    for k in fl.VECTORS:
        want = {0, 1, 30} | (set() if k in ('field', 'fluxbc') else {4, 40})
        assert want <= set(got.get('vector_routes', {}).get(k, [])), (k, got.get('vector_routes'))
    assert '64' in got['routes'] and '30' in got['routes'] and 'grow' in got['routes']
