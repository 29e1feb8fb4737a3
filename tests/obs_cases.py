"""
The observation sets of the parity cases (tests/test_obs_gpu.py, and the input conditions of tests/test_obs_host.py): the five
shapes of tests/test_periodic_gpu.py::CASES with nO observations in place of its nP pairs, the weight rule, and the fp64
reference of each case, computed once and shared.

Test infrastructure (imported by the tests; not a conftest).
"""
import functools

import numpy as np
import torch

from oracle import tf1_graph as og
from tests import obs_ref
from tests.parity_cases import synth
from tests.test_periodic_gpu import BDV, CASES, IDS, oracle_kw, perturbed

# how each case lays its observations out:
#   'one'    a single observation of one point, with a rowptr
#   'points' point sensors, rowptr None (33: one past a 32-row tile of the generic kernels)
#   'mixed'  segments of 1-7 points
#   'long'   segments of 1-7 points and one of 300 points (ten forward tiles); the point total is made no multiple of 32
LAYOUT = ['one', 'points', 'long', 'mixed', 'mixed']
SEED = 11


def obs_rows(ci, with_dir, plain=False, seed=SEED + 4):
    """The observations of CASES[ci], rounded to fp32 as the engine holds them: q ~ U(0.5,1.5)/len, dir ~ 0.5 N(0,1)/len (with_dir),
    value ~ N(0,1), sigma ~ U(0.5,2) (wgt = 1/sigma^2 formed in fp64).  plain: q and wgt None."""
    d_in, dim, nO = CASES[ci][0], CASES[ci][1], CASES[ci][7]
    rng = np.random.default_rng(seed + 10 * ci)
    lay = LAYOUT[ci]
    if lay in ('one', 'points'):
        lens = np.ones(nO, dtype=np.int64)
    else:
        lens = rng.integers(1, 8, nO)
        if lay == 'long':
            lens[nO // 2] = 300
            if lens.sum() % 32 == 0:
                lens[0] = lens[0] % 7 + 1
            assert lens.sum() % 32 != 0
    n = int(lens.sum())
    per_pt = np.repeat(lens, lens).astype(np.float64)
    o = dict(X=rng.uniform(-1, 1, (n, d_in)).astype(np.float32),
             q=(rng.uniform(0.5, 1.5, n) / per_pt).astype(np.float32),
             dir=(0.5 * rng.standard_normal((n, dim)) / per_pt[:, None]).astype(np.float32),
             value=rng.standard_normal(nO).astype(np.float32),
             wgt=(1.0 / rng.uniform(0.5, 2.0, nO) ** 2).astype(np.float32),
             rowptr=None if lay == 'points' else np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    if not with_dir:
        o['dir'] = None
    if plain:
        o['q'] = o['wgt'] = None
    return o


def case_data(ci):
    d_in, dim, widths, q, n_k, nB, bDof, nO, td, act, integW = CASES[ci]
    return synth(SEED, d_in, dim, widths, q, n_k, nB, bDof, integW=integW)


def reference(ci, flat, d, obs, lam, dtype=torch.float64, periodic=None):
    """obs_ref.loss_and_grad on CASES[ci]: (components with 'obs', gradient)."""
    case = CASES[ci]
    f = np.float64 if dtype == torch.float64 else np.float32
    kw = oracle_kw(case, d, f)
    o = None
    if obs is not None:
        o = {k: (None if v is None else (v if k == 'rowptr' else np.asarray(v).astype(f))) for k, v in obs.items()}
        o['lam'] = lam
    return obs_ref.loss_and_grad(flat.astype(f), case[0], case[2], o, periodic=periodic, dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def ref_of(ci, with_dir, plain=False):
    """(flat, obs, lam, ref, gref, ref0, gref0) of CASES[ci] at the parameters every engine of the parity tests starts from;
    ref0 / gref0: the same without the term.  The weight follows the rule of the issue: lam = (loss without the term) / O,
    rounded to fp32, so that the term is half the loss.  Computed once, shared, unchanged."""
    case = CASES[ci]
    d = case_data(ci)
    obs = obs_rows(ci, with_dir, plain)
    flat = perturbed(og.glorot_init(case[0], case[2], 3))                # = the engine's init_params(seed=3), bit for bit
    ref0, gref0 = reference(ci, flat, d, None, 0.0)
    O = reference(ci, flat, d, obs, 0.0)[0]['obs']
    lam = float(np.float32(ref0['loss'] / O))
    ref, gref = reference(ci, flat, d, obs, lam)
    return flat, obs, lam, ref, gref, ref0, gref0
