"""
Host-side tables of the source-identification tests (vn_set_source_basis, vn_set_source_learn): the ten cases of
tests/dedup_term_cases.py (variant 'all': the three polynomial terms registered next to the source) plus one more, their seeded
basis streams and amplitudes, the fp64 reference of tests/source_ref.py computed once per (case, J) and never modified, and the
bar of the amplitude gradient.  Plain module (no GPU, no pytest marks), shared by tests/test_source_host.py and
tests/test_source_gpu.py.

Cases: 0..9 are tests/dedup_term_cases.CASES -- integ_num 6, 8, 16, 36, 64, 100, 216 and 256, dim 1 to 3, a null and a non-null
s0; nT = 462 (case 6) has nT % 4 == 2, so the one-row-per-thread kernels run there, every other nT is a multiple of 4.  Case 10 is
case 6 cut to its first 76 test functions: nT = 456, a multiple of 4 on the network, tables and streams of the case whose full
size takes the other path (its map keeps all 200 unique points; those that lose their rows become row-less points).

Basis (default_rng(41 + 97 i + J), in the case's own coordinates x = Input[:, :dim] in [-1, 1]^dim): stream j is, by j % 3,
  0  a Gaussian bump exp(-|x - c_j|^2 / (2 s_j^2)), c_j in U(-0.7, 0.7), s_j in U(0.3, 0.8);
  1  a wave sin(k_j . x + p_j), k_j in U(1, 3) per dimension: sign-changing, so the row sum carries cancellation;
  2  a bump times (x_0 - c_j0) / s_j: sign-changing around its own centre
(J = 1: kind 2).  Amplitudes: N(0, 1).  Both rounded to fp32: the engine registers fp32.

J = 3 runs on every case; J of 1, 64 and 5 (mask [1, 0, 1, 0, 0]) on cases 0 and 6 only.

Large-row cases (indices N_CASES + k, tests/test_learnt_gpu.py only; not in PAIRS): the network, unique points, BC/IC rows and
scales of case 8 -- 1D + t, widths [24, 31], the smallest network of the cases -- at the (n_k, q) of BIG, J = 9 with entries 0, 7
and 8 learnt (both sides of the boundary between the stream groups of eight).  nT = 65 538 is just above the 256 x 256 rows a capped
reduction grid takes one row per thread of, and nT % 4 == 2: the one-row kernels, a thread taking up to two rows of a partial.
nT = 262 152 is just above four times that and a multiple of 4: the four-row kernels wrap too.  Their basis seeds are the formula's
own (source 41 + 97 i + 9 = 1117 and 1214, field 83 + 97 i + 9 = 1159 and 1256): with them the fp64 reference leaves no learnt
component on the conditioning floor (least |g64_j| / S_j of the learnt ones: source 0.14 and 0.053, field 0.21 and 0.13, against
COND_FLOOR = 0.01; tests/test_learnt_gpu.py asserts it from the reference before it looks at the device).

The bar, per component j:   |g_j - g64_j| <= GRAD_RTOL * max(|g64_j|, COND_FLOOR * S_j)
with S_j = sum_r |row contribution| (tests/source_ref.py).  The floor may be the binding branch for at most BINDING_FRAC of all
components over all (case, J); tests/test_source_host.py asserts that, and that the reference evaluated in fp32 on the CPU stays
within the bar, from the CPU numbers alone.
"""
import functools

import numpy as np
import torch

from tests import dedup_term_cases as dt
from tests import inverse_ref, source_ref
from tests.parity_cases import GRAD_RTOL

COND_FLOOR = 0.01
BINDING_FRAC = 0.05
N_CASES = len(dt.CASES) + 1
IDS = list(dt.IDS) + ['1d_steady_q6_cut76']
EMPTY = list(dt.EMPTY)
WIDE = [0, 6]                                  # the cases that also run J = 1, 64 and 5
MASK5 = [1, 0, 1, 0, 0]
CUT = 76
# (case, J) of every gradient check
PAIRS = [(i, 3) for i in range(N_CASES)] + [(i, J) for i in WIDE for J in (1, 64, 5)]
BIG_BASE = 8
BIG = [(10923, 6), (43692, 6)]                 # (n_k, q) of the large-row cases N_CASES, N_CASES + 1
BIG_IDS = ['1dt_rows65538', '1dt_rows262152']
BIG_J, BIG_MASK = 9, [1, 0, 0, 0, 0, 0, 0, 1, 1]


def base(i):
    """The case of tests/dedup_term_cases.CASES that case i takes its network, tables and BC/IC rows from."""
    return BIG_BASE if i >= N_CASES else 6 if i == N_CASES - 1 else i


def case(i):
    """The row of tests/dedup_term_cases.CASES, with the case's own n_k (a large-row case: and q)."""
    c = list(dt.CASES[base(i)])
    if i >= N_CASES:
        c[4], c[3] = BIG[i - N_CASES]
    elif i != base(i):
        c[4] = CUT
    return tuple(c)


@functools.lru_cache(maxsize=None)
def inputs(i):
    """The seeded inputs of case i (tests/dedup_term_cases.inputs; case 10: the first CUT test functions of case 6)."""
    if i >= N_CASES:
        return dt.inputs(BIG_BASE, *BIG[i - N_CASES])
    d = dt.inputs(base(i))
    if i == base(i):
        return d
    q = case(i)[3]
    n = CUT * q
    d = dict(d)
    for k in ('uid', 'Input', 'gcoef', 'source', 'rate', 'phi', 'psi'):
        if d[k] is not None:
            d[k] = np.ascontiguousarray(d[k][:n])
    d['rowptr'], d['rowidx'] = dt.csr(d['uid'], d['Xu'].shape[0])
    for k, v in d.items():
        if isinstance(v, np.ndarray) and k != 'w':
            v.setflags(write=False)
    return d


def theta(i):
    return dt.theta(base(i))


def ref_kw(i, dtype=torch.float64):
    return dt.ref_kw(base(i), dtype, d=inputs(i))


def terms_of(i):
    return dt.terms_of(base(i), 'all', inputs(i))


def coefs_of(i):
    return inverse_ref.nine(*terms_of(i))


@functools.lru_cache(maxsize=None)
def basis(i, J):
    """(Phi [J, nT] fp32 stream-major, amp [J] fp32-exact doubles) of case i."""
    dim = case(i)[1]
    x = inputs(i)['Input'][:, :dim].astype(np.float64)
    rng = np.random.default_rng(41 + 97 * i + J)
    Phi = np.empty((J, x.shape[0]), dtype=np.float32)
    for j in range(J):
        c, s = rng.uniform(-0.7, 0.7, dim), rng.uniform(0.3, 0.8)
        k, p = rng.uniform(1.0, 3.0, dim), rng.uniform(0.0, 2.0 * np.pi)
        bump = np.exp(-np.sum((x - c) ** 2, axis=1) / (2.0 * s * s))
        kind = 2 if J == 1 else j % 3
        Phi[j] = (bump, np.sin(x @ k + p), bump * (x[:, 0] - c[0]) / s)[kind]
    amp = rng.standard_normal(J).astype(np.float32).astype(np.float64)
    Phi.setflags(write=False)
    amp.setflags(write=False)
    return Phi, amp


def s0_of(i):
    """The case's own source stream [nT] fp32: zeros when the case has none (the engine then gets a zero stream)."""
    d = inputs(i)
    return np.zeros(d['Input'].shape[0], dtype=np.float32) if d['source'] is None else d['source'].reshape(-1)


def mixed(i, J, amp=None):
    """s0 + Phi^T a in fp64, [nT, 1]."""
    Phi, a = basis(i, J)
    a = a if amp is None else np.asarray(amp, dtype=np.float64)
    return (s0_of(i).astype(np.float64) + a @ Phi.astype(np.float64)).reshape(-1, 1)


def evaluate(i, J, amp=None, dtype=torch.float64):
    Phi, a = basis(i, J)
    nldiff, nlflux, reaction = terms_of(i)
    return source_ref.evaluate(theta(i), case(i)[0], case(i)[2], s0_of(i), Phi.T, a if amp is None else amp, coefs_of(i), nldiff, nlflux,
                               reaction, dtype, **ref_kw(i, dtype))


@functools.lru_cache(maxsize=None)
def reference64(i, J):
    """(loss pieces, theta-gradient, amplitude gradient [J], S [J]) of case i in fp64 at the case's own amplitudes."""
    out = evaluate(i, J)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def bars(g64, S):
    """The allowed |g - g64| per component."""
    return GRAD_RTOL * np.maximum(np.abs(g64), COND_FLOOR * S)
