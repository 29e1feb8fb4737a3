"""
Host-side tables of the boundary-data-identification tests (vn_set_bic_basis, vn_set_bic_learn): the ten cases of
tests/dedup_term_cases.py (variant 'all': the three polynomial terms registered) on their own BC/IC rows, their seeded basis streams
and amplitudes, the fp64 reference of tests/bic_ref.py computed once per (case, J) and never modified, and the bar of the amplitude
gradient.  Plain module (no GPU, no pytest marks), shared by tests/test_bic_host.py and tests/test_bic_gpu.py.

Cases: (nB, bDof) runs from (2, 2) to (40, 22), steady and time-dependent; nB of 31 (case 1) and 2 (case 6) are no multiples of 4,
so the one-row mix kernel runs there; case 5 has bDof = nB.  A steady case evaluates its first bDof rows only.

Basis (the formula of tests/source_cases.basis on x = biInput[:, :dim], default_rng(59 + 97 i + J)): stream j is, by j % 3, a
Gaussian bump, a wave sin(k_j . x + p_j), or a bump times (x_0 - c_j0) / s_j (J = 1: the last).  Every stream runs over all nB rows:
the engine does not know a Dirichlet stream from an initial one.  Amplitudes: N(0, 1).  Both rounded to fp32.

J = 3 runs on every case; J of 1, 64 and 5 (mask [1, 0, 1, 0, 0]) on cases 0 and 6 only.

Large-row cases (indices N_CASES + k, GPU only; not in PAIRS): network, scales, interior rows and polynomial terms of case 8 (1D + t,
widths [24, 31]) with BC/IC rows of their own, (nB, bDof) = (65 538, 40 001) -- just above the 256 x 256 rows a capped reduction
grid takes one row per thread of, nB % 4 == 2 -- and (262 152, 131 076), above four times that and a multiple of 4.  biInput is
U(-1, 1) and label0 N(0, 1) from default_rng(seed), the basis from default_rng(seed + 1), seeds 1038 and 1135; J = 9 with entries 0,
7 and 8 learnt (both sides of the boundary between the stream groups of eight).

The bar, per component j:   |g_j - g64_j| <= GRAD_RTOL * max(|g64_j|, COND_FLOOR * S_j)
with S_j = sum_k |row contribution| (tests/bic_ref.py).  The floor may be the binding branch for at most BINDING_FRAC of all
components over all (case, J); tests/test_bic_host.py asserts that, and that the reference evaluated in fp32 on the CPU stays
within the bar, from the CPU numbers alone.
"""
import functools

import numpy as np
import torch

from tests import bic_ref
from tests import dedup_term_cases as dt
from tests import inverse_ref
from tests.parity_cases import GRAD_RTOL

COND_FLOOR = 0.01
BINDING_FRAC = 0.05
N_CASES = len(dt.CASES)
IDS = list(dt.IDS)
WIDE = [0, 6]                                  # the cases that also run J = 1, 64 and 5
MASK5 = [1, 0, 1, 0, 0]
PAIRS = [(i, 3) for i in range(N_CASES)] + [(i, J) for i in WIDE for J in (1, 64, 5)]
BIG_BASE = 8
BIG = [(65538, 40001), (262152, 131076)]       # (nB, bDof) of the large-row cases N_CASES, N_CASES + 1
BIG_SEEDS = [1038, 1135]
BIG_IDS = ['1dt_bic65538', '1dt_bic262152']
BIG_J, BIG_MASK = 9, [1, 0, 0, 0, 0, 0, 0, 1, 1]


def base(i):
    return BIG_BASE if i >= N_CASES else i


def case(i):
    """The row of tests/dedup_term_cases.CASES, a large-row case with its own (nB, bDof)."""
    c = list(dt.CASES[base(i)])
    if i >= N_CASES:
        c[6], c[7] = BIG[i - N_CASES]
    return tuple(c)


@functools.lru_cache(maxsize=None)
def inputs(i):
    """The seeded inputs of case i (tests/dedup_term_cases.inputs; a large-row case: with its own biInput and biLabel)."""
    d = dt.inputs(base(i))
    if i < N_CASES:
        return d
    nB, d_in = BIG[i - N_CASES][0], case(i)[0]
    rng = np.random.default_rng(BIG_SEEDS[i - N_CASES])
    d = dict(d)
    d['biInput'] = rng.uniform(-1, 1, (nB, d_in)).astype(np.float32)
    d['biLabel'] = rng.standard_normal((nB, 1)).astype(np.float32)
    d['biInput'].setflags(write=False)
    d['biLabel'].setflags(write=False)
    return d


def theta(i):
    return dt.theta(base(i))


def rows(i):
    """The BC/IC rows the loss of case i evaluates: all nB, on a steady problem the first bDof."""
    c = case(i)
    return c[6] if c[10] else c[7]


def ref_kw(i, dtype=torch.float64):
    kw = dt.ref_kw(base(i), dtype, d=inputs(i))
    if i >= N_CASES:
        f = np.float64 if dtype == torch.float64 else np.float32
        kw['biInput'] = inputs(i)['biInput'].astype(f)
        kw['bDof'] = case(i)[7]
    return kw


def terms_of(i):
    return dt.terms_of(base(i), 'all', inputs(i))


def coefs_of(i):
    return inverse_ref.nine(*terms_of(i))


@functools.lru_cache(maxsize=None)
def basis(i, J):
    """(B [J, nB] fp32 stream-major, amp [J] fp32-exact doubles) of case i."""
    dim = case(i)[1]
    x = inputs(i)['biInput'][:, :dim].astype(np.float64)
    rng = np.random.default_rng(BIG_SEEDS[i - N_CASES] + 1 if i >= N_CASES else 59 + 97 * i + J)
    B = np.empty((J, x.shape[0]), dtype=np.float32)
    for j in range(J):
        c, s = rng.uniform(-0.7, 0.7, dim), rng.uniform(0.3, 0.8)
        k, p = rng.uniform(1.0, 3.0, dim), rng.uniform(0.0, 2.0 * np.pi)
        bump = np.exp(-np.sum((x - c) ** 2, axis=1) / (2.0 * s * s))
        kind = 2 if J == 1 else j % 3
        B[j] = (bump, np.sin(x @ k + p), bump * (x[:, 0] - c[0]) / s)[kind]
    amp = rng.standard_normal(J).astype(np.float32).astype(np.float64)
    B.setflags(write=False)
    amp.setflags(write=False)
    return B, amp


def label0_of(i):
    """The case's own labels [nB] fp32."""
    return inputs(i)['biLabel'].reshape(-1)


def mixed(i, J, amp=None):
    """label0 + B^T a in fp64, [nB, 1]."""
    B, a = basis(i, J)
    a = a if amp is None else np.asarray(amp, dtype=np.float64)
    return (label0_of(i).astype(np.float64) + a @ B.astype(np.float64)).reshape(-1, 1)


def fma_mix(i, J, amp):
    """The labels vn_learnt_mix_kernel forms, restated: fp32, from label0, j ascending, one fused multiply-add per stream (the product
    of two fp32 numbers is exact in fp64, so each step is one fp64 addition rounded to fp32)."""
    B = basis(i, J)[0]
    s = label0_of(i).astype(np.float32)
    for j in range(J):
        s = (np.float64(np.float32(amp[j])) * B[j].astype(np.float64) + s.astype(np.float64)).astype(np.float32)
    return s


def evaluate(i, J, amp=None, dtype=torch.float64, flat=None, terms=True):
    """tests/bic_ref.evaluate of case i at the amplitudes amp (default: the case's) and the parameters flat (default: the case's);
    terms=False: the same problem without the three polynomial terms (the batch the single-launch route takes)."""
    B, a = basis(i, J)
    nb = rows(i)
    nldiff, nlflux, reaction = terms_of(i) if terms else (None, None, None)
    return bic_ref.evaluate(theta(i) if flat is None else flat, case(i)[0], case(i)[2], label0_of(i)[:nb], B.T[:nb],
                            a if amp is None else amp, coefs_of(i) if terms else np.array(inverse_ref.OFF), nldiff, nlflux, reaction,
                            dtype, **ref_kw(i, dtype))


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
